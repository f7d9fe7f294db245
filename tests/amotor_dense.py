"""The dense float64 restatement of a tick with ball and hinge joints (tests/joint_dense.py) with angular motors added, written
from the definitions in include/dmx_batch.h at DMX_JOINT_AMOTOR.

Test infrastructure, not a test file.  Everything but the AMotors' axes, angles, rates and rows is joint_dense's (and lcp_dense's);
the five-line table is limot_dense.row_values.  It shares no code with the product.

  An AMotor is a joint of the set of kind AMOTOR (5) whose anchors, axes and limot entry are ignored; its data is its entry of the
  table `mot` (AMOTOR_DTYPE, one entry per joint).  R_i = side i's rotation, the identity for a world side; sides AS GIVEN.
    user   a_i = axis[i] turned by the side rel[i] names (0 the world, 1 side 1, 2 side 2);  theta_i = angle[i]
    Euler  a_0 = R_1 axis[0], a_2 = R_2 axis[2], a_1 = (a_2 x a_0) / |a_2 x a_0| (0 when that length is 0), r_i = R_i ref_i,
           theta_0 = -atan2(a_2 . (a_0 x r_1), a_2 . r_1),  theta_1 = -atan2(a_2 . a_0, a_2 . (a_0 x a_1)),
           theta_2 = -atan2(r_2 . a_1, r_2 . (a_1 x a_2))
    rows   axis i < num_axes with fmax[i] > 0 or a finite stop: one row, in axis order, J = [ 0, a_i | 0, -a_i ] in the sides as
           given (both blocks change sign in canonical form after an exchange of sides), c, lo, hi from the hinge's table with
           theta_i, cfm = the world's;  rate_i = a_i . (omega_1 - omega_2)
  An AMotor without a present limot makes no row and still links its two bodies into one island.

Hinges here have no limots (the AMotor tests need balls); with no AMotor in the set `step` returns what joint_dense.step returns.
"""
import numpy as np

import joint_dense as jd
import lcp_dense as ld
import limot_dense as lm

AMOTOR = 5
USER, EULER = 0, 1
# the fields of dmxAMotor (include/dmx_batch.h), in order; batch.AMOTOR_DTYPE is the C layout of the same
AMOTOR_FIELDS = [("mode", np.int32), ("num_axes", np.int32), ("rel", np.int32, (3,)), ("pad", np.int32), ("axis", np.float64, (3, 3)),
                 ("ref1", np.float64, (3,)), ("ref2", np.float64, (3,)), ("angle", np.float64, (3,)), ("lo_stop", np.float64, (3,)),
                 ("hi_stop", np.float64, (3,)), ("vel", np.float64, (3,)), ("fmax", np.float64, (3,))]
AMOTOR_DTYPE = np.dtype(AMOTOR_FIELDS)
REAL_FIELDS = ("axis", "ref1", "ref2", "angle", "lo_stop", "hi_stop", "vel", "fmax")


def rot(bodies, s):
    return ld.quat_to_R(bodies.quat[s]) if s >= 0 else np.eye(3)


def joint(b1, b2):
    """the dmxJoint record of an AMotor between b1 and b2 (its anchors and axes are ignored)"""
    a = np.zeros((), jd.ART_DTYPE)
    a["kind"], a["body1"], a["body2"] = AMOTOR, b1, b2
    return a


def blank():
    m = np.zeros((), AMOTOR_DTYPE)
    m["lo_stop"], m["hi_stop"] = -np.inf, np.inf
    return m


def motors(n):
    """n entries without axes, stops or motors: what a joint of another kind carries"""
    m = np.zeros(n, AMOTOR_DTYPE)
    m["num_axes"] = 1
    m["lo_stop"], m["hi_stop"] = -np.inf, np.inf
    return m


def from_world(bodies, b1, b2, mode, axes, rel=(0, 0, 0)):
    """the record of an AMotor from world-frame axes at the bodies' current poses: user mode stores axis i in the frame rel[i]
    names; Euler mode stores axes 0 and 2 in the frames of sides 1 and 2 and takes the pose as angles zero"""
    m = blank()
    axes = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in axes]
    R = (np.eye(3), rot(bodies, b1), rot(bodies, b2))
    m["mode"] = mode
    if mode == EULER:
        a0, a2 = axes[0], axes[-1]
        assert abs(a0 @ a2) <= 1e-9
        m["num_axes"] = 3
        m["rel"] = (1, 0, 2)
        m["axis"][0], m["axis"][2] = R[1].T @ a0, R[2].T @ a2
        m["ref1"], m["ref2"] = R[1].T @ a2, R[2].T @ a0
        return m
    m["num_axes"] = len(axes)
    for i, x in enumerate(axes):
        m["rel"][i] = rel[i]
        m["axis"][i] = R[int(rel[i])].T @ x
    return m


def axes_angles(bodies, a, m):
    """-> (a [3, 3], theta [3]) of the sides as given; unused axes are zero"""
    b1, b2 = int(a["body1"]), int(a["body2"])
    R = (np.eye(3), rot(bodies, b1), rot(bodies, b2))
    A, th = np.zeros((3, 3)), np.zeros(3)
    if int(m["mode"]) == EULER:
        a0, a2 = R[1] @ m["axis"][0], R[2] @ m["axis"][2]
        c = np.cross(a2, a0)
        n = np.linalg.norm(c)
        a1 = c / n if n > 0 else np.zeros(3)
        r1, r2 = R[1] @ m["ref1"], R[2] @ m["ref2"]
        A[:] = a0, a1, a2
        th[0] = -np.arctan2(a2 @ np.cross(a0, r1), a2 @ r1)
        th[1] = -np.arctan2(a2 @ a0, a2 @ np.cross(a0, a1))
        th[2] = -np.arctan2(r2 @ a1, r2 @ np.cross(a1, a2))
        return A, th
    for i in range(int(m["num_axes"])):
        A[i] = R[int(m["rel"][i])] @ m["axis"][i]
        th[i] = m["angle"][i]
    return A, th


def rates(bodies, a, m):
    b1, b2 = int(a["body1"]), int(a["body2"])
    w1 = bodies.avel[b1] if b1 >= 0 else np.zeros(3)
    w2 = bodies.avel[b2] if b2 >= 0 else np.zeros(3)
    return axes_angles(bodies, a, m)[0] @ (w1 - w2)


def angles(bodies, art, mot):
    """-> (theta [n, 3], rate [n, 3]): 0 for other kinds, unused axes and inactive joints"""
    th, rt = np.zeros((len(art), 3)), np.zeros((len(art), 3))
    if mot is None or len(mot) == 0:
        return th, rt
    for (_, k), _, _, _ in jd.canonical_arts(bodies, art):
        if int(art[k]["kind"]) == AMOTOR:
            th[k] = axes_angles(bodies, art[k], mot[k])[1]
            rt[k] = rates(bodies, art[k], mot[k])
    return th, rt


def present(m, i):
    return bool(i < int(m["num_axes"]) and (m["fmax"][i] > 0 or np.isfinite(m["lo_stop"][i]) or np.isfinite(m["hi_stop"][i])))


def axis_limot(m, i):
    l = np.zeros((), lm.LIMOT_DTYPE)
    l["lo_stop"], l["hi_stop"], l["vel"], l["fmax"] = m["lo_stop"][i], m["hi_stop"][i], m["vel"][i], m["fmax"][i]
    return l


def amotor_rows(bodies, world, loc, nb, b1, b2, a, m, swapped):
    """-> list of (axis, J, c, lo, hi, line, margin, theta) of an active AMotor's present axes, b1 / b2 the canonical sides"""
    A, th = axes_angles(bodies, a, m)
    sgn = -1.0 if swapped else 1.0                 # canonical body 1 is the given body 2
    out = []
    for i in range(3):
        if not present(m, i):
            continue
        J = np.zeros(6 * nb)
        J[6 * loc[b1] + 3:6 * loc[b1] + 6] = sgn * A[i]
        if b2 >= 0:
            J[6 * loc[b2] + 3:6 * loc[b2] + 6] = -sgn * A[i]
        out.append((i, J) + lm.row_values(th[i], axis_limot(m, i), world) + (th[i],))
    return out


class Island(jd.Island):
    """joint_dense's island with every AMotor's rows where the set's order puts them"""

    def __init__(self, bodies, world, slots, members, jts, art, mot):
        others = [c for c in members if not (isinstance(c[0], tuple) and int(art[c[0][1]]["kind"]) == AMOTOR)]
        super().__init__(bodies, world, slots, others, jts, art)
        self.theta_margin = np.inf
        self.amotor_rows, self.amotor_lines, self.amotor_axes, self.amotor_joint = [], [], [], []
        ca = [c for c in members if isinstance(c[0], tuple)]
        loc = {s: k for k, s in enumerate(self.slots)}
        nb = len(self.slots)
        self.J = self.J.reshape(-1, 6 * nb)
        at = 0
        for (_, k), b1, b2, swapped in ca:
            kind = int(art[k]["kind"])
            if kind != AMOTOR:
                at += 5 if kind == jd.HINGE else 3
                continue
            if mot is None or len(mot) == 0:
                continue
            for i, J, c, lo, hi, line, mg, th in amotor_rows(bodies, world, loc, nb, b1, b2, art[k], mot[k], swapped):
                self.J = np.insert(self.J, at, J, axis=0)
                self.c = np.insert(self.c, at, c)
                self.cfm = np.insert(self.cfm, at, world.cfm)
                self.lo = np.insert(self.lo, at, lo)
                self.hi = np.insert(self.hi, at, hi)
                self.row_joint = np.insert(self.row_joint, at, -1)
                self.row_kind = np.insert(self.row_kind, at, -1)
                self.amotor_rows.append(at)
                self.amotor_lines.append(line)
                self.amotor_axes.append(J[6 * loc[b1] + 3:6 * loc[b1] + 6] * (-1.0 if swapped else 1.0))
                self.amotor_joint.append((k, i, th))
                self.theta_margin = min(self.theta_margin, mg)
                at += 1
        if not self.amotor_rows:
            return
        self.n_art_rows += len(self.amotor_rows)
        self.m = len(self.c)
        h = self.h
        self.A = self.J @ self.minv(self.J.T) + np.diag(self.cfm / h)
        self.b = self.c / h - self.J @ (self.v / h + self.minv(self.f))
        self.nu = int(np.sum(np.isinf(self.lo) & np.isinf(self.hi)))
        self.nbd = self.m - self.nu


def step(bodies, world, jts, art=None, mot=None, stepper="quick"):
    """one tick with contact joints `jts`, articulation joints `art` (balls, hinges without limots, AMotors) and the AMotors' table
    `mot` (AMOTOR_DTYPE, one per joint, or None) -> lcp_dense.Result; its islands carry theta_margin, amotor_rows, amotor_lines"""
    if art is None or len(art) == 0 or not np.any(art["kind"] == AMOTOR):
        return jd.step(bodies, world, jts, art, stepper)
    assert mot is None or len(mot) == 0 or len(mot) == len(art)
    jts = np.asarray(jts, ld.JOINT_DTYPE) if len(jts) else np.zeros(0, ld.JOINT_DTYPE)
    members = jd.canonical_arts(bodies, art) + ld.canonical(bodies, jts)
    out = bodies.copy()
    isl, lams, infos, margins = [], [], [], []
    h = world.h
    for slots, ms in ld.islands(bodies, members):
        I = Island(bodies, world, slots, ms, jts, art, mot)
        if stepper == "quick":
            lam, margin = I.quickstep(world.iters, world.sor_w)
            info = {}
        else:
            lam, info = I.exact()
            margin = None
        v = I.velocities(lam)
        for k, s in enumerate(slots):
            if bodies.flags[s] & ld.KINEMATIC:
                lv, av = bodies.lvel[s], bodies.avel[s]
            else:
                lv, av = v[6 * k:6 * k + 3], v[6 * k + 3:6 * k + 6]
            out.lvel[s], out.avel[s] = lv, av
            out.pos[s] = bodies.pos[s] + h * lv
            q = bodies.quat[s] + 0.5 * h * ld.quat_mul(np.concatenate([[0.0], av]), bodies.quat[s])
            out.quat[s] = q / np.linalg.norm(q)
        isl.append(I)
        lams.append(lam)
        infos.append(info)
        margins.append(margin)
    return ld.Result(out, isl, lams, infos, margins)


def theta_margin(result):
    return min([getattr(I, "theta_margin", np.inf) for I in result.islands] + [np.inf])


# ---------------------------------------------------------------------------------------------------------------------
# geometry shared by the CPU and GPU tests
def axis_angle_quat(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return np.concatenate([[np.cos(0.5 * angle)], np.sin(0.5 * angle) * axis])


def random_quats(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1)[:, None]


def perpendicular_pair(rng):
    """two random perpendicular unit vectors"""
    a0 = rng.normal(size=3)
    a0 /= np.linalg.norm(a0)
    a2 = np.cross(a0, rng.normal(size=3))
    return a0, a2 / np.linalg.norm(a2)


def compose(a0, a2, th):
    """the quaternion of D = Rot(a_2, th_2) Rot(a_1, th_1) Rot(a_0, th_0), a_1 = a_2 x a_0"""
    a1 = np.cross(a2, a0)
    return ld.quat_mul(axis_angle_quat(a2, th[2]), ld.quat_mul(axis_angle_quat(a1, th[1]), axis_angle_quat(a0, th[0])))


def euler_pair(rng, th, world2=False):
    """two bodies (or a body and the world) at a random zero pose, an Euler AMotor made there, then side 1 turned by compose(th)
    -> (Bodies, joint, motor)"""
    q = random_quats(rng, 2)
    if world2:
        q[1] = (1.0, 0, 0, 0)
    B = ld.Bodies(rng.normal(size=(2, 3)), q, rng.normal(scale=0.4, size=(2, 3)), rng.normal(scale=0.4, size=(2, 3)),
                  rng.uniform(0.5, 2.0, 2), rng.uniform(0.3, 1.0, (2, 3)))
    a0, a2 = perpendicular_pair(rng)
    b2 = -1 if world2 else 1
    m = from_world(B, 0, b2, EULER, (a0, a2))
    qn = ld.quat_mul(compose(a0, a2, th), B.quat[0])
    B.quat[0] = qn / np.linalg.norm(qn)
    return B, joint(0, b2), m


def random_angles(rng, mid=1.2, outer=3.0):
    return np.array([rng.uniform(-outer, outer), rng.uniform(-mid, mid), rng.uniform(-outer, outer)])


# the worst deviation of csrc/dmx_amotor.hpp's amotor_axes, built for the host, from this module over the 2 000 poses of
# tests/test_amotor_harness.py (|theta_1| <= 1.2), as measured there on the CPU: (angles, axes) per precision.  The tests' bounds are
# 4 x these (the margin covers other seeds; the conditioning is bounded by 1 / cos 1.2); DESIGN.md section 5 records them.
MEASURED_DEV = {"float64": (9.437e-16, 9.992e-16), "float32": (3.020e-07, 2.173e-07)}


def angle_bound(prec):
    return 4.0 * MEASURED_DEV[np.dtype(prec).name][0]


def axis_bound(prec):
    return 4.0 * MEASURED_DEV[np.dtype(prec).name][1]
