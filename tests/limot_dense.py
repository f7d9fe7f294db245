"""The dense float64 restatement of a tick with ball and hinge joints (tests/joint_dense.py) with the hinges' limit / motor rows
added, written from the definitions in include/dmx_batch.h at dmxBatchSetHingeLimots.

Test infrastructure, not a test file.  Everything but the limot row, the angle and the rate is joint_dense's (and lcp_dense's).

  angle  sides (body1, body2) AS GIVEN: q_rel = conj(q_1) q_2 (a world side: the identity), e = q_rel conj(q_0),
         phi = 2 atan2(e_v . axis1, e_w) wrapped into (-pi, pi], theta = -phi; theta_dot = u . (omega_1 - omega_2), u = R_1 axis1
  row    present (fmax > 0 or a finite stop): one row behind the hinge's five, J = [ 0, u | 0, -u ] in the sides as given (both
         blocks change sign in canonical form after an exchange of sides), cfm = the world's, k = erp / h, g = fmax sign(vel);
         limits on = lo_stop <= hi_stop and one of them finite; c, lo, hi by the first line that matches:
             locked (lo_stop == hi_stop)   -k (theta - lo_stop)   -inf     +inf
             theta <= lo_stop              -k (theta - lo_stop)   g        +inf
             theta >= hi_stop              -k (theta - hi_stop)   -inf     g
             fmax > 0                      vel                    -fmax    +fmax
             otherwise                     0                      0        0

With no limots `step` returns exactly what joint_dense.step returns (the same code runs).
"""
import numpy as np

import joint_dense as jd
import lcp_dense as ld

# the fields of dmxHingeLimot (include/dmx_batch.h), in order; batch.HINGE_LIMOT_DTYPE is the C layout of the same
LIMOT_FIELDS = [("lo_stop", np.float64), ("hi_stop", np.float64), ("vel", np.float64), ("fmax", np.float64), ("qrel0", np.float64, (4,))]
LIMOT_DTYPE = np.dtype(LIMOT_FIELDS)
IDENT = np.array([1.0, 0.0, 0.0, 0.0])


def qconj(q):
    return np.array([q[0], -q[1], -q[2], -q[3]])


def qrel(bodies, b1, b2):
    q1 = bodies.quat[b1] if b1 >= 0 else IDENT
    q2 = bodies.quat[b2] if b2 >= 0 else IDENT
    return ld.quat_mul(qconj(q1), q2)


def limot_init(bodies, a):
    """no stops, no motor, and the bodies' current pose as angle zero"""
    l = np.zeros((), LIMOT_DTYPE)
    l["lo_stop"], l["hi_stop"] = -np.inf, np.inf
    l["qrel0"] = qrel(bodies, int(a["body1"]), int(a["body2"]))
    return l


def limots(bodies, art):
    return np.array([limot_init(bodies, a) for a in art], LIMOT_DTYPE)


def angle_of(q1, q2, q0, axis1):
    e = ld.quat_mul(ld.quat_mul(qconj(q1), q2), qconj(q0))
    phi = 2.0 * np.arctan2(e[1:] @ axis1, e[0])
    if phi > np.pi:
        phi -= 2.0 * np.pi
    if phi <= -np.pi:
        phi += 2.0 * np.pi
    return -phi


def angle(bodies, a, l=None):
    """theta of the sides as given; l = None: the zero pose is the identity"""
    b1, b2 = int(a["body1"]), int(a["body2"])
    q1 = bodies.quat[b1] if b1 >= 0 else IDENT
    q2 = bodies.quat[b2] if b2 >= 0 else IDENT
    return angle_of(q1, q2, IDENT if l is None else l["qrel0"], a["axis1"])


def axis_world(bodies, a):
    b1 = int(a["body1"])
    return ld.quat_to_R(bodies.quat[b1]) @ a["axis1"] if b1 >= 0 else np.array(a["axis1"], np.float64)


def rate(bodies, a):
    b1, b2 = int(a["body1"]), int(a["body2"])
    w1 = bodies.avel[b1] if b1 >= 0 else np.zeros(3)
    w2 = bodies.avel[b2] if b2 >= 0 else np.zeros(3)
    return float(axis_world(bodies, a) @ (w1 - w2))


def angles(bodies, art, lim=None):
    """-> (theta [n], theta_dot [n]): 0 for balls and inactive joints"""
    th, thd = np.zeros(len(art)), np.zeros(len(art))
    for (_, k), _, _, _ in jd.canonical_arts(bodies, art):
        if int(art[k]["kind"]) == jd.HINGE:
            th[k] = angle(bodies, art[k], None if lim is None or len(lim) == 0 else lim[k])
            thd[k] = rate(bodies, art[k])
    return th, thd


def present(l):
    return bool(l["fmax"] > 0 or np.isfinite(l["lo_stop"]) or np.isfinite(l["hi_stop"]))


def row_values(theta, l, world):
    """-> (c, lo, hi, line of the table 0..4, |theta - nearest stop| of a limited, unlocked hinge or inf)"""
    k = world.erp / world.h
    lo, hi, vel, fmax = float(l["lo_stop"]), float(l["hi_stop"]), float(l["vel"]), float(l["fmax"])
    limited = lo <= hi and (np.isfinite(lo) or np.isfinite(hi))
    g = fmax * np.sign(vel) if fmax > 0 else 0.0
    margin = min(abs(theta - lo), abs(theta - hi)) if limited and lo != hi else np.inf
    if limited and lo == hi:
        return -k * (theta - lo), -np.inf, np.inf, 0, margin
    if limited and theta <= lo:
        return -k * (theta - lo), g, np.inf, 1, margin
    if limited and theta >= hi:
        return -k * (theta - hi), -np.inf, g, 2, margin
    if fmax > 0:
        return vel, -fmax, fmax, 3, margin
    return 0.0, 0.0, 0.0, 4, margin


def limot_row(bodies, world, loc, nb, b1, b2, a, l, swapped):
    """-> (J, c, lo, hi, line, margin) of a present limot, b1 / b2 the canonical sides"""
    u = axis_world(bodies, a)
    sgn = -1.0 if swapped else 1.0                 # canonical body 1 is the given body 2
    J = np.zeros(6 * nb)
    J[6 * loc[b1] + 3:6 * loc[b1] + 6] = sgn * u
    if b2 >= 0:
        J[6 * loc[b2] + 3:6 * loc[b2] + 6] = -sgn * u
    return (J,) + row_values(angle(bodies, a, l), l, world)


class Island(jd.Island):
    """joint_dense's island with every present limot's row behind its hinge's five"""

    def __init__(self, bodies, world, slots, members, jts, art, lim):
        super().__init__(bodies, world, slots, members, jts, art)
        self.theta_margin = np.inf
        self.limot_rows, self.limot_lines = [], []
        ca = [c for c in members if isinstance(c[0], tuple)]
        loc = {s: k for k, s in enumerate(self.slots)}
        nb = len(self.slots)
        at, ins = 0, []
        for (_, k), b1, b2, swapped in ca:
            hinge = int(art[k]["kind"]) == jd.HINGE
            at += 5 if hinge else 3
            if hinge and present(lim[k]):
                J, c, lo, hi, line, mg = limot_row(bodies, world, loc, nb, b1, b2, art[k], lim[k], swapped)
                ins.append((at + len(ins), J, c, lo, hi))
                self.limot_rows.append(at + len(ins) - 1)
                self.limot_lines.append(line)
                self.theta_margin = min(self.theta_margin, mg)
        if not ins:
            return
        self.J = self.J.reshape(-1, 6 * nb)
        for pos, J, c, lo, hi in ins:
            self.J = np.insert(self.J, pos, J, axis=0)
            self.c = np.insert(self.c, pos, c)
            self.cfm = np.insert(self.cfm, pos, world.cfm)
            self.lo = np.insert(self.lo, pos, lo)
            self.hi = np.insert(self.hi, pos, hi)
            self.row_joint = np.insert(self.row_joint, pos, -1)
            self.row_kind = np.insert(self.row_kind, pos, -1)
        self.n_art_rows += len(ins)
        self.m = len(self.c)
        h = self.h
        self.A = self.J @ self.minv(self.J.T) + np.diag(self.cfm / h)
        self.b = self.c / h - self.J @ (self.v / h + self.minv(self.f))
        self.nu = int(np.sum(np.isinf(self.lo) & np.isinf(self.hi)))
        self.nbd = self.m - self.nu


def step(bodies, world, jts, art=None, lim=None, stepper="quick"):
    """one tick with contact joints `jts`, articulation joints `art` and their limots `lim` (LIMOT_DTYPE, one per joint, or None)
    -> lcp_dense.Result; its islands carry theta_margin, limot_rows and limot_lines"""
    if art is None or len(art) == 0 or lim is None or len(lim) == 0:
        return jd.step(bodies, world, jts, art, stepper)
    assert len(lim) == len(art)
    jts = np.asarray(jts, ld.JOINT_DTYPE) if len(jts) else np.zeros(0, ld.JOINT_DTYPE)
    members = jd.canonical_arts(bodies, art) + ld.canonical(bodies, jts)
    out = bodies.copy()
    isl, lams, infos, margins = [], [], [], []
    h = world.h
    for slots, ms in ld.islands(bodies, members):
        I = Island(bodies, world, slots, ms, jts, art, lim)
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
# scenes shared by the CPU and GPU tests
# lo_stop, hi_stop, vel, fmax of a hinge whose zero pose is its current one (theta = 0): one entry per line of the table, and
# the motor-at-a-stop variants
MODES = {
    "locked": (0.2, 0.2, 0.0, 0.0),
    "low_stop": (0.3, 1.0, 0.0, 0.0),
    "high_stop": (-1.0, -0.3, 0.0, 0.0),
    "motor_free": (-np.inf, np.inf, 2.0, 500.0),
    "motor_saturated": (-np.inf, np.inf, 2.0, 0.05),
    "inside": (-1.0, 1.0, 0.0, 0.0),
    "inside_motor": (-1.0, 1.0, -1.5, 5.0),
    "low_stop_motor_away": (0.3, 1.0, 1.0, 0.5),          # the stop's own push exceeds g: the bound is inactive
    "low_stop_motor_into": (0.3, 1.0, -1.0, 0.5),
    "high_stop_motor_away": (-1.0, -0.3, -1.0, 0.5),
    "low_stop_leaving": (0.01, 1.0, 1.0, 0.5),            # already leaving faster than c: the multiplier sits at g
}
MODE_LINES = {"locked": 0, "low_stop": 1, "high_stop": 2, "motor_free": 3, "motor_saturated": 3, "inside": 4, "inside_motor": 3,
              "low_stop_motor_away": 1, "low_stop_motor_into": 1, "high_stop_motor_away": 2, "low_stop_leaving": 1}


def set_mode(l, mode):
    l["lo_stop"], l["hi_stop"], l["vel"], l["fmax"] = MODES[mode] if isinstance(mode, str) else mode


def one_body(mode, swapped=False, seed=3):
    """one body on a hinge to the world -- given as (body, world) or as (world, body) -- its current pose the zero"""
    rng = np.random.default_rng(seed)
    q = rng.normal(size=4)
    B = ld.Bodies([[0.4, 1.0, -0.2]], [q / np.linalg.norm(q)], [[0.2, -0.1, 0.3]], [[0.5, 1.5, -0.7]], [1.3], [[0.4, 0.7, 0.9]])
    sides = (-1, 0) if swapped else (0, -1)
    art = np.array([jd.from_world(B, jd.HINGE, sides[0], sides[1], (0.0, 1.5, 0.0), (0.2, 1.0, 0.1))], jd.ART_DTYPE)
    lim = limots(B, art)
    set_mode(lim[0], mode)
    return B, art, lim


def two_bodies(mode, kinematic=True, seed=5):
    rng = np.random.default_rng(seed)
    quat = rng.normal(size=(2, 4))
    quat /= np.linalg.norm(quat, axis=1)[:, None]
    B = ld.Bodies([[0.0, 2.0, 0.0], [1.0, 2.2, 0.1]], quat, rng.normal(scale=0.4, size=(2, 3)), rng.normal(scale=0.4, size=(2, 3)),
                  [1.0, 1.7], rng.uniform(0.3, 1.0, (2, 3)))
    if kinematic:
        B.flags[0] |= ld.KINEMATIC
        B.lvel[0], B.avel[0] = (0.5, 0.2, -0.3), (0.0, 1.0, 0.5)
    art = np.array([jd.from_world(B, jd.HINGE, 0, 1, (0.5, 2.1, 0.0), (0.3, 0.2, 1.0))], jd.ART_DTYPE)
    lim = limots(B, art)
    set_mode(lim[0], mode)
    return B, art, lim


def hinge_star(n, seed=0, contacts=False):
    """joint_dense's star round a heavy hub with hinges of random axes for its ball joints; the limots cycle through free motor,
    at the low stop, at the high stop with a weak motor, inside, and saturated motor.  contacts: four frictionless ground
    contacts with leaning normals under the hub, which moves down (test_gpu_joints.star_on_ground's)"""
    B, _ = jd.star(n, seed=seed)
    rng = np.random.default_rng(seed + 100)
    art = np.array([jd.from_world(B, jd.HINGE, k + 1, 0, B.pos[0] + 0.5 * (B.pos[k + 1] - B.pos[0]), rng.normal(size=3)) for k in range(n)],
                   jd.ART_DTYPE)
    B.avel[:] = rng.normal(scale=0.5, size=B.avel.shape)
    lim = limots(B, art)
    for k in range(n):
        m = k % 5
        if m == 0:
            set_mode(lim[k], (-np.inf, np.inf, rng.normal(), 20.0))
        if m == 1:
            set_mode(lim[k], (0.05, 0.5, 0.0, 0.0))
        if m == 2:
            set_mode(lim[k], (-0.5, -0.05, -0.5, 0.3))
        if m == 3:
            set_mode(lim[k], (-0.5, 0.5, 0.0, 0.0))
        if m == 4:
            set_mode(lim[k], (-np.inf, np.inf, 3.0 * rng.normal(), 0.02))
    jts = np.zeros(0, ld.JOINT_DTYPE)
    if contacts:
        B.lvel[0] = (0.0, -1.0, 0.0)
        pts = [(2.0, -0.5, 0.0), (0.0, -0.5, 2.0), (-2.0, -0.5, 0.0), (0.0, -0.5, -2.0)]
        nrm = np.array([(0.5, 1.0, 0.0), (0.0, 1.0, 0.5), (0.0, 1.0, 0.5), (0.5, 1.0, 0.0)])
        nrm /= np.linalg.norm(nrm, axis=1)[:, None]
        jts = np.array([(B.pos[0] + p, n_, 0.01, 0, -1, 0, 0.0, 0, 0, 0, 0) for p, n_ in zip(pts, nrm)], ld.JOINT_DTYPE)
    return B, art, lim, jts


def doors(n, nfree=0, seed=7):
    """n one-hinge doors to the world, the side order alternating, random limots (a third of them at their low stop, half of
    them motorised), then nfree free bodies"""
    rng = np.random.default_rng(seed)
    nt = n + nfree
    pos = np.column_stack([3.0 * np.arange(nt), np.full(nt, 3.0), np.zeros(nt)])
    quat = rng.normal(size=(nt, 4))
    quat /= np.linalg.norm(quat, axis=1)[:, None]
    B = ld.Bodies(pos, quat, rng.normal(scale=0.3, size=(nt, 3)), rng.normal(scale=0.3, size=(nt, 3)), rng.uniform(0.5, 2.0, nt),
                  rng.uniform(0.3, 1.0, (nt, 3)))
    art = np.array([jd.from_world(B, jd.HINGE, k if k % 2 else -1, -1 if k % 2 else k, B.pos[k] + (0.5, 0, 0), rng.normal(size=3))
                    for k in range(n)], jd.ART_DTYPE)
    lim = limots(B, art)
    lim["lo_stop"] = np.where(np.arange(n) % 3 == 0, 0.02, -0.7)
    lim["hi_stop"] = 0.7
    lim["vel"] = rng.normal(size=n)
    lim["fmax"] = np.where(np.arange(n) % 2 == 0, rng.uniform(0.01, 5.0, n), 0.0)
    return B, art, lim


def hinge_limot_chain(rows, seed=0):
    """joint_dense's slowly converging chain with a limot on every hinge, cycling through MODES -- every line of the table, the
    motor-at-a-stop variants included -- and a ball after every second hinge; the zero poses are the poses the joints were made
    at, then every body is disturbed (joint_dense.disturb): |theta| <= 4e-3 rad, 0.006 or more from every stop"""
    plan = jd.plan_rows(rows, [(jd.HINGE, 6), (jd.HINGE, 6), (jd.BALL, 3)])
    B, art = jd.chain([k for k, _ in plan], seed)
    lim = limots(B, art)
    names = list(MODES)
    for n, k in enumerate(k for k, (_, r) in enumerate(plan) if r == 6):
        set_mode(lim[k], names[n % len(names)])
    return jd.disturb(B, seed), art, lim


def small_world(seed=13):
    """48 bodies: 12 two-body pendulums (world - ball - body - hinge with a limot - body), 8 doors, 8 bodies on ground contacts
    and 8 free bodies"""
    rng = np.random.default_rng(seed)
    n = 48
    pos = np.column_stack([3.0 * np.arange(n), np.full(n, 3.0), np.zeros(n)])
    quat = rng.normal(size=(n, 4))
    quat /= np.linalg.norm(quat, axis=1)[:, None]
    B = ld.Bodies(pos, quat, rng.normal(scale=0.3, size=(n, 3)), rng.normal(scale=0.3, size=(n, 3)), rng.uniform(0.5, 2.0, n),
                  rng.uniform(0.3, 1.0, (n, 3)))
    art, modes = [], []
    names = list(MODES)
    for p in range(12):
        a, b = 2 * p, 2 * p + 1
        B.pos[b] = B.pos[a] + (0.0, -1.0, 0.0)
        art.append(jd.from_world(B, jd.BALL, a, -1, B.pos[a] + (0.0, 0.5, 0.0)))
        modes.append(None)
        art.append(jd.from_world(B, jd.HINGE, b, a, B.pos[a] + (0.0, -0.5, 0.0), rng.normal(size=3)))
        modes.append(names[p % len(names)])
    for d in range(8):
        s = 24 + d
        art.append(jd.from_world(B, jd.HINGE, s if d % 2 else -1, -1 if d % 2 else s, B.pos[s] + (0.5, 0, 0), rng.normal(size=3)))
        modes.append(names[(d + 3) % len(names)])
    art = np.array(art, jd.ART_DTYPE)
    lim = limots(B, art)
    for l, m in zip(lim, modes):
        if m is not None:
            set_mode(l, m)
    jts = []
    for s in range(32, 40):
        B.lvel[s] = (0.1, -1.0, 0.0)
        for c in range(1 + s % 3):
            nrm = np.array([0.4 * c, 1.0, 0.3 * (c - 1) * c])
            jts.append((B.pos[s] + (0.3 * c, -0.5, 0.2 * c), nrm / np.linalg.norm(nrm), 0.01, s, -1, 0, 0.0 if c else np.inf, 0, 0, 0, 0))
    return B, art, lim, np.array(jts, ld.JOINT_DTYPE)
