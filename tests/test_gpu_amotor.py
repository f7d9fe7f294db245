"""Angular motors through dmxBatchSetJoints / dmxBatchSetAMotors / dmxBatchStepJoints (both steppers, both precisions, the general
path and the single-launch tick) and dmxBatchAMotorAngles, against the dense float64 reference with AMotor rows
(tests/amotor_dense.py).

Every case uploads a synthetic state, takes one tick and compares it with the reference restarted from the device's own pre-tick
state.  The rules and tolerances are test_gpu_hinge_limot.compare's, unchanged: float64 QuickStep 1e-10 and float64 dWorldStep 1e-8
relative to max(|v_ref|, g h), float32 dWorldStep 10 eps32 kappa(A) asserted <= 1e-3, float32 QuickStep the per-body band of
tests/quick_band.py at K = quick_band.K["joint"] with the old allowance as a second ceiling where the old rule admits the tick
(quick_band.assert_in_old_allowance), every compared tick 1e-3 rad or more from every stop.  A ball's rows carry
quick_band.joint_scales' term as before; an AMotor's rows carry NO term for the prepared angles' rounding: the band does not need
one -- on the device the worst body of this file's 38 float32 QuickStep ticks stood at 2.13 eps32 M_v without it, K = 8 allowing 8
(1.78 with the term S = 2 x D / eps32 + |theta - stop|, D = amotor_dense.MEASURED_DEV's float32 angle figure, which compare still
prints)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import amotor_dense as am
import joint_dense as jd
import lcp_dense as ld
import limot_dense as lm
import quick_band as qb
import slider_dense as sd
from __graft_entry__ import load_package

pkg = load_package()
B_ = pkg.batch
pytestmark = pytest.mark.gpu

H = 1.0 / 60.0
EPS32 = float(np.finfo(np.float32).eps)
PRECS = ["float64", "float32"]
STEPPERS = ["quick", "exact"]
SMALLS = [B_.SMALL_TICK_OFF, B_.SMALL_TICK_AUTO]
EINVAL = -3
THETA_MARGIN = 1e-3
NO_CONTACTS = np.zeros(0, ld.JOINT_DTYPE)


def world(**kw):
    kw.setdefault("cfm", 1e-5)
    return ld.World(**kw)


def to_c(arr, dtype):
    out = np.zeros(len(arr), dtype)
    for f in dtype.names:
        out[f] = arr[f]
    return out


def as_precision(prec, W, jts, art, mot):
    """world parameters, contact, joint and AMotor fields as the device holds them (rounded to float32 in a float32 batch)"""
    if np.dtype(prec).itemsize == 8:
        return W, jts, art, mot
    r = lambda x: float(np.float32(x))
    W2 = ld.World(h=r(W.h), gravity=np.asarray(W.gravity, np.float32).astype(np.float64), erp=r(W.erp), cfm=r(W.cfm),
                  iters=W.iters, sor_w=r(W.sor_w), gyro=W.gyro)
    j2, a2 = jts.copy(), art.copy()
    for f in ("pos", "normal", "depth", "mu", "bounce", "bounce_vel", "soft_erp", "soft_cfm"):
        j2[f] = np.asarray(jts[f], np.float32).astype(np.float64)
    for f in ("anchor1", "anchor2", "axis1", "axis2"):
        a2[f] = np.asarray(art[f], np.float32).astype(np.float64)
    m2 = None
    if mot is not None:
        m2 = mot.copy()
        for f in am.REAL_FIELDS:
            m2[f] = np.asarray(mot[f], np.float32).astype(np.float64)
    return W2, j2, a2, m2


class Run:
    """a batch with a state, a joint set and its AMotors uploaded; tick() steps once and returns (pre-tick Bodies, post state)"""

    def __init__(self, prec, B, W, art, mot, stepper, small=None):
        self.prec, self.B, self.W, self.art, self.mot, self.stepper = prec, B, W, art, mot, stepper
        w = self.w = B_.BatchWorld(B.n, prec, gravity=tuple(W.gravity))
        w.set_erp(W.erp); w.set_cfm(W.cfm); w.set_quickstep(W.iters, W.sor_w); w.set_gyro_mode(W.gyro)
        w.set_stepper(B_.STEPPER_EXACT if stepper == "exact" else B_.STEPPER_QUICK)
        if small is not None:
            w.set_small_tick(small)
        w.upload(B_.POS, B.pos); w.upload(B_.QUAT_RAW, B.quat); w.upload(B_.LVEL, B.lvel); w.upload(B_.AVEL, B.avel)
        w.upload(B_.MASS, B.mass); w.upload(B_.INERTIA, B.inertia)
        w.upload_body_flags(B.flags)
        w.set_joints(to_c(art, B_.JOINT_DTYPE))
        if mot is not None:
            w.set_amotors(to_c(mot, B_.AMOTOR_DTYPE))
        self.mass = w.download(B_.MASS).astype(np.float64).reshape(-1)
        self.inertia = w.download(B_.INERTIA).astype(np.float64)

    def bodies(self, state):
        return ld.Bodies(state[:, 0:3], state[:, 3:7], state[:, 7:10], state[:, 10:13], self.mass, self.inertia, self.B.flags)

    def state(self):
        return self.w.download(B_.STATE).astype(np.float64)

    def tick(self, jts):
        pre = self.state()
        self.w.step_joints(self.W.h, jts.astype(B_.CONTACT_JOINT_DTYPE))
        self.w.synchronize()
        return self.bodies(pre), self.state()

    def close(self):
        self.w.close()


def attach_joint_term(result, bodies, world_, jts, art, mot, amotor_term=False):
    """quick_band.attach_joint_term for a set of balls and AMotors: c_round = (erp / h) S_i per row.  The balls' rows carry
    quick_band.joint_scales' term; an AMotor's rows carry NONE: the band does not need one (see the module's docstring).
    amotor_term = True gives them S = 2 D / eps32 + |theta - stop|, for the record compare prints"""
    jts = np.asarray(jts, ld.JOINT_DTYPE) if len(jts) else np.zeros(0, ld.JOINT_DTYPE)
    members = jd.canonical_arts(bodies, art) + ld.canonical(bodies, jts)
    lim = sd.default_limots(len(art))
    k = world_.erp / world_.h
    D = am.MEASURED_DEV["float32"][0]
    for I, (slots, ms) in zip(result.islands, ld.islands(bodies, members)):
        assert list(slots) == list(I.slots)
        S = []
        for c in ms:
            if not isinstance(c[0], tuple):
                continue
            (_, j), b1, b2, swapped = c
            if int(art[j]["kind"]) != am.AMOTOR:
                S += qb.joint_scales(bodies, world_, art[j], lim[j], b1, b2, swapped)
                continue
            if mot is None:
                continue
            th = am.axes_angles(bodies, art[j], mot[j])[1]
            for i in range(3):
                if not am.present(mot[j], i):
                    continue
                l = am.axis_limot(mot[j], i)
                _, _, _, line, _ = lm.row_values(th[i], l, world_)
                stop = float(l["hi_stop"]) if line == 2 else float(l["lo_stop"])
                S.append(2.0 * D / EPS32 + abs(th[i] - stop) if line <= 2 and amotor_term else 0.0)
        assert len(S) == getattr(I, "n_art_rows", 0), (len(S), getattr(I, "n_art_rows", 0))
        I.c_round = np.concatenate([k * np.array(S, np.float64), np.zeros(I.m - len(S))])
    result._mv_slots = None
    return result


def compare(run, Bp, post, jts):
    """test_gpu_hinge_limot.compare with amotor_dense's reference -> the reference's Result"""
    prec, stepper = run.prec, run.stepper
    Wr, jr, ar, mr = as_precision(prec, run.W, jts, run.art, run.mot)
    r = am.step(Bp, Wr, jr, ar, mr, stepper)
    tm = am.theta_margin(r)
    print(f"{prec} {stepper}: theta margin {tm:.3e}")
    assert tm >= THETA_MARGIN, f"an AMotor axis is {tm:.2e} rad from a stop: too close for two precisions to agree on the row"
    f32 = np.dtype(prec).itemsize == 4
    live = np.nonzero(Bp.flags & ld.ALIVE)[0]
    if f32 and stepper == "quick":
        # for the record, with a term for the prepared angles' rounding on the AMotor rows; asserted without one
        attach_joint_term(r, Bp, Wr, jr, ar, mr, amotor_term=True)
        with_term = float(np.max(qb.deviation(r, post[:, 7:10], post[:, 10:13])[live], initial=0.0))
        attach_joint_term(r, Bp, Wr, jr, ar, mr)
        worst = qb.assert_in_band(r, Wr, post, qb.K["joint"], live)
        used = qb.assert_in_old_allowance(r, Wr, post, live)
        print(f"f32 QuickStep on the device: {worst:.2f} eps32 M_v (K = {qb.K['joint']}); with a term on the AMotor rows {with_term:.2f}; "
              + ("the old rule does not admit the tick" if used is None else f"{used:.3f} of the old allowance"))
        return r
    if not f32:
        t = 1e-10 if stepper == "quick" else 1e-8
    else:
        t = 10 * EPS32 * max([I.kappa() for I in r.islands] + [1.0])
        assert t <= 1e-3, f"float32 tolerance {t:.2e}: too ill-conditioned a case to be a test"
    scale = ld.velocity_scale(r.bodies, Wr, live)
    err = ld.velocity_error(r.bodies, post[:, 7:10], post[:, 10:13], live)
    print(f"{prec} {stepper}: velocity error {err:.3e}, allowed {t:.1e} x {scale:.3e}")
    assert err <= t * scale, f"velocity error {err:.3e} > {t:.1e} x {scale:.3e}"
    eps = 4 * (EPS32 if f32 else 2.2e-16)
    xerr = np.max(np.abs(post[live, 0:3] - r.bodies.pos[live]))
    assert xerr <= t * scale * Wr.h + eps * max(1.0, np.max(np.abs(r.bodies.pos[live]))), f"position error {xerr:.3e}"
    qerr = np.max(np.abs(post[live, 3:7] - r.bodies.quat[live]))
    assert qerr <= t * scale * Wr.h + eps, f"quaternion error {qerr:.3e}"
    return r


def check(prec, B, W, art, mot, stepper, jts=NO_CONTACTS, small=None):
    """-> (the reference's Result, lcp stats, small-tick stats, final state)"""
    run = Run(prec, B, W, art, mot, stepper, small)
    try:
        Bp, post = run.tick(jts)
        r = compare(run, Bp, post, jts)
        return r, run.w.lcp_stats(), run.w.small_tick_stats(), post
    finally:
        run.close()


def path_of(st):
    return (st["small"], st["general"])


# ---------------------------------------------------------------------------------------------------------------------
# 4. one body on a user-mode AMotor to the world: every line of the table on each of three axes
def user_one_body_per_mode(swapped, shift=0, seed=3):
    """one body per entry of limot_dense.MODES, each its own island: a user-mode AMotor to the world with three axes of rel 0, 1, 2,
    the line under test on axis (k + shift) % 3 -- over shift = 0, 1, 2 every line stands on each axis -- (the supplied angle is 0, as the stops of MODES expect) and a weak motor on another axis"""
    rng = np.random.default_rng(seed)
    names = list(lm.MODES)
    n = len(names)
    B = ld.Bodies(np.column_stack([3.0 * np.arange(n), np.ones(n), np.zeros(n)]), am.random_quats(rng, n), rng.normal(scale=0.3, size=(n, 3)),
                  rng.normal(scale=0.8, size=(n, 3)), rng.uniform(0.8, 1.5, n), rng.uniform(0.4, 0.9, (n, 3)))
    art, mot = [], []
    for k, name in enumerate(names):
        b1, b2 = (-1, k) if swapped else (k, -1)
        rel = [0, 2, 1] if swapped else [0, 1, 2]          # (rel 1 / 2 name the given sides: one of them is the world)
        m = am.from_world(B, b1, b2, am.USER, [rng.normal(size=3) for _ in range(3)], rel=[rel[(i + k) % 3] for i in range(3)])
        i = (k + shift) % 3
        m["lo_stop"][i], m["hi_stop"][i], m["vel"][i], m["fmax"][i] = lm.MODES[name]
        j = (i + 1) % 3
        m["vel"][j], m["fmax"][j] = 0.7, 0.02
        art.append(am.joint(b1, b2))
        mot.append(m)
    art, mot = np.array(art, jd.ART_DTYPE), np.array(mot, am.AMOTOR_DTYPE)
    k = names.index("low_stop_leaving")
    i = (k + shift) % 3
    B.avel[k] = 3.0 * am.axes_angles(B, art[k], mot[k])[0][i] * (-1.0 if swapped else 1.0)
    return B, art, mot


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("swapped", [False, True])
@pytest.mark.parametrize("small", SMALLS)
@pytest.mark.parametrize("shift", [0, 1, 2])
def test_one_body_on_a_user_amotor_to_the_world_every_line_of_the_table(prec, stepper, swapped, small, shift):
    """every line of the table (and the motor-at-a-stop variants) on each of the three axes: mode k stands on axis (k + shift) % 3"""
    B, art, mot = user_one_body_per_mode(swapped, shift)
    r, _, st, _ = check(prec, B, world(), art, mot, stepper, small=small)
    names = list(lm.MODES)
    assert [I.m for I in r.islands] == [2] * len(names)
    for k, (I, name) in enumerate(zip(r.islands, names)):
        row = [q for q, (_, i, _) in enumerate(I.amotor_joint) if i == (k + shift) % 3][0]
        assert I.amotor_lines[row] == lm.MODE_LINES[name]
    assert {i for I in r.islands for (_, i, _) in I.amotor_joint} == {0, 1, 2}
    assert path_of(st) == ((1, 0) if small == B_.SMALL_TICK_AUTO else (0, 1))


# ---------------------------------------------------------------------------------------------------------------------
# 5. two bodies, a ball plus an Euler AMotor
EULER_POSES = {
    # name: (the angles the pair stands at, (lo, hi) per axis, (vel, fmax) on the middle axis)
    "inside": ((0.2, -0.3, 0.4), [(-1.0, 1.0)] * 3, (0.0, 0.0)),
    "beyond_axis0": ((0.9, 0.1, -0.2), [(-0.5, 0.5), (-1.0, 1.0), (-1.0, 1.0)], (0.0, 0.0)),
    "beyond_axis1": ((0.1, -0.8, 0.2), [(-1.0, 1.0), (-0.5, 0.5), (-1.0, 1.0)], (0.0, 0.0)),
    "beyond_axis2": ((-0.2, 0.3, 1.1), [(-1.0, 1.0), (-1.0, 1.0), (-0.5, 0.5)], (0.0, 0.0)),
    "two_stops": ((0.8, 0.2, -0.9), [(-0.5, 0.5), (-1.0, 1.0), (-0.5, 0.5)], (0.0, 0.0)),
    "middle_motor": ((0.2, 0.1, -0.1), [(-1.0, 1.0), (-np.inf, np.inf), (-1.0, 1.0)], (1.5, 40.0)),
}
EULER_LINES = {"inside": [4, 4, 4], "beyond_axis0": [2, 4, 4], "beyond_axis1": [4, 1, 4], "beyond_axis2": [4, 4, 2],
               "two_stops": [2, 4, 1], "middle_motor": [4, 3, 4]}


def ball_and_euler(name, kinematic=False, seed=5):
    """two bodies on a ball joint with an Euler AMotor beside it, side 1 turned by the pose's angles from the zero pose"""
    th, stops, (vel, fmax) = EULER_POSES[name]
    rng = np.random.default_rng(seed)
    B = ld.Bodies([[0.0, 2.0, 0.0], [1.0, 2.2, 0.1]], am.random_quats(rng, 2), rng.normal(scale=0.4, size=(2, 3)), rng.normal(scale=0.4, size=(2, 3)),
                  [1.0, 1.7], rng.uniform(0.3, 1.0, (2, 3)))
    if kinematic:
        B.flags[1] |= ld.KINEMATIC
        B.lvel[1], B.avel[1] = (0.5, 0.2, -0.3), (0.0, 1.0, 0.5)
    a0, a2 = am.perpendicular_pair(rng)
    m = am.from_world(B, 0, 1, am.EULER, (a0, a2))
    q = ld.quat_mul(am.compose(a0, a2, th), B.quat[0])
    B.quat[0] = q / np.linalg.norm(q)
    for i, (lo, hi) in enumerate(stops):
        m["lo_stop"][i], m["hi_stop"][i] = lo, hi
    m["vel"][1], m["fmax"][1] = vel, fmax
    art = np.array([jd.from_world(B, jd.BALL, 0, 1, (0.5, 2.1, 0.0)), am.joint(0, 1)], jd.ART_DTYPE)
    mot = am.motors(2)
    mot[1] = m
    return B, art, mot


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("name", list(EULER_POSES))
@pytest.mark.parametrize("small", SMALLS)
def test_ball_plus_euler_amotor(prec, stepper, name, small):
    B, art, mot = ball_and_euler(name)
    r, _, st, _ = check(prec, B, world(), art, mot, stepper, small=small)
    (I,), (lam,) = r.islands, r.lams
    assert I.m == 6 and I.amotor_lines == EULER_LINES[name]
    got = np.array([t for (_, _, t) in I.amotor_joint])
    assert np.max(np.abs(got - EULER_POSES[name][0])) <= 1e-5        # (the pose is the one asked for; float32 inputs)
    for q, line in zip(I.amotor_rows, I.amotor_lines):
        if line == 4:
            assert lam[q] == 0.0                                     # inside all stops: the row does nothing
    assert path_of(st) == ((1, 0) if small == B_.SMALL_TICK_AUTO else (0, 1))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
def test_ball_plus_euler_amotor_one_body_kinematic(prec, stepper):
    B, art, mot = ball_and_euler("two_stops", kinematic=True)
    r, _, _, _ = check(prec, B, world(), art, mot, stepper)
    assert r.islands[0].amotor_lines == EULER_LINES["two_stops"]


# ---------------------------------------------------------------------------------------------------------------------
# 6. dmxBatchAMotorAngles against numpy
@pytest.mark.parametrize("prec", PRECS)
def test_amotor_angles_against_numpy(prec):
    rng = np.random.default_rng(23)
    n = 64
    B = ld.Bodies(rng.normal(size=(2 * n, 3)), am.random_quats(rng, 2 * n), rng.normal(size=(2 * n, 3)), rng.normal(size=(2 * n, 3)),
                  np.ones(2 * n), np.ones((2 * n, 3)))
    art, mot, want = [], [], []
    for k in range(n):
        b1, b2 = 2 * k, 2 * k + 1
        if k % 4 == 3:                                              # user mode: the supplied angles come back
            m = am.from_world(B, b1, b2, am.USER, [rng.normal(size=3) for _ in range(1 + k % 3)], rel=[k % 3, (k + 1) % 3, (k + 2) % 3])
            m["angle"][:int(m["num_axes"])] = rng.uniform(-3, 3, int(m["num_axes"]))
            want.append(np.array(m["angle"]))
        else:
            if k % 4 == 1:
                b2 = -1
            if k % 4 == 2:
                b1, b2 = -1, b1
            a0, a2 = am.perpendicular_pair(rng)
            m = am.from_world(B, b1, b2, am.EULER, (a0, a2))
            th = am.random_angles(rng)
            D = am.compose(a0, a2, th)
            s, D = (b1, D) if b1 >= 0 else (b2, lm.qconj(D))
            q = ld.quat_mul(D, B.quat[s])
            B.quat[s] = q / np.linalg.norm(q)
            want.append(th)
        art.append(am.joint(b1, b2))
        mot.append(m)
    art.append(jd.from_world(B, jd.BALL, 0, 1, (0.0, 0.0, 0.0)))        # another kind: zeros
    art.append(am.joint(3, 3))                                          # inactive: zeros
    art, mot = np.array(art, jd.ART_DTYPE), np.concatenate([np.array(mot, am.AMOTOR_DTYPE), am.motors(2)])
    run = Run(prec, B, world(), art, mot, "quick")
    try:
        th, rate = run.w.amotor_angles()
        Bd = run.bodies(run.state())
    finally:
        run.close()
    _, _, ar, mr = as_precision(prec, world(), NO_CONTACTS, art, mot)
    rth, rrate = am.angles(Bd, ar, mr)
    f32 = np.dtype(prec).itemsize == 4
    print(f"{prec}: worst angle deviation {np.max(np.abs(th - rth)):.3e} (bound {am.angle_bound(prec):.3e}), "
          f"rate {np.max(np.abs(rate - rrate)):.3e}")
    assert np.max(np.abs(th - rth)) <= am.angle_bound(prec)
    # the rate is a_i . (omega_1 - omega_2): the axes' bound times |omega_1 - omega_2|, and the dot product's own rounding
    dw = 2.0 * np.max(np.abs(Bd.avel)) * np.sqrt(3.0)
    assert np.max(np.abs(rate - rrate)) <= am.axis_bound(prec) * dw * 3 + 8 * (EPS32 if f32 else 2.2e-16) * dw
    assert np.array_equal(th[n:], np.zeros((2, 3))) and np.array_equal(rate[n:], np.zeros((2, 3)))
    for k in range(n):
        if k % 4 == 3:
            assert np.array_equal(th[k], np.asarray(mr[k]["angle"]))      # echoed exactly (as the batch holds them)
        else:                                                        # ... and the composition's angles come back
            assert np.max(np.abs(th[k] - want[k])) <= (2e-5 if f32 else 1e-12)


# ---------------------------------------------------------------------------------------------------------------------
# 7. a hanging chain of ball + Euler AMotor links with stops that some links violate, on every solver form
def amotor_chain(rows, seed=0, contacts=False):
    """a chain of bodies, link k on a ball joint to link k - 1 (link 0 to the world) with an Euler AMotor beside it: 3 + 3 rows per
    link, the tail made up with balls to other anchors so that the island has exactly `rows` rows.  Every third link stands beyond a
    stop of one axis, every fifth has a motor on its middle axis; the joints carry errors to correct (joint_dense.disturb)"""
    reserve = 9 if contacts else 0
    links = (rows - reserve) // 6
    extra = rows - reserve - 6 * links                     # 0 or 3: one more ball
    assert extra in (0, 3)
    nb = links + (1 if extra else 0)
    B, balls = jd.chain([jd.BALL] * nb, seed)
    rng = np.random.default_rng(seed + 7)
    art, mot = [], []
    for k in range(links):
        art.append(balls[k])
        mot.append(am.motors(1)[0])
        b2 = k - 1
        a0, a2 = am.perpendicular_pair(rng)
        m = am.from_world(B, k, b2, am.EULER, (a0, a2))
        m["lo_stop"], m["hi_stop"] = -0.5, 0.5
        if k % 3 == 0:                                     # beyond a stop of axis (k // 3) % 3 by 0.05 .. 0.2 rad
            i = (k // 3) % 3
            if k % 2:
                m["hi_stop"][i] = -rng.uniform(0.05, 0.2)
            else:
                m["lo_stop"][i] = rng.uniform(0.05, 0.2)
        if k % 5 == 1:
            m["lo_stop"][1], m["hi_stop"][1], m["vel"][1], m["fmax"][1] = -np.inf, np.inf, rng.normal(), 0.3
        art.append(am.joint(k, b2))
        mot.append(m)
    if extra:
        art.append(balls[links])
        mot.append(am.motors(1)[0])
    jd.disturb(B, seed)
    jts = NO_CONTACTS
    if contacts:
        # three ground contacts with friction under the last link, which moves down and sideways: normal rows loaded, friction at a bound
        s = nb - 1
        B.lvel[s] = (0.6, -1.0, 0.2)
        jl = []
        for c in range(3):
            nrm = np.array([0.3 * c, 1.0, 0.2 * (c - 1)])
            jl.append((B.pos[s] + (0.3 * c, -0.5, 0.2 * c), nrm / np.linalg.norm(nrm), 0.01, s, -1, 0, 0.4, 0, 0, 0, 0))
        jts = np.array(jl, ld.JOINT_DTYPE)
    return B, np.array(art, jd.ART_DTYPE), np.array(mot, am.AMOTOR_DTYPE), jts


def _chain_checks(r, rows):
    (I,), (lam,) = r.islands, r.lams
    assert I.m == rows
    assert {1, 2, 4} <= set(I.amotor_lines) and (rows < 60 or 3 in I.amotor_lines)
    stops = [q for q, line in zip(I.amotor_rows, I.amotor_lines) if line in (1, 2)]
    assert any(lam[q] != 0.0 for q in stops)


QUICK_CHAIN_ROWS = [252, 258, 1020, 1026]


@pytest.mark.parametrize("rows", QUICK_CHAIN_ROWS)
def test_quickstep_chain_either_side_of_the_row_forms_f32(rows):
    """one link (6 rows) either side of 256 rows (one wavefront / registers, 256 threads) and of 1 024 (256 / 512 threads)"""
    B, art, mot, jts = amotor_chain(rows)
    r, _, st, _ = check("float32", B, world(), art, mot, "quick", jts, small=B_.SMALL_TICK_OFF)
    _chain_checks(r, rows)
    assert path_of(st) == (0, 1)


@pytest.mark.parametrize("prec", PRECS)
def test_quickstep_chain_with_ground_contacts_that_clamp(prec):
    B, art, mot, jts = amotor_chain(45, contacts=True)
    r, _, _, _ = check(prec, B, world(), art, mot, "quick", jts, small=B_.SMALL_TICK_OFF)
    (I,), (lam,) = r.islands, r.lams
    assert I.m == 45 and np.any(lam[I.row_kind == 0] > 0)
    fr = np.isfinite(I.hi) & (I.row_kind > 0)
    assert np.any((lam[fr] == I.hi[fr]) | (lam[fr] == I.lo[fr])), "a friction row at a bound"


def child_lane_per_island_chain():
    """(run by test_chain_on_the_lane_per_island_form under DMX_BIG_ISLAND_ROWS=64) 42 rows with the single-launch tick off: swept by
    one lane (row_sor in solve_islands)"""
    assert int(os.environ["DMX_BIG_ISLAND_ROWS"]) == 64
    for prec in PRECS:
        B, art, mot, jts = amotor_chain(42)
        r, _, st, _ = check(prec, B, world(), art, mot, "quick", jts, small=B_.SMALL_TICK_OFF)
        _chain_checks(r, 42)
        assert path_of(st) == (0, 1), st


def test_chain_on_the_lane_per_island_form():
    """DMX_BIG_ISLAND_ROWS is read once per process: a child"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_amotor as t; t.child_lane_per_island_chain(); "
            "print('CHILD-OK')") % (here, os.path.dirname(here))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600,
                       env={**os.environ, "DMX_BIG_ISLAND_ROWS": "64"})
    assert p.returncode == 0 and "CHILD-OK" in p.stdout, (p.stdout[-2000:] + p.stderr[-3000:])


def amotor_star(rows, seed=0):
    """rows / 6 rotated bodies round a heavy hub (joint_dense.star's layout), each on a ball joint to the hub with an Euler AMotor
    beside it, stops and motors as amotor_chain's.  A chain's condition number grows with its length -- at 42 rows float32
    dWorldStep's tolerance 10 eps32 kappa(A) is past the 1e-3 the rule admits -- a star's does not"""
    n = rows // 6
    assert rows == 6 * n
    B, _ = jd.star(n, seed=seed)
    rng = np.random.default_rng(seed + 11)
    B.quat[:] = am.random_quats(rng, n + 1)
    B.avel[:] = rng.normal(scale=0.4, size=B.avel.shape)
    art, mot = [], []
    for k in range(n):
        art.append(jd.from_world(B, jd.BALL, k + 1, 0, 0.5 * (B.pos[0] + B.pos[k + 1])))
        mot.append(am.motors(1)[0])
        a0, a2 = am.perpendicular_pair(rng)
        m = am.from_world(B, k + 1, 0, am.EULER, (a0, a2))
        m["lo_stop"], m["hi_stop"] = -0.5, 0.5
        if k % 3 == 0:
            i = (k // 3) % 3
            if k % 2:
                m["hi_stop"][i] = -rng.uniform(0.05, 0.2)
            else:
                m["lo_stop"][i] = rng.uniform(0.05, 0.2)
        if k % 5 == 1:
            m["lo_stop"][1], m["hi_stop"][1], m["vel"][1], m["fmax"][1] = -np.inf, np.inf, rng.normal(), 0.3
        art.append(am.joint(k + 1, 0))
        mot.append(m)
    jd.disturb(B, seed)
    return B, np.array(art, jd.ART_DTYPE), np.array(mot, am.AMOTOR_DTYPE)


@pytest.mark.parametrize("rows", [42, 198])
def test_dworldstep_chain_in_lds_and_on_the_grid_f64(rows):
    """42 rows: one workgroup, the solve in LDS; 198 rows (192 or more): the grid-wide solve"""
    B, art, mot, jts = amotor_chain(rows)
    r, lcp, st, _ = check("float64", B, world(), art, mot, "exact", jts, small=B_.SMALL_TICK_OFF)
    _chain_checks(r, rows)
    assert path_of(st) == (0, 1)
    assert (lcp["solves"] >= 1) == (rows >= 192), lcp


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("rows", [42, 300])
def test_dworldstep_star_in_lds_and_on_the_grid(prec, rows):
    """the same two forms in both precisions, on islands float32's rule admits (300 rows: past what a workgroup's LDS holds in
    float32 too, where 198 rows still fit)"""
    B, art, mot = amotor_star(rows)
    r, lcp, st, _ = check(prec, B, world(), art, mot, "exact", small=B_.SMALL_TICK_OFF)
    _chain_checks(r, rows)
    assert path_of(st) == (0, 1)
    assert (lcp["solves"] >= 1) == (rows >= 192), lcp


# ---------------------------------------------------------------------------------------------------------------------
# 8. the single-launch tick against the general path bit for bit; feedback; auto-disable
def small_world(seed=13):
    """24 two-link arms (48 bodies): world - ball + Euler AMotor - link - ball + Euler AMotor - link; the first AMotor of every
    second arm is given as (world, body).  A third of the AMotors stand beyond a stop, some have a motor on the middle axis"""
    rng = np.random.default_rng(seed)
    n = 48
    pos = np.column_stack([3.0 * (np.arange(n) // 2), 3.0 - (np.arange(n) % 2), np.zeros(n)])
    B = ld.Bodies(pos, am.random_quats(rng, n), rng.normal(scale=0.3, size=(n, 3)), rng.normal(scale=0.3, size=(n, 3)),
                  rng.uniform(0.5, 2.0, n), rng.uniform(0.3, 1.0, (n, 3)))
    art, mot = [], []
    for p in range(24):
        a, b = 2 * p, 2 * p + 1
        for (b1, b2, anchor) in (((-1, a) if p % 2 else (a, -1)) + (B.pos[a] + (0.0, 0.5, 0.0),), (b, a, B.pos[a] + (0.0, -0.5, 0.0))):
            art.append(jd.from_world(B, jd.BALL, b1, b2, anchor))
            mot.append(am.motors(1)[0])
            a0, a2 = am.perpendicular_pair(rng)
            m = am.from_world(B, b1, b2, am.EULER, (a0, a2))
            m["lo_stop"], m["hi_stop"] = -0.6, 0.6
            k = len(art) // 2
            if k % 3 == 0:
                m["lo_stop"][k % 3] = rng.uniform(0.05, 0.3)
            if k % 3 == 1:
                m["hi_stop"][(k // 3) % 3] = -rng.uniform(0.05, 0.3)
            if k % 4 == 2:
                m["lo_stop"][1], m["hi_stop"][1], m["vel"][1], m["fmax"][1] = -np.inf, np.inf, rng.normal(), 0.5
            art.append(am.joint(b1, b2))
            mot.append(m)
    return B, np.array(art, jd.ART_DTYPE), np.array(mot, am.AMOTOR_DTYPE)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
def test_single_launch_tick_matches_the_general_path_bit_for_bit(prec, stepper):
    B, art, mot = small_world()
    out = {}
    for small in SMALLS:
        run = Run(prec, B, world(), art, mot, stepper, small)
        try:
            run.w.set_feedback(True)
            for t in range(3):
                Bp, post = run.tick(NO_CONTACTS)
                if t == 0:
                    r = compare(run, Bp, post, NO_CONTACTS)
            out[small] = (post, run.w.joint_feedback(), run.w.small_tick_stats())
        finally:
            run.close()
    assert out[B_.SMALL_TICK_AUTO][2]["small"] == 3 and out[B_.SMALL_TICK_OFF][2]["small"] == 0
    assert np.array_equal(out[B_.SMALL_TICK_OFF][0], out[B_.SMALL_TICK_AUTO][0])
    assert np.array_equal(out[B_.SMALL_TICK_OFF][1], out[B_.SMALL_TICK_AUTO][1])
    assert {1, 2, 3, 4} <= {l for I in r.islands for l in I.amotor_lines}


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("small", SMALLS)
def test_feedback_of_an_amotor_at_a_stop(prec, stepper, small):
    """t1 = -t2 = sum lambda_i a_i over the AMotor's rows and zero forces, in the sides as given -- after an exchange too"""
    B, art, mot = small_world()
    run = Run(prec, B, world(), art, mot, stepper, small)
    try:
        run.w.set_feedback(True)
        Bp, post = run.tick(NO_CONTACTS)
        fb = run.w.joint_feedback()
        r = compare(run, Bp, post, NO_CONTACTS)
    finally:
        run.close()
    f32 = np.dtype(prec).itemsize == 4
    want = np.zeros((len(art), 3))
    for I, lam in zip(r.islands, r.lams):
        for q, ax, (k, i, _) in zip(I.amotor_rows, I.amotor_axes, I.amotor_joint):
            want[k] += lam[q] * ax
    scale = max(np.max(np.abs(want)), 1.0)
    tol = (2e-3 if f32 else 1e-7) * scale           # (lambda: the solve's own agreement, as test_gpu_feedback holds it)
    exchanged = loaded = 0
    for k in range(len(art)):
        if int(art[k]["kind"]) != am.AMOTOR:
            continue
        assert np.array_equal(fb[k, 0], np.zeros(3)) and np.array_equal(fb[k, 2], np.zeros(3))      # forces
        b1, b2 = int(art[k]["body1"]), int(art[k]["body2"])
        t1 = want[k] if b1 >= 0 else np.zeros(3)
        t2 = -want[k] if b2 >= 0 else np.zeros(3)
        assert np.max(np.abs(fb[k, 1] - t1)) <= tol and np.max(np.abs(fb[k, 3] - t2)) <= tol, (k, fb[k], want[k])
        if b1 >= 0 and b2 >= 0:
            assert np.array_equal(fb[k, 1], -fb[k, 3])
        exchanged += b1 < 0 and np.any(fb[k, 3] != 0)
        loaded += bool(np.any(want[k] != 0))
    assert exchanged >= 3 and loaded >= 12


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("small", SMALLS)
def test_sleeping_island_with_an_amotor_is_not_stepped(prec, small):
    B, art, mot = ball_and_euler("two_stops")
    B2 = ld.Bodies(np.vstack([B.pos, B.pos + (5.0, 0, 0)]), np.vstack([B.quat, B.quat]), np.vstack([B.lvel, B.lvel]), np.vstack([B.avel, B.avel]),
                   np.concatenate([B.mass, B.mass]), np.vstack([B.inertia, B.inertia]))
    art2 = np.concatenate([art, art])
    art2["body1"][2:], art2["body2"][2:] = 2, 3
    mot2 = np.concatenate([mot, mot])
    A, AD, DIS = B_.BODY_ALIVE, B_.BODY_AUTODISABLE, B_.BODY_DISABLED
    B2.flags[:] = [A | AD | DIS, A | AD | DIS, A, A]
    run = Run(prec, B2, world(), art2, mot2, "quick", small)
    try:
        run.w.set_feedback(True)
        pre = run.state()
        run.w.step_joints(H, NO_CONTACTS.astype(B_.CONTACT_JOINT_DTYPE))
        run.w.synchronize()
        post = run.state()
        fb = run.w.joint_feedback()
        stats = run.w.auto_disable_stats()
    finally:
        run.close()
    assert np.array_equal(post[:2], pre[:2]) and not np.array_equal(post[2:, 7:13], pre[2:, 7:13])
    assert stats["islands_skipped"] == 1
    assert np.array_equal(fb[:2], np.zeros((2, 4, 3))) and np.any(fb[3] != 0)
    # the awake pair moved as the same pair alone moves
    alone = Run(prec, B, world(), art, mot, "quick", small)
    try:
        _, p1 = alone.tick(NO_CONTACTS)
    finally:
        alone.close()
    assert np.array_equal(post[2:, 3:13], p1[:, 3:13])


# ---------------------------------------------------------------------------------------------------------------------
# 9. "changes nothing"
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("small", SMALLS)
def test_amotors_without_a_present_limot_change_nothing(prec, stepper, small):
    """AMotors beside the balls that link the islands anyway, no stop finite and no fmax > 0: bit-identical to the same set with
    inactive joints in their place"""
    B, art, mot = small_world()
    mot["lo_stop"], mot["hi_stop"], mot["fmax"] = -np.inf, np.inf, 0.0
    inactive = art.copy()
    for k in range(len(art)):
        if int(art[k]["kind"]) == am.AMOTOR:
            inactive[k] = jd.from_world(B, jd.BALL, -1, -1, (0.0, 0.0, 0.0))
    out = []
    for a, m in ((art, mot), (inactive, None)):
        run = Run(prec, B, world(), a, m, stepper, small)
        try:
            for _ in range(2):
                _, post = run.tick(NO_CONTACTS)
            out.append(post)
        finally:
            run.close()
    assert np.array_equal(out[0], out[1])


@pytest.mark.parametrize("prec", PRECS)
def test_an_empty_amotor_table_changes_nothing(prec):
    B, art, lim = lm.doors(6, nfree=2)
    out = []
    for empty_call in (False, True):
        w = B_.BatchWorld(B.n, prec)
        try:
            w.upload(B_.POS, B.pos); w.upload(B_.QUAT_RAW, B.quat); w.upload(B_.LVEL, B.lvel); w.upload(B_.AVEL, B.avel)
            w.upload(B_.MASS, B.mass); w.upload(B_.INERTIA, B.inertia); w.upload_body_flags(B.flags)
            w.set_joints(to_c(art, B_.JOINT_DTYPE))
            w.set_hinge_limots(to_c(lim, B_.HINGE_LIMOT_DTYPE))
            if empty_call:
                w.set_amotors(None)
            for _ in range(2):
                w.step_joints(H, NO_CONTACTS.astype(B_.CONTACT_JOINT_DTYPE))
            w.synchronize()
            out.append(w.download(B_.STATE))
        finally:
            w.close()
    assert np.array_equal(out[0], out[1])


# ---------------------------------------------------------------------------------------------------------------------
# 10. refusals
def _bad_motors(mot, k):
    """every refused entry, from a good table"""
    def with_(f):
        m = mot.copy()
        f(m[k])
        return m
    def put(field, value, i=None):
        def f(e):
            if i is None:
                e[field] = value
            else:
                e[field][i] = value
        return f
    yield "mode", with_(put("mode", 2))
    yield "mode", with_(put("mode", -1))
    yield "num_axes", with_(put("num_axes", 0))
    yield "num_axes", with_(put("num_axes", 4))
    yield "euler num_axes", with_(put("num_axes", 2))
    yield "rel", with_(put("rel", 3, 1))
    yield "rel", with_(put("rel", -1, 0))
    yield "axis", with_(lambda e: e["axis"].__setitem__((2, 1), np.nan))
    yield "axis", with_(lambda e: e["axis"].__setitem__((0, 0), np.inf))
    yield "ref", with_(put("ref1", np.inf, 0))
    yield "ref", with_(put("ref2", np.nan, 2))
    yield "angle", with_(put("angle", np.nan, 1))
    yield "vel", with_(put("vel", np.inf, 1))
    yield "fmax", with_(put("fmax", np.nan, 0))
    yield "stop", with_(put("lo_stop", np.nan, 2))
    yield "stop", with_(put("hi_stop", np.nan, 0))


@pytest.mark.parametrize("prec", PRECS)
def test_refusals_leave_state_and_feedback_untouched(prec, capfd):
    B, art, mot = ball_and_euler("two_stops")
    run = Run(prec, B, world(), art, mot, "quick")
    try:
        w = run.w
        w.set_feedback(True)
        run.tick(NO_CONTACTS)
        state, fb = run.state(), w.joint_feedback()
        th = w.amotor_angles()[0]
        good = to_c(mot, B_.AMOTOR_DTYPE)
        capfd.readouterr()
        for n in (1, 3):                                            # n other than 0 or the joint count
            with pytest.raises(B_.DmxError) as e:
                w.set_amotors(np.concatenate([good, good])[:n])
            assert e.value.code == EINVAL
            assert "dmxBatchSetAMotors" in capfd.readouterr().err
        for what, bad in _bad_motors(good, 1):
            with pytest.raises(B_.DmxError) as e:
                w.set_amotors(bad)
            assert e.value.code == EINVAL, what
            err = capfd.readouterr().err
            assert err.count("\n") == 1 and "dmxBatchSetAMotors" in err, (what, err)
        bad_axes = np.array([[1.0, 0, 0], [0, 0, 0], [1.0, 1e-6, 0.0]])
        with pytest.raises(B_.DmxError) as e:                        # Euler axes 0 and 2 not perpendicular
            w.amotor_from_world(0, 1, B_.AMOTOR_EULER, bad_axes)
        assert e.value.code == EINVAL
        # nothing changed: the table still serves the same angles, the state and the last feedback stand
        assert np.array_equal(w.amotor_angles()[0], th)
        assert np.array_equal(run.state(), state) and np.array_equal(w.joint_feedback(), fb)
        # the refusals of a non-empty set apply to AMotors as to every kind
        with pytest.raises(B_.DmxError) as e:
            w.step(H, 1)
        assert e.value.code == EINVAL
        assert np.array_equal(run.state(), state)
    finally:
        run.close()


def test_quickstep_under_the_ode_row_order_refuses_a_set_with_amotors(capfd):
    B, art, mot = ball_and_euler("two_stops")
    run = Run("float64", B, world(), art, mot, "quick")
    try:
        run.w.set_row_order(B_.ORDER_ODE)
        state = run.state()
        with pytest.raises(B_.DmxError) as e:
            run.w.step_joints(H, NO_CONTACTS.astype(B_.CONTACT_JOINT_DTYPE))
        assert e.value.code == EINVAL and "DMX_ORDER_ODE" in capfd.readouterr().err
        assert np.array_equal(run.state(), state)
    finally:
        run.close()


@pytest.mark.parametrize("prec", PRECS)
def test_amotor_from_world_matches_the_reference_record(prec):
    B, art, mot = ball_and_euler("inside")
    run = Run(prec, B, world(), art, mot, "quick")
    try:
        Bd = run.bodies(run.state())
        rng = np.random.default_rng(2)
        a0, a2 = am.perpendicular_pair(rng)
        got = run.w.amotor_from_world(0, 1, B_.AMOTOR_EULER, [a0, (0, 0, 0), a2])
        ref = am.from_world(Bd, 0, 1, am.EULER, (a0, a2))
        # (a float32 batch's quaternions are unit to eps32 only, and two spellings of R(q) differ by that much)
        tol = 1e-14 if np.dtype(prec).itemsize == 8 else 4 * EPS32
        for f in ("axis", "ref1", "ref2"):
            assert np.max(np.abs(got[f] - ref[f])) <= tol, f
        assert int(got["mode"]) == am.EULER and int(got["num_axes"]) == 3
        assert np.all(got["lo_stop"] == -np.inf) and np.all(got["hi_stop"] == np.inf) and not np.any(got["fmax"])
        axes = [rng.normal(size=3) for _ in range(2)]
        got = run.w.amotor_from_world(-1, 1, B_.AMOTOR_USER, axes, rel=(2, 1, 0))
        ref = am.from_world(Bd, -1, 1, am.USER, axes, rel=(2, 1, 0))
        assert np.max(np.abs(got["axis"] - ref["axis"])) <= tol and list(got["rel"]) == [2, 1, 0] and int(got["num_axes"]) == 2
    finally:
        run.close()


# ---------------------------------------------------------------------------------------------------------------------
# an AMotor as the ONLY link between two bodies, none of its limots present: an island of two bodies without a row
def sole_link_pair(seed=9):
    rng = np.random.default_rng(seed)
    B = ld.Bodies([[0.0, 2.0, 0.0], [1.5, 2.2, 0.1], [6.0, 2.0, 0.0]], am.random_quats(rng, 3), rng.normal(scale=0.4, size=(3, 3)),
                  rng.normal(scale=0.4, size=(3, 3)), [1.0, 1.7, 0.8], rng.uniform(0.3, 1.0, (3, 3)))
    m = am.from_world(B, 0, 1, am.EULER, am.perpendicular_pair(rng))          # stops -+inf, fmax 0: no row
    art = np.array([am.joint(0, 1)], jd.ART_DTYPE)
    return B, art, np.array([m], am.AMOTOR_DTYPE)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("small", SMALLS)
def test_rowless_amotor_as_the_only_link_steps_as_the_reference(prec, stepper, small):
    B, art, mot = sole_link_pair()
    r, _, st, _ = check(prec, B, world(), art, mot, stepper, small=small)
    assert [(list(I.slots), I.m) for I in r.islands] == [([0, 1], 0), ([2], 0)]
    assert path_of(st) == ((1, 0) if small == B_.SMALL_TICK_AUTO else (0, 1))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("small", SMALLS)
def test_rowless_amotor_links_its_bodies_for_auto_disable(prec, small):
    """the pair is one island: an awake body wakes its sleeping partner, and a sleeping pair is skipped as ONE island -- with an
    inactive joint in the AMotor's place the partner sleeps on and two islands are skipped"""
    B, art, mot = sole_link_pair()
    A, AD, DIS = B_.BODY_ALIVE, B_.BODY_AUTODISABLE, B_.BODY_DISABLED
    inactive = art.copy()
    inactive["body1"], inactive["body2"] = -1, -1
    got = {}
    for flags in ((A | AD | DIS, A, A), (A | AD | DIS, A | AD | DIS, A)):
        for name, a in (("amotor", art), ("inactive", inactive)):
            B.flags[:] = flags
            run = Run(prec, B, world(), a, mot, "quick", small)
            try:
                pre = run.state()
                run.w.step_joints(H, NO_CONTACTS.astype(B_.CONTACT_JOINT_DTYPE))
                run.w.synchronize()
                got[(flags[1] == A, name)] = (pre, run.state(), run.w.auto_disable_stats(), run.w.body_flags())
            finally:
                run.close()
    pre, post, stats, fl = got[(True, "amotor")]                      # body 1 awake: body 0 is woken and stepped
    assert stats["woken"] == 1 and stats["islands_skipped"] == 0 and not (fl[0] & DIS)
    assert not np.array_equal(post[0, 7:10], pre[0, 7:10])
    pre, post, stats, fl = got[(True, "inactive")]
    assert stats["woken"] == 0 and stats["islands_skipped"] == 1 and (fl[0] & DIS) and np.array_equal(post[0], pre[0])
    pre, post, stats, fl = got[(False, "amotor")]                     # both asleep: one island left out
    assert stats["islands_skipped"] == 1 and np.array_equal(post[:2], pre[:2]) and not np.array_equal(post[2], pre[2])
    assert got[(False, "inactive")][2]["islands_skipped"] == 2


# ---------------------------------------------------------------------------------------------------------------------
# an AMotor in a tick that launches the kernels' APX instantiations (some contact of the tick has friction bounded by the normal force)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("small", SMALLS)
def test_amotor_rows_in_a_tick_with_pyramid_friction(prec, stepper, small):
    """a ball + Euler AMotor pair at two stops with a ground contact under its second body, and a third body on a ground contact of its
    own.  With DMX_CONTACT_APPROX1 on the third body's contacts the whole tick takes the APX kernels: the pair's island -- units and a
    box-friction contact -- must come out bit for bit as in the same tick without the bits, which is held to the reference"""
    B2, art, mot = ball_and_euler("two_stops")
    B = ld.Bodies(np.vstack([B2.pos, [[6.0, 0.5, 0.0]]]), np.vstack([B2.quat, [[1.0, 0, 0, 0]]]), np.vstack([B2.lvel, [[0.8, -1.0, 0.3]]]),
                  np.vstack([B2.avel, [[0.0, 0.0, 0.0]]]), np.concatenate([B2.mass, [1.0]]), np.vstack([B2.inertia, [[1.0, 1.0, 1.0]]]))
    B.lvel[1] = (0.3, -1.0, 0.2)
    jl = [(B.pos[1] + (0.0, -0.5, 0.0), (0.0, 1.0, 0.0), 0.01, 1, -1, 0, 0.4, 0, 0, 0, 0)]
    jl.append((B.pos[2] + (0.0, -0.5, 0.0), (0.0, 1.0, 0.0), 0.01, 2, -1, 0, 0.5, 0, 0, 0, 0))
    plain = np.array(jl, ld.JOINT_DTYPE)
    pyramid = plain.copy()
    pyramid["mode"][1:] = B_.CONTACT_APPROX1
    out = []
    for jts in (plain, pyramid):
        run = Run(prec, B, world(), art, mot, stepper, small)
        try:
            Bp, post = run.tick(jts)
            if jts is plain:
                r = compare(run, Bp, post, jts)
            out.append(post)
        finally:
            run.close()
    assert [I.m for I in r.islands] == [9, 3] and r.islands[0].amotor_lines == EULER_LINES["two_stops"]
    assert np.array_equal(out[0][:2], out[1][:2])
    assert not np.array_equal(out[0][2, 7:13], out[1][2, 7:13])       # (the bits did act on the third body)
