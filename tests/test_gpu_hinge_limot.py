"""Hinge limits and motors through dmxBatchSetHingeLimots / dmxBatchStepJoints (both steppers, both precisions, the general path
and the single-launch tick) and dmxBatchHingeAngles, against the dense float64 reference with limot rows (tests/limot_dense.py).

The Run / compare shape is test_gpu_joints.py's: every case uploads a synthetic state, a set of joints with limots and a list of
contact joints, takes a tick (or a few) and compares each with the reference restarted from the device's own pre-tick state.
Tolerances are that file's (velocities): float64 QuickStep 1e-10 and float64 dWorldStep 1e-8 relative to max(|v_ref|, g h), float32
dWorldStep 10 eps32 kappa(A) with kappa from the reference, asserted <= 1e-3, float32 QuickStep the per-body band of
tests/quick_band.py with the joint rows' term at K = quick_band.K["joint"] -- no clamp-margin gate: a limot row at its bound is
held like any other (the old allowance stays as a second ceiling where the old rule admits the tick:
quick_band.assert_in_old_allowance).  One condition stays: every compared tick asserts that the reference's hinges are 1e-3 rad or more from
their stops (theta_margin), so that float32 and float64 cannot disagree about which line of the limot's table applies -- that
choice is discontinuous, a clamp is not.  Every float32 QuickStep case is listed in F32_QUICK_CASES (tests/test_quick_band.py runs
the float32 emulation over them); CHAIN_CASES are the ones a dropped sweep cannot pass."""
import numpy as np
import pytest

import joint_dense as jd
import lcp_dense as ld
import limot_dense as lm
import quick_band as qb
from __graft_entry__ import load_package

pkg = load_package()
B_ = pkg.batch
pytestmark = pytest.mark.gpu

H = 1.0 / 60.0
EPS32 = float(np.finfo(np.float32).eps)
PRECS = ["float64", "float32"]
STEPPERS = ["quick", "exact"]
EINVAL = -3
THETA_MARGIN = 1e-3
NO_CONTACTS = np.zeros(0, ld.JOINT_DTYPE)
DEVICE_WORST = {"joint": 0.0}            # the largest device deviation of this process, in eps32 M_v (printed by compare)


def world(**kw):
    kw.setdefault("cfm", 1e-5)
    return ld.World(**kw)


def as_precision(prec, W, jts, art, lim):
    """world parameters, contact, joint and limot fields as the device holds them (rounded to float32 in a float32 batch)"""
    if np.dtype(prec).itemsize == 8:
        return W, jts, art, lim
    r = lambda x: float(np.float32(x))
    W2 = ld.World(h=r(W.h), gravity=np.asarray(W.gravity, np.float32).astype(np.float64), erp=r(W.erp), cfm=r(W.cfm),
                  iters=W.iters, sor_w=r(W.sor_w), gyro=W.gyro)
    j2, a2 = jts.copy(), art.copy()
    for f in ("pos", "normal", "depth", "mu", "bounce", "bounce_vel", "soft_erp", "soft_cfm"):
        j2[f] = np.asarray(jts[f], np.float32).astype(np.float64)
    for f in ("anchor1", "anchor2", "axis1", "axis2"):
        a2[f] = np.asarray(art[f], np.float32).astype(np.float64)
    l2 = None
    if lim is not None:
        l2 = lim.copy()
        for f in lm.LIMOT_DTYPE.names:
            l2[f] = np.asarray(lim[f], np.float32).astype(np.float64)
    return W2, j2, a2, l2


def to_c(arr, dtype):
    out = np.zeros(len(arr), dtype)
    for f in dtype.names:
        out[f] = arr[f]
    return out


class Run:
    """a batch with a state, a joint set and its limots uploaded; tick() steps once and returns (pre-tick Bodies, post state (n, 13))"""

    def __init__(self, prec, B, W, art, lim, stepper, small=None):
        self.prec, self.B, self.W, self.art, self.lim, self.stepper = prec, B, W, art, lim, stepper
        w = self.w = B_.BatchWorld(B.n, prec, gravity=tuple(W.gravity))
        w.set_erp(W.erp); w.set_cfm(W.cfm); w.set_quickstep(W.iters, W.sor_w); w.set_gyro_mode(W.gyro)
        w.set_stepper(B_.STEPPER_EXACT if stepper == "exact" else B_.STEPPER_QUICK)
        if small is not None:
            w.set_small_tick(small)
        w.upload(B_.POS, B.pos); w.upload(B_.QUAT_RAW, B.quat); w.upload(B_.LVEL, B.lvel); w.upload(B_.AVEL, B.avel)
        w.upload(B_.MASS, B.mass); w.upload(B_.INERTIA, B.inertia)
        w.upload_body_flags(B.flags)
        w.set_joints(to_c(art, B_.JOINT_DTYPE))
        if lim is not None:
            w.set_hinge_limots(to_c(lim, B_.HINGE_LIMOT_DTYPE))
        self.mass = w.download(B_.MASS).astype(np.float64).reshape(-1)
        self.inertia = w.download(B_.INERTIA).astype(np.float64)

    def set_limots(self, lim):
        self.lim = lim
        self.w.set_hinge_limots(to_c(lim, B_.HINGE_LIMOT_DTYPE))

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


def compare(run, Bp, post, jts):
    """one device tick against the reference from the same pre-tick state; -> the reference's Result"""
    prec, stepper = run.prec, run.stepper
    Wr, jr, ar, lr = as_precision(prec, run.W, jts, run.art, run.lim)
    r = lm.step(Bp, Wr, jr, ar, lr, stepper)
    tm = lm.theta_margin(r)
    print(f"{prec} {stepper}: theta margin {tm:.3e}")
    assert tm >= THETA_MARGIN, f"a hinge is {tm:.2e} rad from a stop: too close for two precisions to agree on the row"
    f32 = np.dtype(prec).itemsize == 4
    live = np.nonzero(Bp.flags & ld.ALIVE)[0]
    if f32 and stepper == "quick":
        qb.attach_joint_term(r, Bp, Wr, jr, ar, lr)
        worst = qb.assert_in_band(r, Wr, post, qb.K["joint"], live)
        DEVICE_WORST["joint"] = max(DEVICE_WORST["joint"], worst)
        used = qb.assert_in_old_allowance(r, Wr, post, live)
        print(f"f32 QuickStep on the device: {worst:.2f} eps32 M_v (K = {qb.K['joint']}; largest so far {DEVICE_WORST['joint']:.2f}); "
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


def check(prec, B, W, art, lim, stepper, jts=NO_CONTACTS, ticks=1, small=None):
    """-> (the reference's Result per tick, lcp stats, small-tick stats, final state)"""
    run = Run(prec, B, W, art, lim, stepper, small)
    try:
        res = []
        for _ in range(ticks):
            Bp, post = run.tick(jts)
            res.append(compare(run, Bp, post, jts))
        return res, run.w.lcp_stats(), run.w.small_tick_stats(), post
    finally:
        run.close()


# ---------------------------------------------------------------------------------------------------------------------
# scenes
MODE_SEED = 3


def one_body_per_mode(swapped):
    """one body on a hinge to the world per entry of limot_dense.MODES -- every line of the table, the motor-at-a-stop variants
    with the shifted bound inactive (low_stop_motor_away) and active (low_stop_leaving: lo_stop = 0.01 with the body already
    leaving) -- each its own island, 3 apart"""
    parts = [lm.one_body(mode, swapped, seed=MODE_SEED + k) for k, mode in enumerate(lm.MODES)]
    n = len(parts)
    B = ld.Bodies(np.vstack([p[0].pos + (3.0 * k, 0, 0) for k, p in enumerate(parts)]), np.vstack([p[0].quat for p in parts]),
                  np.vstack([p[0].lvel for p in parts]), np.vstack([p[0].avel for p in parts]), np.concatenate([p[0].mass for p in parts]),
                  np.vstack([p[0].inertia for p in parts]))
    art = np.concatenate([p[1] for p in parts])
    for k in range(n):
        side = "body2" if swapped else "body1"
        art[side][k] = k
        art["anchor2" if not swapped else "anchor1"][k] += (3.0 * k, 0, 0)       # (the world side's anchor moves with the body)
    lim = np.concatenate([p[2] for p in parts])
    B.avel[list(lm.MODES).index("low_stop_leaving")] = 3.0 * lm.axis_world(B, art[list(lm.MODES).index("low_stop_leaving")]) * (-1.0 if swapped else 1.0)
    return B, art, lim


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("swapped", [False, True])
@pytest.mark.parametrize("small", [B_.SMALL_TICK_OFF, B_.SMALL_TICK_AUTO])
def test_one_body_on_a_hinge_to_the_world_every_line_of_the_table(prec, stepper, swapped, small):
    """one-body islands of 6 rows, one per line of the table and per motor-at-a-stop variant, given as (body, world) and as
    (world, body), on the general path and on the single-launch tick"""
    B, art, lim = one_body_per_mode(swapped)
    (r,), _, st, _ = check(prec, B, world(), art, lim, stepper, small=small)
    assert [I.m for I in r.islands] == [6] * len(lm.MODES)
    assert [I.limot_lines[0] for I in r.islands] == [lm.MODE_LINES[m] for m in lm.MODES]
    names = list(lm.MODES)
    # the shifted bound g is active in the one, inactive in the other
    k = names.index("low_stop_leaving")
    assert r.lams[k][5] == r.islands[k].lo[5] == 0.5
    k = names.index("low_stop_motor_away")
    assert r.lams[k][5] > r.islands[k].lo[5] == 0.5
    assert (st["small"], st["general"]) == ((1, 0) if small == B_.SMALL_TICK_AUTO else (0, 1))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("mode", ["motor_free", "low_stop_motor_into", "high_stop"])
def test_two_bodies_on_a_hinge_one_of_them_kinematic(prec, stepper, mode):
    B, art, lim = lm.two_bodies(mode, kinematic=True)
    res, _, _, _ = check(prec, B, world(), art, lim, stepper, ticks=2)
    assert res[0].islands[0].m == 6


# (seeds for which the reference meets the float32 QuickStep clamp-margin rule, found on the CPU)
STAR_SEEDS = {8: 0, 40: 3, 100: 1}
STAR_GROUND_SEEDS = {8: 3, 40: 3}


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("n", [8, 40, 100])
def test_star_of_hinges_with_mixed_limots(prec, stepper, n):
    """a heavy hub and n spokes on hinges of random axes, the limots cycling through free motor, at the low stop, at the high stop
    with a weak motor, inside, and saturated motor: 48, 240 and 600 rows -- QuickStep's one-wavefront form (<= 256 rows) and
    workgroup forms, dWorldStep's LDS solve and, past its fit, the grid solve, which must pivot on the limots' bounded rows"""
    B, art, lim, jts = lm.hinge_star(n, seed=STAR_SEEDS[n])
    (r,), st, _, _ = check(prec, B, world(), art, lim, stepper, jts)
    I = r.islands[0]
    assert (I.m, I.nbd) == (6 * n, n) and len(I.limot_rows) == n
    if stepper == "exact":
        # (the LDS solve holds 240 rows of which 40 can clamp in f32 -- 126 KB of its 150 -- and not in f64)
        grid = n == 100 or (n == 40 and prec == "float64")
        assert st["solves"] == (1 if grid else 0)
        if grid:
            info = r.infos[0]
            assert (st["last_m"], st["last_nbd"]) == (I.m, n) and st["last_nu"] == I.m - n
            # (every bounded row of this island is a limot row -- last_nbd == n -- so a second pivoting round on the device means a
            #  limot row changed sides; that some end clamped is the reference's active set, which the compared velocities follow)
            assert info["n_lo"] + info["n_hi"] > 0 and st["rounds"] >= 2, "the grid solve did not pivot on a limot row"


CARRY_TICKS, CARRY_FMAX = 4, 0.03125          # (a float32 number: the reference of a float32 batch sees the same bound)


def toggled_limots(lim0, theta, t):
    """the star's limots for tick t, every stop placed relative to the hinge's angle at the tick's start (0.05 rad or more away).
    The motorised spokes (k % 5 in (0, 4)) toggle: on even ticks a weak motor asked for +-3 rad/s, which saturates at +fmax (k even)
    or -fmax (k odd); on odd ticks the same spoke is at its low stop (k even: hi = +inf) or its high stop (k odd: lo = -inf) with
    that motor -- the bound its row ended the tick before on is not there any more"""
    lim = lim0.copy()
    for k in range(len(lim)):
        m, th = k % 5, theta[k]
        up = k % 2 == 0
        if m in (0, 4):
            if t % 2 == 0:
                lm.set_mode(lim[k], (-np.inf, np.inf, 3.0 if up else -3.0, CARRY_FMAX))
            elif up:
                lm.set_mode(lim[k], (th + 0.05, th + 1.0, 3.0, CARRY_FMAX))
            else:
                lm.set_mode(lim[k], (th - 1.0, th - 0.05, -3.0, CARRY_FMAX))
        if m == 1:
            lm.set_mode(lim[k], (th + 0.05, th + 0.5, 0.0, 0.0))
        if m == 2:
            lm.set_mode(lim[k], (th - 0.5, th - 0.05, -0.5, 0.3))
        if m == 3:
            lm.set_mode(lim[k], (th - 0.5, th + 0.5, 0.0, 0.0))
    return lim


@pytest.mark.parametrize("prec", PRECS)
def test_grid_solve_carries_its_active_set_over_limots_whose_bounds_change(prec):
    """The 100-spoke star under dWorldStep, one island of 600 rows on the grid solve, which starts every tick from the active set
    the rows ended the last one with.  dmxBatchSetHingeLimots per tick turns rows saturated at -fmax / +fmax into high-stop /
    low-stop rows (lo = -inf / hi = +inf) and back: a remembered LO / HI then names a bound that is infinite this tick, and
    clamping there would put an infinity into lambda.  Every tick is compared with the reference"""
    n = 100
    B, art, lim0, jts = lm.hinge_star(n, seed=STAR_SEEDS[n])
    motors = [k for k in range(n) if k % 5 in (0, 4)]
    run = Run(prec, B, world(), art, lim0, "exact")
    try:
        for t in range(CARRY_TICKS):
            theta = run.w.hinge_angles()[0]
            run.set_limots(toggled_limots(lim0, theta, t))
            Bp, post = run.tick(jts)
            r = compare(run, Bp, post, jts)
            I, lam = r.islands[0], r.lams[0]
            rows = dict(zip(range(n), I.limot_rows))
            if t % 2 == 0:
                # the reference's motor rows do end saturated, on the side the next tick takes away
                assert all(lam[rows[k]] == (CARRY_FMAX if k % 2 == 0 else -CARRY_FMAX) for k in motors)
            else:
                assert all((I.lo[rows[k]], I.hi[rows[k]]) == ((CARRY_FMAX, np.inf) if k % 2 == 0 else (-np.inf, -CARRY_FMAX)) for k in motors)
        st = run.w.lcp_stats()
    finally:
        run.close()
    assert st["solves"] == CARRY_TICKS and (st["last_m"], st["last_nbd"]) == (6 * n, n)


@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("prec,n", [("float32", 8), ("float64", 8), ("float64", 40)])
def test_star_of_hinges_on_ground_contacts(prec, stepper, n):
    """the same with four frictionless ground contacts under the hub: limot rows and contact rows clamp in one island
    (kappa ~ 4e2 at 8 spokes: float32 is a test there, and only there)"""
    B, art, lim, jts = lm.hinge_star(n, seed=STAR_GROUND_SEEDS[n], contacts=True)
    (r,), _, _, _ = check(prec, B, world(), art, lim, stepper, jts)
    assert r.islands[0].m == 6 * n + 4


DOORS_SEED = 30          # (the reference meets the float32 QuickStep clamp-margin rule on every one of the 600 islands: found on the CPU)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
def test_600_doors_next_to_free_bodies(prec, stepper):
    """600 one-hinge doors, the side order alternating, random limots, and 40 free bodies: the general path, many small islands"""
    B, art, lim = lm.doors(600, nfree=40, seed=DOORS_SEED)
    res, _, st, _ = check(prec, B, world(), art, lim, stepper)
    ms = sorted(I.m for I in res[0].islands)
    assert ms.count(6) == 600 and ms.count(0) == 40 and st["general"] == 1


# ---------------------------------------------------------------------------------------------------------------------
# Chains a wrong sweep cannot pass (limot_dense.hinge_limot_chain: rotated bodies, errors to correct, a limot on every hinge over
# every line of the table), one island each: 40 rows on the single-launch tick, and on either side of the boundary between the
# 256-thread and the 512-thread register form of float32 QuickStep (csrc/dmx_islands.hip: big_max_rows > 1 024).  Limot rows at
# their bounds are held to the band like the rest.
CHAIN_CASES = ["hinge_limot_chain-40", "hinge_limot_chain-1024", "hinge_limot_chain-1028"]
FORM_CASES = {"single-launch tick": ["hinge_limot_chain-40"], "registers, 256 threads": ["hinge_limot_chain-1024"],
              "registers, 512 threads": ["hinge_limot_chain-1028"]}


@pytest.mark.parametrize("rows", [40, 1024, 1028])
def test_quickstep_chain_of_hinges_with_limots_f32(rows):
    B, art, lim = lm.hinge_limot_chain(rows)
    (r,), _, st, _ = check("float32", B, world(), art, lim, "quick", small=B_.SMALL_TICK_AUTO)
    (I,), (lam,) = r.islands, r.lams
    assert I.m == rows and set(I.limot_lines) == ({0, 1, 2, 3} if rows == 40 else {0, 1, 2, 3, 4})      # (40 rows: four limots)
    at = [k for k in I.limot_rows if np.isfinite(I.lo[k]) or np.isfinite(I.hi[k])]
    assert any(lam[k] in (I.lo[k], I.hi[k]) for k in at) and any(lam[k] not in (I.lo[k], I.hi[k]) for k in at)
    assert (st["small"], st["general"]) == ((1, 0) if rows <= 256 else (0, 1)), st


# every float32 QuickStep case `compare` sees: name -> () -> (Bodies, World, contact joints, joints, limots, ticks[, before(t, limots)]).
# tests/test_quick_band.py runs the float32 emulation of a float32 batch's rows and sweeps over them (quick_band.MEASURED["joint"])
def _case(B, art, lim, jts=NO_CONTACTS, ticks=1):
    return B, world(), jts, art, lim, ticks


def _motor_door_case():
    B, art, lim, W = motor_door()

    def before(t, lim):
        lim["vel"][0] = motor_vel(t)
    return B, W, NO_CONTACTS, art, lim, MOTOR_TICKS, before


F32_QUICK_CASES = {
    "one_body_per_mode": lambda: _case(*one_body_per_mode(False)),
    "one_body_per_mode-swapped": lambda: _case(*one_body_per_mode(True)),
    "star_on_ground-8": lambda: _case(*lm.hinge_star(8, seed=STAR_GROUND_SEEDS[8], contacts=True)),
    "doors": lambda: _case(*lm.doors(600, nfree=40, seed=DOORS_SEED)),
    "motor_door": lambda: _motor_door_case(),
}
for _mode in ("motor_free", "low_stop_motor_into", "high_stop"):
    F32_QUICK_CASES[f"two_bodies-{_mode}"] = lambda mode=_mode: _case(*lm.two_bodies(mode, kinematic=True), ticks=2)
for _n in (8, 40, 100):
    F32_QUICK_CASES[f"hinge_star-{_n}"] = lambda n=_n: _case(*lm.hinge_star(n, seed=STAR_SEEDS[n]))
for _rows in (40, 1024, 1028):
    F32_QUICK_CASES[f"hinge_limot_chain-{_rows}"] = lambda rows=_rows: _case(*lm.hinge_limot_chain(rows))


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
def test_small_tick_and_general_path_agree_bit_for_bit(prec, stepper):
    B, art, lim, jts = lm.small_world()
    assert B.n == 48
    out = {}
    for mode in (B_.SMALL_TICK_OFF, B_.SMALL_TICK_AUTO):
        run = Run(prec, B, world(), art, lim, stepper, small=mode)
        try:
            for _ in range(3):
                _, post = run.tick(jts)
            out[mode] = (post, run.w.small_tick_stats())
        finally:
            run.close()
    assert out[B_.SMALL_TICK_AUTO][1]["small"] == 3 and out[B_.SMALL_TICK_AUTO][1]["general"] == 0
    assert out[B_.SMALL_TICK_OFF][1]["small"] == 0
    assert np.array_equal(out[B_.SMALL_TICK_OFF][0], out[B_.SMALL_TICK_AUTO][0])


# ---------------------------------------------------------------------------------------------------------------------
MOTOR_TICKS, MOTOR_HI, MOTOR_FMAX, MOTOR_CFM = 120, 0.5, 60.0, 1e-3


def motor_vel(t):
    """the controller: what the limot's vel is replaced with before tick t"""
    return 1.0 + 0.25 * np.sin(0.3 * t)


def motor_door():
    """a door of mass 4 whose centre is 1 from a horizontal hinge to the world, its arm level at angle zero, stops at -0.5 and
    MOTOR_HI, a motor of MOTOR_FMAX.  Gravity turns it the way the motor does, and goes on pressing it against the stop: the
    row's multiplier there is minus that load (the motor's own torque is inside the bound g, not in the multiplier), and with
    the world's CFM at 1e-3 the door rests cfm m g r cos(0.5) / k = 2.9e-3 rad past the stop -- every tick of the run starts
    1e-3 rad or more from it"""
    q = np.array([0.9, 0.1, -0.3, 0.2])
    B = ld.Bodies([[1.0, 2.0, 0.0]], [q / np.linalg.norm(q)], [[0.0, 0.0, 0.0]], [[0.0, 0.0, 0.0]], [4.0], [[0.5, 0.7, 0.6]])
    art = np.array([jd.from_world(B, jd.HINGE, 0, -1, (0.0, 2.0, 0.0), (0.0, 0.0, -1.0))], jd.ART_DTYPE)
    lim = lm.limots(B, art)
    lm.set_mode(lim[0], (-0.5, MOTOR_HI, motor_vel(0), MOTOR_FMAX))
    return B, art, lim, world(cfm=MOTOR_CFM)


def reference_motor_run(stepper):
    """-> (the reference's largest theta - hi_stop over a reference-only run, its smallest theta margin)"""
    B, art, lim, W = motor_door()
    over, tm = 0.0, np.inf
    for t in range(MOTOR_TICKS):
        lim["vel"][0] = motor_vel(t)
        r = lm.step(B, W, NO_CONTACTS, art, lim, stepper)
        tm = min(tm, lm.theta_margin(r))
        B = r.bodies
        over = max(over, lm.angle(B, art[0], lim[0]) - MOTOR_HI)
    return over, tm


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
def test_motor_drives_a_door_into_its_stop_and_holds_it_there(prec, stepper):
    """120 ticks: the motor, its vel replaced every tick (dmxBatchSetHingeLimots per tick), drives the door from 0 to its high stop
    at 0.5 and holds it there.  Every tick is compared with the reference restarted from the device's pre-tick state; the
    largest overshoot past the stop (dmxBatchHingeAngles) stays within twice the reference's own over a reference-only run --
    the margin the chain-drift test of test_gpu_joints.py uses for joint errors."""
    ref_over, ref_tm = reference_motor_run(stepper)
    assert ref_over > 0 and ref_tm >= 1.5 * THETA_MARGIN, (ref_over, ref_tm)
    B, art, lim, W = motor_door()
    run = Run(prec, B, W, art, lim, stepper)
    try:
        over, lines = 0.0, []
        for t in range(MOTOR_TICKS):
            lim["vel"][0] = motor_vel(t)
            run.set_limots(lim)
            Bp, post = run.tick(NO_CONTACTS)
            r = compare(run, Bp, post, NO_CONTACTS)
            lines.append(r.islands[0].limot_lines[0])
            over = max(over, run.w.hinge_angles()[0][0] - MOTOR_HI)
    finally:
        run.close()
    print(f"{prec} {stepper}: largest overshoot {over:.4e}, the reference's {ref_over:.4e}")
    assert lines[0] == 3 and lines[-1] == 2 and lines.count(2) > MOTOR_TICKS // 2
    assert over <= 2 * ref_over


# ---------------------------------------------------------------------------------------------------------------------
def random_joints(n=1000, nb=64, seed=17):
    """n joints between nb bodies with random poses and spins: hinges and balls, some inactive, some given as (world, body), random
    zero poses -- and every tenth hinge's zero pose chosen so that its angle is within 1e-3 of +-pi"""
    rng = np.random.default_rng(seed)
    quat = rng.normal(size=(nb, 4))
    quat /= np.linalg.norm(quat, axis=1)[:, None]
    B = ld.Bodies(rng.normal(scale=3.0, size=(nb, 3)), quat, rng.normal(size=(nb, 3)), rng.normal(scale=2.0, size=(nb, 3)), np.ones(nb), np.ones((nb, 3)))
    B.flags[5] = 0                                   # a dead slot: its joints are inactive
    art = jd.arts(n)
    lim = np.zeros(n, lm.LIMOT_DTYPE)
    for k in range(n):
        b1, b2 = (int(x) for x in rng.integers(0, nb, 2))
        form = k % 7
        if form == 1:
            b1 = -1                                  # (world, body)
        if form == 2:
            b2 = -1
        if form == 3 and k % 21 == 3:
            b1 = b2 = -1                             # inactive
        if form == 4 and k % 28 == 4:
            b2 = b1                                  # inactive
        art[k] = jd.from_world(B, jd.BALL if form == 5 else jd.HINGE, b1, b2, rng.normal(size=3), rng.normal(size=3))
        q0 = rng.normal(size=4)
        lim[k]["qrel0"] = q0 / np.linalg.norm(q0)
        if k % 10 == 0:
            # theta = +-(pi - d): q_0 = conj(rot(axis1, -+(pi - d))) applied to the current relative pose
            d = rng.uniform(0.0, 1e-3) * (1 if k % 20 else -1)
            a = -(np.pi - d)
            turn = np.concatenate([[np.cos(0.5 * a)], np.sin(0.5 * a) * art[k]["axis1"]])
            lim[k]["qrel0"] = ld.quat_mul(lm.qconj(turn), lm.qrel(B, b1, b2))
    lim["lo_stop"], lim["hi_stop"] = -np.inf, np.inf
    return B, art, lim


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("with_limots", [True, False])
def test_hinge_angles_against_numpy(prec, with_limots):
    B, art, lim = random_joints()
    run = Run(prec, B, world(), art, lim if with_limots else None, "quick")
    try:
        th, thd = run.w.hinge_angles()
        state = run.state()
    finally:
        run.close()
    _, _, ar, lr = as_precision(prec, run.W, NO_CONTACTS, art, lim)
    rt, rd = lm.angles(run.bodies(state), ar, lr if with_limots else None)
    eps = EPS32 if prec == "float32" else 2.2e-16
    d = (th - rt + np.pi) % (2 * np.pi) - np.pi
    print(f"{prec}: angle error {np.max(np.abs(d)):.3e} ({np.max(np.abs(d)) / eps:.1f} eps), rate error {np.max(np.abs(thd - rd)):.3e}")
    assert np.max(np.abs(d)) <= 32 * eps
    assert np.max(np.abs(thd - rd)) <= 32 * eps * np.max(np.abs(state[:, 10:13]))
    hinge = art["kind"] == jd.HINGE
    active = np.array([k for (_, k), *_ in jd.canonical_arts(run.bodies(state), art)])
    off = np.ones(len(art), bool)
    off[active] = False
    assert np.all(th[~hinge] == 0) and np.all(thd[~hinge] == 0) and np.all(th[off] == 0) and np.all(thd[off] == 0) and off.sum() > 20
    if with_limots:
        near = np.abs(np.abs(rt) - np.pi) < 1e-3
        assert near.sum() >= 50 and np.any(rt[near] > 0) and np.any(rt[near] < 0)


# ---------------------------------------------------------------------------------------------------------------------
def test_api_refuses_what_it_must_and_set_joints_drops_the_limots():
    B, art, lim = lm.two_bodies("motor_free", kinematic=False)
    run = Run("float64", B, world(), art, lim, "quick")
    w = run.w
    try:
        def refused(l):
            with pytest.raises(B_.DmxError) as e:
                w.set_hinge_limots(to_c(l, B_.HINGE_LIMOT_DTYPE))
            assert e.value.code == EINVAL
        refused(np.concatenate([lim, lim]))                          # n is neither 0 nor the joint count
        for f, v in (("vel", np.inf), ("vel", np.nan), ("fmax", -np.inf), ("fmax", np.nan), ("lo_stop", np.nan), ("hi_stop", np.nan)):
            bad = lim.copy()
            bad[f] = v
            refused(bad)
        got = w.hinge_limot_init(to_c(art, B_.JOINT_DTYPE)[0])
        assert np.max(np.abs(got["qrel0"] - lm.limot_init(B, art[0])["qrel0"])) <= 1e-15
        assert (got["lo_stop"], got["hi_stop"], got["vel"], got["fmax"]) == (-np.inf, np.inf, 0.0, 0.0)
        th0 = w.hinge_angles()[0][0]
        assert abs(th0) <= 1e-15                                      # the zero pose is the current one
        w.set_joints(to_c(art, B_.JOINT_DTYPE))                      # drops the limots: the angle is relative to the identity again
        assert abs(w.hinge_angles()[0][0] - lm.angle(B, art[0], None)) <= 1e-14 and abs(lm.angle(B, art[0], None)) > 0.1
        Bp, post = run.tick(NO_CONTACTS)
        r = jd.step(Bp, run.W, NO_CONTACTS, art, "quick")           # five rows: no motor any more
        assert r.islands[0].m == 5 and ld.velocity_error(r.bodies, post[:, 7:10], post[:, 10:13]) <= 1e-10 * ld.velocity_scale(r.bodies, run.W)
        w.set_hinge_limots(None)                                     # n = 0 is always accepted
    finally:
        run.close()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
def test_limots_none_of_which_is_present_change_nothing(prec, stepper):
    """a set with limots -- zero poses, a vel without fmax -- but none present gives the same post-tick state, bit for bit, as the
    same set without limots, on the single-launch tick and on the general path"""
    B, art, lim, jts = lm.small_world()
    lim["lo_stop"], lim["hi_stop"], lim["fmax"], lim["vel"] = -np.inf, np.inf, 0.0, 2.0
    out = []
    for l in (None, lim):
        for mode in (B_.SMALL_TICK_OFF, B_.SMALL_TICK_AUTO):
            run = Run(prec, B, world(), art, l, stepper, small=mode)
            try:
                for _ in range(2):
                    _, post = run.tick(jts)
                out.append(post)
            finally:
                run.close()
    assert all(np.array_equal(out[0], o) for o in out[1:])
