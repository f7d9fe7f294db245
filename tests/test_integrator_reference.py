"""The CPU oracle's rigid-body integrator (oracle/orc_step.c: step_island's free part, gyro_torque, step_body) against the float64
definition of tests/integrator_reference.py -- no GPU.  The device copies are bit-identical to the oracle (tests/test_gpu_integrator.py
asserts it on the same populations), so what is pinned here pins them.

a. closed forms that need no recollection of ODE: the world-frame spin, stepping back, forces acting once, unit quaternions
b. / c. one tick of both oracles within c eps64 M / k eps32 M of the reference, over every population, place and gyro mode
d. 64 ticks of the float32 oracle against the reference, on the bodies the reference calls comparable
e. the populations contain what they claim"""
import numpy as np
import pytest

from tests import integrator_reference as ir
from oracle.orc_ctypes import Oracle

H = ir.H
DTYPES = ("float64", "float32")


# ---------------------------------------------------------------------------------------------------------------- a. closed forms
def _spinners(n=96, seed=5):
    """isotropic bodies at random orientations, spinning about random world axes: |w| h from 0.01 to 0.5 and, every fourth, to 20"""
    rng = np.random.default_rng(seed)
    q = ir._f32(ir._unit(rng, n, 4))
    wh = np.where(np.arange(n) % 4 == 3, ir._logu(rng, 0.5, 20.0, n), ir._logu(rng, 0.01, 0.5, n))
    w = ir._f32(ir._unit(rng, n) * (wh / H)[:, None])
    return q, w


def _oracle_spin(dtype, q, w, hs, inertia=1.0):
    """the oracle in zero gravity, one tick per entry of `hs` (ticks may differ in sign); a callable entry is applied to the world
    (orc, ow) between ticks -> the quaternions after every tick"""
    orc = Oracle(dtype)
    ow = orc.world(gravity=(0.0, 0.0, 0.0))
    n = len(q)
    k = np.arange(n)
    pos = np.stack([(k % 64) * ir.PITCH, np.zeros(n), (k // 64) * ir.PITCH], axis=1)
    ow.add_boxes(pos, q, np.zeros((n, 3)), w, np.ones(n), np.full((n, 3), inertia), np.full((n, 3), 0.5))
    out = []
    for h in hs:
        if callable(h):
            h(orc, ow)
            continue
        ow.tick(orc.dtype.type(h))
        out.append(ow.state()[1].astype(float))
    ow.close()
    return out


def _rot_err(Ra, Rb):
    return np.max(np.abs(Ra - Rb), axis=(1, 2))


@pytest.mark.parametrize("dtype", DTYPES)
def test_spin_is_about_the_world_axis(dtype):
    """Isotropic inertia, no gravity: w is constant, and q' = normalise((1, h w / 2) (x) q) is the rotation by 2 atan(|w| h / 2) about
    w / |w| applied AFTER R(q), in the world frame: R(q') = Rot(w / |w|, 2 atan(|w| h / 2)) R(q); after 25 ticks, 25 times the
    angle.  With the product the other way round the body would turn about R(q) w instead."""
    q, w = _spinners()
    wn = np.linalg.norm(w, axis=1)
    axis = w / wn[:, None]
    theta = 2.0 * np.arctan(0.5 * wn * H)
    R0 = ir.rotation_of(ir.normalise(q))
    # the axes do not commute with q: the body-frame answer R(q) Rot differs visibly from the world-frame one for every body
    wrong = R0 @ ir.rot(axis, theta)
    right = ir.rot(axis, theta) @ R0
    assert np.min(_rot_err(wrong, right)) > 1e-3, "a spin axis commutes with its body's orientation"
    after = _oracle_spin(dtype, q, w, [H] * 25)
    eps = ir.EPS32 if dtype == "float32" else ir.EPS64
    for ticks in (1, 25):
        got = ir.rotation_of(after[ticks - 1])
        err = _rot_err(got, ir.rot(axis, ticks * theta) @ R0)
        # per tick: the band of the quaternion (k eps (1 + h |w| / 2)), twice over in R; the rounding of w itself is none (it never changes)
        tol = ticks * 2.0 * ir.K_BAND[("quat", "implicit")] * eps * (1.0 + 0.5 * H * wn) * 2.0
        i = int(np.argmax(err / tol))
        assert err[i] <= tol[i], f"{dtype}, {ticks} tick(s): R(q') is off the world-frame spin by {err[i]:.3g} (tolerance {tol[i]:.3g}) for q={q[i]!r} w={w[i]!r}"
        assert np.min(_rot_err(got, R0 @ ir.rot(axis, ticks * theta))) > 1e-4, "the body-frame spin would have passed too"
    # the reference itself obeys the same closed form
    st = (np.zeros_like(w), ir.normalise(q), np.zeros_like(w), w)
    for _ in range(25):
        st = ir.tick(st, np.ones(len(q)), np.ones((len(q), 3)), H, (0, 0, 0), ir.GYRO_IMPLICIT)
    assert np.max(_rot_err(ir.rotation_of(st[1]), ir.rot(axis, 25 * theta) @ R0)) < 1e-12


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_negated_tick_returns_the_start_orientation(dtype):
    """normalise((1, -h w / 2)) is the conjugate of normalise((1, h w / 2)): a tick with h negated (w as it is), or with w negated (h
    as it is), undoes the tick before it; with h AND w negated h w is the same, and so is the tick."""
    q, w = _spinners()
    wn = np.linalg.norm(w, axis=1)
    eps = ir.EPS32 if dtype == "float32" else ir.EPS64
    tol = 4.0 * ir.K_BAND[("quat", "implicit")] * eps * (1.0 + 0.5 * H * wn)
    q0 = ir.normalise(q)
    R0 = ir.rotation_of(q0)

    def negate_w(orc, ow):
        for b in range(len(w)):
            orc.lib.orc_body_set_angular_vel(ow.w, b, *[float(-x) for x in w[b]])

    fwd, back = _oracle_spin(dtype, q, w, [H, -H])
    assert np.all(_rot_err(ir.rotation_of(back), R0) <= tol), "h negated does not undo the tick"
    assert np.min(_rot_err(ir.rotation_of(fwd), R0)) > 1e-4
    fwd2, back2 = _oracle_spin(dtype, q, w, [H, negate_w, H])
    assert np.all(_rot_err(ir.rotation_of(back2), R0) <= tol), "w negated does not undo the tick"
    both, = _oracle_spin(dtype, q, -w, [-H])
    assert np.all(_rot_err(ir.rotation_of(both), ir.rotation_of(fwd)) <= tol), "h and w both negated is not the same tick"


@pytest.mark.parametrize("dtype", DTYPES)
def test_force_and_torque_act_in_the_first_tick_only(dtype):
    """zero gravity, gyro off, anisotropic bodies: after the first tick v = v0 + h f / m and w = w0 + h I_w^-1 t; the second and the
    third tick leave both velocities as they are, bit for bit (v + (h / m) 0 = v)."""
    pop = ir.stress("near0g")
    orc = Oracle(dtype)
    ow = orc.world(gravity=pop.gravity)
    orc.lib.orc_world_set_gyro_mode(ow.w, ir.GYRO_OFF)
    ow.add_boxes(pop.pos, pop.quat, pop.lvel, pop.avel, pop.mass, pop.inertia, pop.sides)
    forced = np.flatnonzero(pop.forced)
    assert len(forced) > 1000 and (~pop.forced).sum() > 2000
    for b in forced:
        orc.lib.orc_body_add_force(ow.w, int(b), *[float(x) for x in pop.force[b]])
        orc.lib.orc_body_add_torque(ow.w, int(b), *[float(x) for x in pop.torque[b]])
    h = orc.dtype.type(H)
    ow.tick(h)
    s1 = [a.copy() for a in ow.state()]
    ref = ir.tick(pop.start(), pop.mass, pop.inertia, H, pop.gravity, ir.GYRO_OFF, pop.force, pop.torque)
    ir.check_one_tick(s1, ref, pop, ir.GYRO_OFF, dtype, "forced tick")
    dv = np.linalg.norm(s1[2].astype(float) - pop.lvel, axis=1)
    want = H * np.linalg.norm(pop.force, axis=1) / pop.mass
    assert np.all(dv[forced] > 0.5 * want[forced]) and np.all(want[forced] > 0), "a force never acted"
    assert np.all(dv[~pop.forced] == 0)
    dw = np.linalg.norm(s1[3].astype(float) - pop.avel, axis=1)              # gyro off: without a torque w stays as it is
    least = H * np.linalg.norm(pop.torque, axis=1) / pop.inertia.max(axis=1)      # |h I_w^-1 t| >= h |t| / I_max
    seen = pop.forced & (least > 1e-4 * np.linalg.norm(pop.avel, axis=1))         # ... and large enough to show in float32
    assert seen.sum() > 500 and np.all(dw[seen] > 0.5 * least[seen]), "a torque never acted"
    assert np.all(dw[~pop.forced] == 0)
    for t in (2, 3):
        ow.tick(h)
        st = ow.state()
        assert np.array_equal(st[2], s1[2]), f"tick {t}: a force acted again"
        assert np.array_equal(st[3], s1[3]), f"tick {t}: a torque acted again"
    ow.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_zero_quaternion_comes_out_as_the_identity(dtype):
    q = np.zeros((3, 4)); q[1] = (0.0, 0.6, 0.0, 0.8); q[2] = (-0.0, 0.0, -0.0, 0.0)
    w = np.zeros((3, 3))
    after, = _oracle_spin(dtype, q, w, [H])
    assert np.array_equal(after[0], [1.0, 0.0, 0.0, 0.0]) and np.array_equal(after[2], [1.0, 0.0, 0.0, 0.0])
    assert np.allclose(after[1], q[1], atol=1e-6)
    assert np.array_equal(ir.normalise(q)[0], [1.0, 0.0, 0.0, 0.0])


# ------------------------------------------------------------------------------------------------ b. / c. one tick, both precisions
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ir.MODES, ids=lambda m: ir.MODE_NAME[m])
@pytest.mark.parametrize("variant", ir.VARIANTS)
def test_one_tick_against_the_definition(variant, mode, dtype):
    """every class of the stress population, extreme spins included: finite wherever the reference is, within the band, |q| = 1"""
    ref = ir.reference_run("stress", variant, mode, 1)
    pop = ref["pop"]
    got = ir.oracle_run(pop, dtype, mode, 1)
    fin = ir.finite_rows(ref["state"])
    assert fin.mean() > 0.99
    worst = ir.check_one_tick(got, ref["state"], pop, mode, dtype, "oracle")
    unit = ir.check_unit_quaternions(got[1], fin, pop, f"oracle {dtype} {ir.MODE_NAME[mode]}")
    print(f"{variant} {ir.MODE_NAME[mode]} {dtype}: " + " ".join(f"{f}={v:.3g}" for f, v in worst.items()) + f" | |q|-1: {unit:.3g} eps")


# ---------------------------------------------------------------------------------------------------------------------- d. 64 ticks
@pytest.mark.parametrize("mode", ir.MODES, ids=lambda m: ir.MODE_NAME[m])
@pytest.mark.parametrize("variant", ir.VARIANTS)
def test_64_ticks_in_float32_against_the_definition(variant, mode):
    ref = ir.reference_run("flight", variant, mode, ir.N_TICKS)
    pop = ref["pop"]
    assert ref["excused"] <= ir.MAX_EXCUSED, f"the reference excuses {ref['excused']:.1%} of {pop.name}"
    got = ir.oracle_run(pop, "float32", mode, ir.N_TICKS)
    worst = ir.check_n_ticks(got, ref["state"], ref["comparable"], pop, variant, mode, "float32 oracle")
    ir.check_unit_quaternions(got[1], ref["comparable"], pop, "float32 oracle, 64 ticks")
    print(f"{variant} {ir.MODE_NAME[mode]}: excused {ref['excused']:.2%} " + str({c: {f: round(v, 2) for f, v in d.items()} for c, d in worst.items()}))


# ---------------------------------------------------------------------------------------------------------------------- e. coverage
@pytest.mark.parametrize("kind", ["stress", "flight"])
@pytest.mark.parametrize("variant", ir.VARIANTS)
def test_populations_contain_what_they_claim(kind, variant):
    pop = (ir.stress if kind == "stress" else ir.flight)(variant)
    assert pop.n == ir.N_GPU
    for a in (pop.pos, pop.quat, pop.lvel, pop.avel, pop.mass, pop.inertia, pop.force, pop.torque):
        assert np.array_equal(a, a.astype(np.float32).astype(np.float64)), "a value is not a float32"
    # the lattice: no two bodies nearer than 8 m, at the start and -- |v| <= 2.6 + h |f| / m, 64 ticks -- ever
    k = np.arange(pop.n)
    shift = np.asarray(ir.FAR) if pop.far else np.zeros(3)
    assert np.allclose(pop.pos - shift, np.stack([(k % 64) * 8.0, 0 * k, (k // 64) * 8.0], axis=1))
    reach = ir.N_TICKS * H * (np.linalg.norm(pop.lvel, axis=1) + H * np.linalg.norm(pop.force, axis=1) / pop.mass)
    assert reach.max() < 0.5 * (8.0 - 0.5 * np.sqrt(3.0)), "two bodies could meet"
    kap = pop.kappa
    classes = ir.KAPPA_CLASSES if kind == "stress" else ("iso", "k3")
    for c, cname in enumerate(ir.KAPPA_CLASSES):
        m = pop.kclass == c
        if cname not in classes:
            assert not m.any()
            continue
        assert m.sum() >= pop.n // len(classes) - 1
        if cname == "iso":
            assert np.all(kap[m] == 1.0) and np.all(pop.inertia[m, 0] == pop.inertia[m, 2])
        else:
            lo, hi = ir._KAPPA_RANGE[cname]
            assert np.all((kap[m] > 1.0) & (kap[m] > lo * (1 - 1e-6)) & (kap[m] <= hi * (1 + 1e-6)))
            assert kap[m].max() > 0.8 * hi, f"{cname}: no body near the class's upper end"
            # any of the three axes may be the slender one
            assert set(np.argmax(pop.inertia[m], axis=1).tolist()) == {0, 1, 2}
        # every class has forced and unforced bodies, and (stress) extreme spins
        assert (m & pop.forced).sum() > 50 and (m & ~pop.forced).sum() > 50
        if kind == "stress":
            assert (m & pop.extreme).sum() > 50
    wh = np.linalg.norm(pop.avel, axis=1) * H
    tame = ~pop.extreme
    hi = 0.5 if kind == "stress" else 0.05
    assert wh[tame].min() < 2e-4 and wh[tame].max() > 0.8 * hi and wh[tame].max() <= hi * (1 + 1e-6)
    if kind == "stress":
        assert wh[pop.extreme].max() > 50 and wh[pop.extreme].max() <= 100 * (1 + 1e-6) and wh[pop.extreme].min() >= 0.5 * (1 - 1e-6)
    else:
        assert not pop.extreme.any()
    assert pop.mass.min() < 2e-3 and pop.mass.max() > 500
    assert abs(pop.forced.mean() - 1 / 3) < 0.01 and np.array_equal(pop.force.any(axis=1), pop.torque.any(axis=1))
    # both signs of every component
    for name, a in (("quat", pop.quat), ("lvel", pop.lvel), ("avel", pop.avel), ("force", pop.force), ("torque", pop.torque)):
        assert np.all((a > 0).sum(axis=0) > 100) and np.all((a < 0).sum(axis=0) > 100), name
    # orientations are away from the identity and the spin axes do not commute with them
    q = ir.normalise(pop.quat)
    assert np.median(np.abs(q[:, 0])) < 0.8
    u = q[:, 1:] / np.linalg.norm(q[:, 1:], axis=1, keepdims=True)
    s = np.abs(np.sum(u * pop.avel / np.linalg.norm(pop.avel, axis=1, keepdims=True), axis=1))
    assert np.mean(s < 0.9) > 0.8
    assert pop.gravity == ((0.0, 0.0, 0.0) if variant == "near0g" else ir.G)
    # the excused share, from the reference alone
    for mode in ir.MODES:
        ticks = 1 if kind == "stress" else ir.N_TICKS
        ref = ir.reference_run(kind, variant, mode, ticks)
        assert ref["excused"] <= ir.MAX_EXCUSED, f"{pop.name} {ir.MODE_NAME[mode]}: {ref['excused']:.1%} excused"


def test_the_bands_follow_their_rule():
    """k and c are 2 x the measured maxima rounded up to a power of two, and none is above 64 (a larger one would mean that the
    condition model lacks a factor); the N-tick tolerance is 4 x the measured maxima"""
    for band, measured in ((ir.K_BAND, ir.ONE_TICK_MEASURED_F32), (ir.C_BAND, ir.ONE_TICK_MEASURED_F64)):
        for mode in ir.MODES:
            for i, f in enumerate(ir.FIELDS):
                worst = max(measured[(ir.MODE_NAME[mode], p)][i] for p in ("near", "far"))
                k = band[(f, ir.MODE_NAME[mode])]
                assert k == ir._pow2_at_least(2.0 * worst) and k <= 64
    for band, measured in ((ir.K_GYRO, ir.GYRO_MEASURED_F32), (ir.C_GYRO, ir.GYRO_MEASURED_F64)):
        for mode in ("explicit", "implicit"):
            assert band[mode] == ir._pow2_at_least(2.0 * max(measured[mode])) and band[mode] <= 64
    assert ir.TICK_FACTOR == 4.0
    assert set(ir.TICK_MEASURED) == {(c, p, ir.MODE_NAME[m]) for c in ("iso", "k3") for p in ("near", "far") for m in ir.MODES}
