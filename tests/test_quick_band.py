"""The band of tests/quick_band.py measured, and shown to decide something.  CPU only.

  1. The measurement behind quick_band.MEASURED / quick_band.K, re-run and asserted: (a) the float32 oracle's one-tick deviation
     from the float64 reference on the 90 QuickStep scenes of tests/test_solver_dense.py, (b) the float32 emulation of the
     reference's own sweeps on the inputs of every float32 QuickStep case of the GPU files that take the band (their
     F32_QUICK_CASES).  Both stay at or below K / 2; K is the K_BAND rule applied to the table; the table is what is measured.
  2. The clamp-margin gate the band replaces refused 84 of the 90 oracle scenes; on those no float32 oracle deviation exceeds
     K -- the clamp is non-expansive, so a decision flipped next to a bound moves lambda by no more than the rounding did.
  3. The band can tell: the reference with one parameter changed -- one sweep fewer, another sor_w, friction bounds 1 % off, a
     surface flag ignored -- leaves the unchanged reference's band by 10 x or more on at least one body."""
import functools

import numpy as np
import pytest

import lcp_dense as ld
import quick_band as qb
import joint_dense as jd
import limot_dense as lm
import slider_dense as sd
import test_gpu_body_flags as gbf
import test_gpu_hinge_limot as ghl
import test_gpu_joints as gj
import test_gpu_slider as gsl
import test_gpu_small_tick as gst
import test_gpu_solver_dense as gsd
import test_solver_dense as tsd

GYROS = [ld.GYRO_OFF, ld.GYRO_EXPLICIT, ld.GYRO_IMPLICIT]
ORACLE_CASES = [(s, mu, b, g) for s in tsd.SCENES for mu in (0.0, 0.3, np.inf) for b in (False, True) for g in GYROS]
GATE_REFUSED = 84                           # of the 90 (re-measured by test_the_gate_refused_what_the_band_holds)


def test_k_is_the_rule_applied_to_the_table():
    for family, m in qb.MEASURED.items():
        worst = max(m.values())
        assert qb.K[family] == 2 ** int(np.ceil(np.log2(2 * worst))) and worst <= qb.K[family] / 2, family
        assert qb.K[family] <= qb.K_MAX, f"{family}: a K above {qb.K_MAX} means the model misses a factor"


# --------------------------------------------------------------------------------------------------------------------- 1 (a), 2
@functools.lru_cache(maxsize=None)
def _oracle_population(orc32):
    """-> per case (deviation in eps32 M_v, whether the old gate passes)"""
    out = []
    for case in ORACLE_CASES:
        r, W, post, _, _ = tsd.oracle_tick_f32(orc32, *case)
        out.append((float(np.max(qb.deviation(r, post[:, 7:10], post[:, 10:13]))), qb.gate_passes(r)))
    return out


def _matches(measured, table):
    """the committed figure is the measured one (to the two digits it is written with, and 2 % for another BLAS's summation order
    in the float32 dot products; what holds the device is the K / 2 assertion beside each use)"""
    return abs(measured - table) <= 0.02 * table + 0.01


def test_float32_oracle_population(orc32):
    worst = max(d for d, _ in _oracle_population(orc32))
    print(f"contact rows, population (a), float32 oracle on {len(ORACLE_CASES)} scenes: largest deviation {worst:.2f} eps32 M_v "
          f"(table {qb.MEASURED['contact']['oracle']}, K = {qb.K['contact']})")
    assert worst <= qb.K["contact"] / 2
    assert _matches(worst, qb.MEASURED["contact"]["oracle"])


def test_the_gate_refused_what_the_band_holds(orc32):
    pop = _oracle_population(orc32)
    refused = [d for d, ok in pop if not ok]
    print(f"the clamp-margin gate refuses {len(refused)} of {len(pop)} oracle scenes; largest deviation among them "
          f"{max(refused):.2f} eps32 M_v")
    assert (len(refused), len(pop)) == (GATE_REFUSED, 90)
    assert max(refused) <= qb.K["contact"]


# --------------------------------------------------------------------------------------------------------------------- 1 (b)
def _reference_f32(B, jts, W):
    B2, W2, j2 = qb.as_f32_inputs(B, W, jts)
    return ld.step(B2, W2, j2, "quick"), W2


@functools.lru_cache(maxsize=None)
def _emulated(module, name):
    """-> (largest emulation deviation, whether the old gate passes, facts about a one-island case: rows, kappa(A) below 1 025
    rows, whether normal rows end at 0 and friction rows at hi and at lo); the reference itself is not kept (3 073 rows: 75 MB)"""
    r, W = _reference_f32(*module.F32_QUICK_CASES[name]())
    facts = None
    if len(r.islands) == 1:
        (I,), (lam,) = r.islands, r.lams
        fr = np.isfinite(I.hi)
        facts = (I.m, I.kappa() if I.m <= 1025 else None, bool(np.any(lam[I.row_kind == 0] == 0)),
                 bool(np.any(lam[fr] == I.hi[fr])), bool(np.any(lam[fr] == I.lo[fr])), bool(np.all(np.diag(I.A) > 0) and np.all(np.isfinite(I.A))))
    return float(np.max(qb.emulation_deviation(r, W))), qb.gate_passes(r), facts


def _flags_change_ticks():
    """the six ticks of test_gpu_body_flags.test_flags_change_between_ticks, each from the reference's last state rounded to
    float32 (the device's differs from it by less than the band), with the flags then in force"""
    B, jts, W = gbf.F32_QUICK_CASES["flags_change"]()
    worst, gate = 0.0, True
    for t, f40 in enumerate(gbf.FLAGS_OF_BODY_40):
        B.flags[40] = f40
        r, W2 = _reference_f32(B, jts, W)
        worst = max(worst, float(np.max(qb.emulation_deviation(r, W2))))
        gate = gate and qb.gate_passes(r)
        B = r.bodies
    return worst, gate


EMULATED = [(mod, name) for mod in (gsd, gst, gbf) for name in mod.F32_QUICK_CASES]


def test_float32_emulation_population():
    devs = {(mod.__name__, name): _emulated(mod, name)[:2] for mod, name in EMULATED}
    devs[("test_gpu_body_flags", "flags_change, six ticks")] = _flags_change_ticks()
    worst_key = max(devs, key=lambda k: devs[k][0])
    worst = devs[worst_key][0]
    refused = sorted(f"{m.replace('test_gpu_', '')}:{n}" for (m, n), (_, ok) in devs.items() if not ok)
    print(f"contact rows, population (b), float32 sweeps on {len(devs)} GPU cases: largest deviation {worst:.2f} eps32 M_v on "
          f"{worst_key[1]} (table {qb.MEASURED['contact']['emulation']}, K = {qb.K['contact']})")
    print(f"cases the clamp-margin gate would refuse ({len(refused)}): {', '.join(refused)}")
    assert worst <= qb.K["contact"] / 2
    assert _matches(worst, qb.MEASURED["contact"]["emulation"])


@pytest.mark.parametrize("m", sorted(gsd.CLAMP_SEEDS))
def test_clamp_chains_clamp_and_stay_conditioned(m):
    """the seeds of the GPU file's clamping islands: a finite kappa(A), rows at 0 and at both friction bounds, the gate refuses
    them, and the emulation stays at or below K / 2"""
    dev, gate, (rows, kappa, at_zero, at_hi, at_lo, finite) = _emulated(gsd, f"clamp_chain-{m}")
    assert rows == m and not gate
    assert finite and (kappa is None or kappa < 1.0 / (10 * qb.EPS32))          # (3 073 rows: eigvalsh would be this file's minute)
    assert at_zero and at_hi and at_lo
    jts = gsd.clamp_chain(m)[1]
    assert np.any(jts["mode"] == ld.CONTACT_BOUNCE) and np.any(jts["mode"] == 0)
    assert dev <= qb.K["contact"] / 2


# --------------------------------------------------------------------------------------------------------------------- 3
def _one_island(case, rows):
    """the case's inputs cut down to the island with `rows` rows"""
    B, jts, W = case
    B2, W2, j2 = qb.as_f32_inputs(B, W, jts)
    for slots, cj in ld.islands(B2, ld.canonical(B2, j2)):
        I = ld.Island(B2, W2, slots, cj, j2)
        if I.m == rows:
            keep = np.isin(j2["body1"], slots)
            sub = ld.Bodies(B.pos[slots], B.quat[slots], B.lvel[slots], B.avel[slots], B.mass[slots], B.inertia[slots], B.flags[slots])
            j = jts[keep].copy()
            to = {s: k for k, s in enumerate(slots)}
            j["body1"] = [to[b] for b in j["body1"]]
            j["body2"] = [to.get(b, -1) for b in j["body2"]]
            return sub, j, W
    raise AssertionError(f"no island of {rows} rows")


def _changed(case, change):
    """-> the largest |v_changed - v_ref| over the unchanged reference's band, over bodies"""
    B, jts, W = case
    r, W2 = _reference_f32(B, jts, W)
    jc = jts.copy()
    Wc = ld.World(h=W.h, gravity=W.gravity, erp=W.erp, cfm=W.cfm, iters=W.iters, sor_w=W.sor_w, gyro=W.gyro)
    if change == "19 sweeps":
        Wc.iters = W.iters - 1
    elif change == "sor_w 1.25":
        Wc.sor_w = 1.25
    elif change == "mu x 1.01":
        jc["mu"] = np.where(np.isfinite(jts["mu"]), 1.01 * jts["mu"], jts["mu"])
    elif change == "soft CFM ignored":
        jc["mode"] = jts["mode"] & ~ld.CONTACT_SOFT_CFM
    elif change == "soft ERP ignored":
        jc["mode"] = jts["mode"] & ~ld.CONTACT_SOFT_ERP
    elif change == "bounce ignored":
        jc["mode"] = jts["mode"] & ~ld.CONTACT_BOUNCE
    else:
        raise KeyError(change)
    rc, _ = _reference_f32(B, jc, Wc)
    band = qb.velocity_band(r, W2, qb.K["contact"])
    dv = np.maximum(np.max(np.abs(rc.bodies.lvel - r.bodies.lvel), axis=1), np.max(np.abs(rc.bodies.avel - r.bodies.avel), axis=1))
    return float(np.max(dv / band))


CAN_TELL = {
    "19 sweeps, press_chain 256": (lambda: gsd.F32_QUICK_CASES["press_chain-256"](), "19 sweeps"),
    "19 sweeps, bounce_mixed": (lambda: gsd.F32_QUICK_CASES["surface-bounce_mixed"](), "19 sweeps"),
    "19 sweeps, chain 80 x 320 mu = inf": (lambda: _one_island(gsd.F32_QUICK_CASES["mixed_islands"](), 960), "19 sweeps"),
    "19 sweeps, mass ratios implicit gyro": (lambda: gsd.F32_QUICK_CASES[f"mass_ratios-gyro{ld.GYRO_IMPLICIT}"](), "19 sweeps"),
    "sor_w 1.25, bounce_mixed": (lambda: gsd.F32_QUICK_CASES["surface-bounce_mixed"](), "sor_w 1.25"),
    "mu x 1.01, bounce_mixed": (lambda: gsd.F32_QUICK_CASES["surface-bounce_mixed"](), "mu x 1.01"),
    "mu x 1.01, chain 5 x 20": (lambda: _one_island(gsd.F32_QUICK_CASES["mixed_islands"](), 60), "mu x 1.01"),
    "soft CFM ignored, soft_cfm_1e-3": (lambda: gsd.F32_QUICK_CASES["surface-soft_cfm_1e-3"](), "soft CFM ignored"),
    "soft ERP ignored, soft_erp_08": (lambda: gsd.F32_QUICK_CASES["surface-soft_erp_08"](), "soft ERP ignored"),
    "bounce ignored, bounce_mixed": (lambda: gsd.F32_QUICK_CASES["surface-bounce_mixed"](), "bounce ignored"),
}


@pytest.mark.parametrize("name", sorted(CAN_TELL))
def test_the_band_can_tell(name):
    case, change = CAN_TELL[name]
    out = _changed(case(), change)
    print(f"{name}: the changed reference leaves the band by {out:.3g} x")
    assert out >= 10.0


# --------------------------------------------------------------------------------------------------------------------- 4
# Islands with joint rows: why the three joint files (test_gpu_joints.py, test_gpu_hinge_limot.py, test_gpu_slider.py) are NOT on
# the band.  Every float32 QuickStep case their `compare` sees, as (step function, Bodies, World, contact joints, joints, limots,
# ticks[, before(t, limots)]); a later tick starts from the reference's last state.
def _w():
    return ld.World(cfm=1e-5)


def _motor_door():
    B, art, lim, W = ghl.motor_door()

    def before(t, lim):
        lim["vel"][0] = ghl.motor_vel(t)
    return B, W, ghl.NO_CONTACTS, art, lim, ghl.MOTOR_TICKS, before


def _j(B, art, jts=gj.NO_CONTACTS, ticks=1):
    return B, _w(), jts, art, None, ticks


def _l(B, art, lim, jts=ghl.NO_CONTACTS, ticks=1):
    return B, _w(), jts, art, lim, ticks


JOINT_CASES = {
    "joints:one_body-ball": lambda: _j(*gj.one_body(jd.BALL)), "joints:one_body-hinge": lambda: _j(*gj.one_body(jd.HINGE)),
    "joints:two_bodies-plain": lambda: _j(*gj.two_bodies(), ticks=2),
    "joints:two_bodies-body1_is_world": lambda: _j(*gj.two_bodies(first_is_world_side=True), ticks=2),
    "joints:two_bodies-kinematic": lambda: _j(*gj.two_bodies(kinematic=True), ticks=2),
    "joints:chain_on_ground": lambda: _j(*gj.chain_on_ground()),
    "joints:star-64": lambda: _j(*jd.star(64)), "joints:star-90": lambda: _j(*jd.star(90)),
    "joints:star_on_ground-100": lambda: _j(*gj.star_on_ground(100)),
    "joints:pendulum_pairs": lambda: _j(*gj.pendulum_pairs()),
    "hinge_limot:one_body_per_mode": lambda: _l(*ghl.one_body_per_mode(False)),
    "hinge_limot:one_body_per_mode-swapped": lambda: _l(*ghl.one_body_per_mode(True)),
    "hinge_limot:star_on_ground-8": lambda: _l(*lm.hinge_star(8, seed=ghl.STAR_GROUND_SEEDS[8], contacts=True)),
    "hinge_limot:doors": lambda: _l(*lm.doors(600, nfree=40, seed=ghl.DOORS_SEED)),
    "hinge_limot:motor_door": _motor_door,
    "slider:one_body_per_mode": lambda: _l(*sd.one_body_per_mode(False, gsl.MODE_SEED)),
    "slider:one_body_per_mode-swapped": lambda: _l(*sd.one_body_per_mode(True, gsl.MODE_SEED)),
    "slider:one_body_fixed": lambda: _l(*sd.one_body(None, False, gsl.MODE_SEED, kind=sd.FIXED), ticks=2),
    "slider:one_body_fixed-swapped": lambda: _l(*sd.one_body(None, True, gsl.MODE_SEED, kind=sd.FIXED), ticks=2),
    "slider:cart_pole": lambda: _l(*sd.cart_pole(), ticks=3),
    "slider:all_kinds_chain": lambda: _l(*sd.all_kinds_chain(gsl.CHAIN_SEED)),
    "slider:star_on_ground-8": lambda: _l(*sd.star(8, seed=gsl.STAR_GROUND_SEED, contacts=True)),
    "slider:small_world": lambda: _l(*sd.small_world(gsl.WORLD_SEED)),
}
for _mode in ("motor_free", "low_stop_motor_into", "high_stop"):
    JOINT_CASES[f"hinge_limot:two_bodies-{_mode}"] = lambda mode=_mode: _l(*lm.two_bodies(mode, kinematic=True), ticks=2)
for _n in (8, 40, 100):
    JOINT_CASES[f"hinge_limot:hinge_star-{_n}"] = lambda n=_n: _l(*lm.hinge_star(n, seed=ghl.STAR_SEEDS[n]))
    JOINT_CASES[f"slider:star-{_n}"] = lambda n=_n: _l(*sd.star(n, seed=gsl.STAR_SEEDS[n]))
for _kind, _mode in [(sd.SLIDER, "motor_free"), (sd.SLIDER, "low_stop_motor_into"), (sd.SLIDER, None), (sd.FIXED, None)]:
    JOINT_CASES[f"slider:two_bodies-{_kind}-{_mode}"] = lambda k=_kind, m=_mode: _l(*sd.two_bodies(k, m, kinematic=True, seed=gsl.TWO_SEED), ticks=2)


def _side_f32(bodies, s, anchor, axis):
    """joint_dense.side with the body's rotation, R anchor and R axis evaluated in float32 (the quaternion, the anchor and the axis
    are float32 numbers already): what a float32 batch can know of a_i = R_i anchor_i"""
    f = np.float32
    if s < 0:
        return np.array(anchor, np.float64), np.zeros(3), np.array(axis, np.float64)
    w, x, y, z = (bodies.quat[s].astype(f) / np.sqrt(np.sum(bodies.quat[s].astype(f) ** 2, dtype=f))).astype(f)
    one, two = f(1), f(2)
    R = np.array([[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
                  [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
                  [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]], f)
    return bodies.pos[s], (R @ np.asarray(anchor, f)).astype(np.float64), (R @ np.asarray(axis, f)).astype(np.float64)


def _joint_step(B, W, jts, art, lim, f32_sides):
    """the reference's QuickStep tick of a float32 batch holding these inputs -> (Result, the world as the batch holds it)"""
    B2, _, _ = qb.as_f32_inputs(B, W, jts)
    Wr, jr, ar, lr = ghl.as_precision("float32", W, jts, art, lim)
    side = jd.side
    jd.side = _side_f32 if f32_sides else side
    try:
        return sd.step(B2, Wr, jr, ar, lr, "quick"), Wr
    finally:
        jd.side = side


@functools.lru_cache(maxsize=None)
def _joint_population():
    """-> per case (sweeps alone in float32, sweeps and the rows' R anchor / R axis in float32), largest deviation from the float64
    reference over bodies and ticks in eps32 M_v"""
    out = {}
    for name, case in JOINT_CASES.items():
        B, W, jts, art, lim, ticks, *before = case()
        sweeps = rows = 0.0
        for t in range(ticks):
            if before:
                before[0](t, lim)
            r, Wr = _joint_step(B, W, jts, art, lim, False)
            sweeps = max(sweeps, float(np.max(qb.emulation_deviation(r, Wr))))
            r32, _ = _joint_step(B, W, jts, art, lim, True)
            lv, av = B.lvel.copy(), B.avel.copy()
            for I in r32.islands:
                v = I.velocities(qb.emulate_f32(I, Wr.iters, Wr.sor_w).astype(np.float64)).reshape(-1, 6) if I.m else I.velocities(np.zeros(0)).reshape(-1, 6)
                lv[I.slots], av[I.slots] = v[:, :3], v[:, 3:]
            kin = (B.flags & ld.KINEMATIC) != 0
            lv[kin], av[kin] = r.bodies.lvel[kin], r.bodies.avel[kin]
            rows = max(rows, float(np.max(qb.deviation(r, lv, av))))
            B = r.bodies
        out[name] = (sweeps, rows)
    return out


def test_joint_rows_need_a_term_the_model_lacks():
    """Two float32 emulations of every float32 QuickStep case of the three joint files, both from the float64 reference of the same
    float32 inputs.  The sweeps alone (A, b, lo, hi cast to float32) stay where contact rows do: quick_band.JOINT_MEASURED["sweeps"].
    With the rows' a_i = R_i anchor_i and R_i axis_i evaluated in float32 as well -- nothing else changed -- the deviation reaches
    JOINT_MEASURED["rows"]: above K_MAX / 2 = 32, so by the K rule the family would need K = 128.  A joint row's right-hand side is
    ERP / h times a position error, and (ERP / h) eps32 |a| of it is rounding of R anchor whatever lambda is: a term M_v lacks.
    That is why those files keep 10 eps32 kappa(A) (the issue's rule for a family whose emulation cannot be kept under 32).  The
    device, run once with the band applied at K = 8, left it by up to 35.4 on the same case this emulation puts at the top; the
    bodies of the stars are not rotated, their R is exact, and both emulations agree on them."""
    pop = _joint_population()
    sweeps = max(pop, key=lambda k: pop[k][0])
    rows = max(pop, key=lambda k: pop[k][1])
    print(f"joint rows, float32 sweeps on {len(pop)} cases: largest deviation {pop[sweeps][0]:.2f} eps32 M_v on {sweeps} "
          f"(table {qb.JOINT_MEASURED['sweeps']})")
    print(f"joint rows, float32 sweeps and float32 R anchor / R axis: largest deviation {pop[rows][1]:.2f} eps32 M_v on {rows} "
          f"(table {qb.JOINT_MEASURED['rows']}); above 8: " + ", ".join(f"{k} {v[1]:.1f}" for k, v in pop.items() if v[1] > 8))
    assert _matches(pop[sweeps][0], qb.JOINT_MEASURED["sweeps"]) and pop[sweeps][0] <= qb.K["contact"] / 2
    assert _matches(pop[rows][1], qb.JOINT_MEASURED["rows"])
    assert pop[rows][1] > qb.K_MAX / 2 and qb.k_rule(pop[rows][1]) > qb.K_MAX, "the joint family fits the model after all: move it onto the band"
    assert rows == "hinge_limot:doors"
    for name in ("joints:star-64", "joints:star-90", "hinge_limot:hinge_star-100", "slider:star-100"):
        assert pop[name][0] == pop[name][1], name              # identity rotations: R anchor is exact in float32
