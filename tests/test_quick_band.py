"""The band of tests/quick_band.py measured, and shown to decide something.  CPU only.

  1. The measurement behind quick_band.MEASURED / quick_band.K, re-run and asserted: (a) the float32 oracle's one-tick deviation
     from the float64 reference on the 90 QuickStep scenes of tests/test_solver_dense.py, (b) the float32 emulation of the
     reference's own sweeps on the inputs of every float32 QuickStep case of the GPU files that take the band (their
     F32_QUICK_CASES).  Both stay at or below K / 2; K is the K_BAND rule applied to the table; the table is what is measured.
  2. The clamp-margin gate the band replaces refused 84 of the 90 oracle scenes; on those no float32 oracle deviation exceeds
     K -- the clamp is non-expansive, so a decision flipped next to a bound moves lambda by no more than the rounding did.
  3. The band can tell: the reference with one parameter changed -- one sweep fewer, another sor_w, friction bounds 1 % off, a
     surface flag ignored -- leaves the unchanged reference's band by 10 x or more on at least one body.
  4. Islands with joint rows: the record that M_v without the joint rows' term needs K above 64; the family's population with the
     term and everything a float32 batch computes for a joint row emulated in float32 (K["joint"]); the band against the allowance
     it replaces, case by case; and the chains of the joint files, on each of which 19 sweeps, sor_w 1.25, ERP x 1.01 and the
     world's CFM ignored leave the band by 10 x or more -- one per file and per device form at least for the dropped sweep."""
import functools

import numpy as np
import pytest

import lcp_dense as ld
import quick_band as qb
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
# Islands with joint rows (test_gpu_joints.py, test_gpu_hinge_limot.py, test_gpu_slider.py; test_gpu_small_tick.py holds no
# articulation joint -- the joint files run the single-launch tick themselves).  Every float32 QuickStep case their `compare` sees is
# in their F32_QUICK_CASES as () -> (Bodies, World, contact joints, joints, limots, ticks[, before(t, limots)]); a later tick starts
# from the reference's last state.
JOINT_FILES = {"joints": gj, "hinge_limot": ghl, "slider": gsl}
JOINT_CASES = {f"{f}:{name}": case for f, mod in JOINT_FILES.items() for name, case in mod.F32_QUICK_CASES.items()}
# the scenes a dropped sweep cannot pass (section 3 of each file); the others are the 36 the old model's figures were measured on
CHAIN_CASES = [f"{f}:{name}" for f, mod in JOINT_FILES.items() for name in mod.CHAIN_CASES]


@functools.lru_cache(maxsize=None)
def _joint_case(name):
    """-> per tick of the case, largest over bodies: (float32 sweeps alone, old model; float32 sweeps and R anchor / R axis, old
    model; everything a float32 batch computes for a row in float32, the model with the joint term; the new band at K["joint"] over
    the old allowance 10 eps32 kappa x scale, both as the largest velocity error allowed over live bodies)"""
    B, W, jts, art, lim, ticks, *before = JOINT_CASES[name]()
    out = []
    for t in range(ticks):
        if before:
            before[0](t, lim)
        r, inp = qb.joint_reference(B, W, jts, art, lim)
        dev = []
        for rows, term in ((False, False), ("sides", False), (True, True)):
            if name in CHAIN_CASES and not term:             # (the old model's record is about the 36 older cases)
                dev.append(np.nan)
                continue
            lv, av = qb.joint_emulation(r, inp, rows)
            dev.append(float(np.max(qb.deviation(r, lv, av, term))))
        live = np.nonzero(inp[0].flags & ld.ALIVE)[0]
        old = qb.old_allowance(r, inp[1], live)             # (None: the old rule does not admit the tick)
        ratio = np.nan if old is None else float(np.max(qb.velocity_band(r, inp[1], qb.K["joint"])[live])) / old
        out.append((*dev, ratio))
        B = r.bodies
    return out


def _joint_population():
    """-> per case the largest of each figure over its ticks (nan where a tick has none)"""
    return {name: tuple(float(np.max([tick[k] for tick in _joint_case(name)])) for k in range(4)) for name in JOINT_CASES}


def test_joint_rows_need_a_term_the_model_lacks():
    """The record of why the joint term exists, on the 36 cases the model was first tried on, with the model WITHOUT the term.  The
    float32 sweeps alone (A, b, lo, hi cast to float32) stay where contact rows do: quick_band.JOINT_MEASURED["sweeps"].  With the
    rows' a_i = R_i anchor_i and R_i axis_i evaluated in float32 as well -- nothing else changed -- the deviation reaches
    JOINT_MEASURED["rows"]: above K_MAX / 2 = 32, so by the K rule the family would need K = 128.  The bodies of the stars are
    not rotated, their R is exact, and both emulations agree on them."""
    pop = {k: v for k, v in _joint_population().items() if k not in CHAIN_CASES}
    assert len(pop) == 36
    sweeps = max(pop, key=lambda k: pop[k][0])
    rows = max(pop, key=lambda k: pop[k][1])
    print(f"joint rows, old model, float32 sweeps on {len(pop)} cases: largest deviation {pop[sweeps][0]:.2f} eps32 M_v on {sweeps} "
          f"(table {qb.JOINT_MEASURED['sweeps']})")
    print(f"joint rows, old model, float32 sweeps and float32 R anchor / R axis: largest deviation {pop[rows][1]:.2f} eps32 M_v on {rows} "
          f"(table {qb.JOINT_MEASURED['rows']}); above 8: " + ", ".join(f"{k} {v[1]:.1f}" for k, v in pop.items() if v[1] > 8))
    assert _matches(pop[sweeps][0], qb.JOINT_MEASURED["sweeps"]) and pop[sweeps][0] <= qb.K["contact"] / 2
    assert _matches(pop[rows][1], qb.JOINT_MEASURED["rows"])
    assert pop[rows][1] > qb.K_MAX / 2 and qb.k_rule(pop[rows][1]) > qb.K_MAX
    assert rows == "hinge_limot:doors"
    for name in ("joints:star-64", "joints:star-90", "hinge_limot:hinge_star-100", "slider:star-100"):
        assert pop[name][0] == pop[name][1], name              # identity rotations: R anchor is exact in float32


def test_joint_family_population():
    """population (b) of the joint family, with the joint term in the model: everything a float32 batch computes for a joint row done
    in float32 (quick_band.float32_rows, round_rows), then the float32 sweeps, over every float32 QuickStep case the joint files
    hold to the band, every tick, the chains of their section 3 included.  (The oracle has no joints: no population (a).)"""
    pop = _joint_population()
    worst = max(pop, key=lambda k: pop[k][2])
    print(f"joint rows, population (b), float32 rows and sweeps on {len(pop)} cases: largest deviation {pop[worst][2]:.2f} eps32 M_v on "
          f"{worst} (table {qb.MEASURED['joint']['emulation']}, K = {qb.K['joint']}); above 2: " +
          ", ".join(f"{k} {v[2]:.2f}" for k, v in pop.items() if v[2] > 2))
    assert pop[worst][2] <= qb.K["joint"] / 2
    assert _matches(pop[worst][2], qb.MEASURED["joint"]["emulation"])


BAND_WIDER = 29          # of the 36 (re-measured below)


def test_no_joint_case_is_held_to_less_than_before():
    """Per float32 QuickStep case the joint files had before the band: the band at K["joint"] over the old allowance
    10 eps32 kappa(A) x max(|v_ref|, g h), both as the largest velocity error allowed over live bodies.  The band is the wider one
    on most of them -- kappa ~ 1 .. 10 allowed 10 .. 100 eps32 of the velocity scale, less than the (ERP / h) eps32 |a| the rows'
    inputs can carry -- so the GPU files assert the old allowance too wherever the old rule admits the tick
    (quick_band.assert_in_old_allowance).  It admits every tick of every one of these cases: none is held to less than before"""
    pop = {k: v[3] for k, v in _joint_population().items() if k not in CHAIN_CASES}
    for k in sorted(pop, key=pop.get):
        print(f"{k}: band / old allowance {pop[k]:.3g}")
    assert all(np.isfinite(v) for v in pop.values()), [k for k, v in pop.items() if not np.isfinite(v)]
    assert sum(v > 1.0 for v in pop.values()) == BAND_WIDER
    chains = {k: v[3] for k, v in _joint_population().items() if k in CHAIN_CASES}
    print("chains the old rule admits: " + (", ".join(f"{k} (band / old allowance {v:.3g})" for k, v in chains.items() if np.isfinite(v)) or "none"))


# ---- the band can tell, on islands with joint rows
JOINT_CHANGES = ["19 sweeps", "sor_w 1.25", "ERP x 1.01", "CFM ignored"]


@functools.lru_cache(maxsize=None)
def _joint_changed(name):
    """-> per change, the largest |v_changed - v_ref| over the unchanged reference's band at K["joint"], over bodies (first tick)"""
    B, W, jts, art, lim, ticks, *before = JOINT_CASES[name]()
    if before:
        before[0](0, lim)
    r, (B2, W2, j2, a2, l2) = qb.joint_reference(B, W, jts, art, lim)
    band = qb.velocity_band(r, W2, qb.K["joint"])
    out = {}
    for change in JOINT_CHANGES:
        Wc = ld.World(h=W2.h, gravity=W2.gravity, erp=W2.erp, cfm=W2.cfm, iters=W2.iters, sor_w=W2.sor_w, gyro=W2.gyro)
        if change == "19 sweeps":
            Wc.iters = W2.iters - 1
        elif change == "sor_w 1.25":
            Wc.sor_w = 1.25
        elif change == "ERP x 1.01":
            Wc.erp = 1.01 * W2.erp
        else:
            Wc.cfm = 0.0
        rc = sd.step(B2, Wc, j2, a2, l2, "quick")
        dv = np.maximum(np.max(np.abs(rc.bodies.lvel - r.bodies.lvel), axis=1), np.max(np.abs(rc.bodies.avel - r.bodies.avel), axis=1))
        nz = band > 0
        out[change] = float(np.max(dv[nz] / band[nz]))
    return out


@pytest.mark.parametrize("name", CHAIN_CASES)
def test_the_band_can_tell_on_joint_chains(name):
    """every chain of the joint files' section 3: the reference with 19 sweeps, sor_w 1.25, ERP x 1.01 and the world's CFM ignored
    each leaves the unchanged reference's band by 10 x or more"""
    out = _joint_changed(name)
    print(f"{name}: " + ", ".join(f"{c} {v:.3g} x" for c, v in out.items()))
    for change, v in out.items():
        assert v >= 10.0, change


def test_every_family_and_every_form_has_a_case_that_tells_a_dropped_sweep():
    """the joint files name, per device form (FORM_CASES: the lane-per-island form, the single-launch tick, the one-wavefront form, the
    256- and 512-thread register forms, the streamed form), the chains that run on it; one per form and one per file must tell"""
    tells = lambda name: _joint_changed(name)["19 sweeps"] >= 10.0
    forms = {}
    for f, mod in JOINT_FILES.items():
        assert any(tells(f"{f}:{name}") for name in mod.CHAIN_CASES), f
        for form, names in mod.FORM_CASES.items():
            forms.setdefault(form, []).extend(f"{f}:{name}" for name in names)
    assert sorted(forms) == sorted(["lane per island", "single-launch tick", "one wavefront", "registers, 256 threads",
                                    "registers, 512 threads", "streamed"])
    for form, names in forms.items():
        assert any(tells(name) for name in names), form


def test_most_old_joint_cases_cannot_tell_a_dropped_sweep():
    """why the chains were needed: of the 36 cases the joint files had, the reference with 19 sweeps leaves the band at K["joint"] on
    a handful only -- the others have converged long before the 19th sweep"""
    told = sorted(k for k in JOINT_CASES if k not in CHAIN_CASES and _joint_changed(k)["19 sweeps"] >= 1.0)
    print(f"19 sweeps leaves the band on {len(told)} of 36: {', '.join(told)}")
    assert len(told) <= 8


