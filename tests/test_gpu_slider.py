"""Slider and fixed joints through dmxBatchSetJoints / dmxBatchSetHingeLimots / dmxBatchStepJoints (both steppers, both precisions,
the general path and the single-launch tick), dmxBatchSliderPositions and dmxBatchJointErrors, against the dense float64 reference
with these joints (tests/slider_dense.py).

Run and the tolerances are test_gpu_hinge_limot.py's: every case uploads a synthetic state, a set of joints with limots and a list
of contact joints, takes a tick (or a few) and compares each with the reference restarted from the device's own pre-tick state.
Velocities: float64 QuickStep 1e-10 and float64 dWorldStep 1e-8 relative to max(|v_ref|, g h), float32 dWorldStep 10 eps32 kappa(A)
with kappa from the reference, asserted <= 1e-3, float32 QuickStep the per-body band of tests/quick_band.py with the joint rows' term
at K = quick_band.K["joint"], no clamp-margin gate (the old allowance stays as a second ceiling where the old rule admits the tick:
quick_band.assert_in_old_allowance); and that file's THETA_MARGIN rule, here also in metres: every compared tick
asserts that the reference's hinges and sliders are 1e-3 (rad, m) or more from their stops.  Every float32 QuickStep case is listed
in F32_QUICK_CASES (tests/test_quick_band.py runs the float32 emulation over them); CHAIN_CASES are the ones a dropped sweep cannot
pass.  (tests/test_gpu_feedback.py takes `reference_tick` with the rules this file had before the band.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

import joint_dense as jd
import lcp_dense as ld
import limot_dense as lm
import quick_band as qb
import slider_dense as sd
import test_gpu_hinge_limot as hl
from __graft_entry__ import load_package

pkg = load_package()
B_ = pkg.batch
pytestmark = pytest.mark.gpu

H = hl.H
EPS32 = hl.EPS32
PRECS = hl.PRECS
STEPPERS = hl.STEPPERS
EINVAL = hl.EINVAL
THETA_MARGIN = hl.THETA_MARGIN
NO_CONTACTS = hl.NO_CONTACTS
Run, world, as_precision, to_c = hl.Run, hl.world, hl.as_precision, hl.to_c
SMALL = [B_.SMALL_TICK_OFF, B_.SMALL_TICK_AUTO]
DEVICE_WORST = {"joint": 0.0}            # the largest device deviation of this process, in eps32 M_v (printed by compare)


def reference_tick(prec, stepper, W, Bp, jts, art, lim, band=False):
    """the reference's tick of a batch of this precision, and the tolerance it allows by test_gpu_hinge_limot.compare's rules.
    band: float32 QuickStep is held to the band of tests/quick_band.py instead (tolerance None, the joint term attached); without it
    the rule from before the band, 10 eps32 kappa(A) where the clamp-margin gate passes"""
    Wr, jr, ar, lr = as_precision(prec, W, jts, art, lim)
    r = sd.step(Bp, Wr, jr, ar, lr, stepper)
    tm = min(lm.theta_margin(r), sd.pos_margin(r))
    print(f"{prec} {stepper}: stop margin {tm:.3e}")
    assert tm >= THETA_MARGIN, f"a hinge or a slider is {tm:.2e} from a stop: too close for two precisions to agree on the row"
    f32 = np.dtype(prec).itemsize == 4
    if f32 and stepper == "quick" and band:
        return qb.attach_joint_term(r, Bp, Wr, jr, ar, lr), Wr, None
    if not f32:
        t = 1e-10 if stepper == "quick" else 1e-8
    else:
        t = 10 * EPS32 * max([I.kappa() for I in r.islands] + [1.0])
        assert t <= 1e-3, f"float32 tolerance {t:.2e}: too ill-conditioned a case to be a test"
        if stepper == "quick":
            for I, lam, margin in zip(r.islands, r.lams, r.margins):
                if I.m:
                    assert margin > 1e-3 * np.max(np.abs(lam)), "f32 QuickStep case too close to a clamp to compare"
    return r, Wr, t


def compare(run, Bp, post, jts):
    """one device tick against the reference from the same pre-tick state; -> the reference's Result"""
    prec, stepper = run.prec, run.stepper
    r, Wr, t = reference_tick(prec, stepper, run.W, Bp, jts, run.art, run.lim, band=True)
    f32 = np.dtype(prec).itemsize == 4
    live = np.nonzero(Bp.flags & ld.ALIVE)[0]
    if t is None:
        worst = qb.assert_in_band(r, Wr, post, qb.K["joint"], live)
        DEVICE_WORST["joint"] = max(DEVICE_WORST["joint"], worst)
        used = qb.assert_in_old_allowance(r, Wr, post, live)
        print(f"f32 QuickStep on the device: {worst:.2f} eps32 M_v (K = {qb.K['joint']}; largest so far {DEVICE_WORST['joint']:.2f}); "
              + ("the old rule does not admit the tick" if used is None else f"{used:.3f} of the old allowance"))
        return r
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
# (seeds for which the reference meets the conditions in both precisions and under both steppers: found on the CPU)
MODE_SEED = 3
TWO_SEED = 5
CHAIN_SEED = 11
STAR_SEEDS = {8: 0, 40: 0, 100: 3}
STAR_GROUND_SEED = 9
CARRY_SEED = 0
WORLD_SEED = 13


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("swapped", [False, True])
@pytest.mark.parametrize("small", SMALL)
def test_one_body_on_a_slider_to_the_world_every_line_of_the_table(prec, stepper, swapped, small):
    """one-body islands of 6 rows, one per line of the table and per motor-at-a-stop variant, given as (body, world) and as
    (world, body), on the general path and on the single-launch tick"""
    B, art, lim = sd.one_body_per_mode(swapped, MODE_SEED)
    (r,), _, st, _ = check(prec, B, world(), art, lim, stepper, small=small)
    assert [I.m for I in r.islands] == [6] * len(sd.MODES)
    assert [I.limot_lines[0] for I in r.islands] == [sd.MODE_LINES[m] for m in sd.MODES]
    names = list(sd.MODES)
    k = names.index("low_stop_leaving")
    assert r.lams[k][5] == r.islands[k].lo[5] == 0.5
    k = names.index("low_stop_motor_away")
    assert r.lams[k][5] > r.islands[k].lo[5] == 0.5
    assert (st["small"], st["general"]) == ((1, 0) if small == B_.SMALL_TICK_AUTO else (0, 1))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("swapped", [False, True])
@pytest.mark.parametrize("small", SMALL)
def test_one_body_fixed_to_the_world(prec, stepper, swapped, small):
    B, art, lim = sd.one_body(None, swapped, MODE_SEED, kind=sd.FIXED)
    res, _, st, _ = check(prec, B, world(), art, lim, stepper, ticks=2, small=small)
    assert res[0].islands[0].m == 6 and res[0].islands[0].nbd == 0
    assert st["small"] == (2 if small == B_.SMALL_TICK_AUTO else 0)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("kind,mode", [(sd.SLIDER, "motor_free"), (sd.SLIDER, "low_stop_motor_into"), (sd.SLIDER, None), (sd.FIXED, None)])
def test_two_bodies_one_of_them_kinematic(prec, stepper, kind, mode):
    B, art, lim = sd.two_bodies(kind, mode, kinematic=True, seed=TWO_SEED)
    res, _, _, _ = check(prec, B, world(), art, lim, stepper, ticks=2)
    assert res[0].islands[0].m == (6 if kind == sd.FIXED or mode else 5)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("small", SMALL)
def test_cart_pole(prec, stepper, small):
    """a cart on a motorised slider along x carrying a pole on a hinge: one island of 6 + 5 rows, three ticks"""
    B, art, lim = sd.cart_pole()
    res, _, st, _ = check(prec, B, world(), art, lim, stepper, ticks=3, small=small)
    assert all(r.islands[0].m == 11 and r.islands[0].limot_lines == [3] for r in res)
    assert st["small"] == (3 if small == B_.SMALL_TICK_AUTO else 0)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("small", SMALL)
def test_one_island_with_all_four_kinds(prec, stepper, small):
    """world - slider - hinge - ball - fixed - slider over five bodies: 6 + 6 + 3 + 6 + 6 rows"""
    B, art, lim = sd.all_kinds_chain(CHAIN_SEED)
    (r,), _, _, _ = check(prec, B, world(), art, lim, stepper, small=small)
    assert len(r.islands) == 1 and r.islands[0].m == 27 and r.islands[0].nbd == 3


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("n", [8, 40, 100])
def test_star_of_sliders_and_welds_with_mixed_limots(prec, stepper, n):
    """a heavy hub and n spokes on sliders and welds, the sliders' limots cycling through the table's lines: QuickStep's
    one-wavefront and workgroup forms, dWorldStep's LDS solve (n = 40) and the grid solve (n = 100)"""
    B, art, lim, jts = sd.star(n, seed=STAR_SEEDS[n])
    (r,), st, _, _ = check(prec, B, world(), art, lim, stepper, jts)
    I = r.islands[0]
    m, nl = sd.star_rows(art, lim)
    assert (I.m, I.nbd) == (m, nl) and len(I.limot_rows) == nl
    if stepper == "exact":
        # (40 spokes are 240 rows of which 27 can clamp: the LDS solve holds them in float32 and not in float64 -- a workgroup's LDS is
        #  what it is, test_gpu_hinge_limot.py's 40-star is in the same place -- so the float64 case runs the grid solve too)
        grid = n == 100 or (n == 40 and prec == "float64")
        if n == 100:
            assert st["solves"] == 1, "the grid solve did not run"
        if n == 40 and prec == "float32":
            assert st["solves"] == 0, "the LDS solve did not run"
        assert st["solves"] == (1 if grid else 0)
        if grid:
            assert (st["last_m"], st["last_nbd"], st["last_nu"]) == (m, nl, m - nl)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
def test_star_on_ground_contacts(prec, stepper):
    """the 8-star with four frictionless ground contacts under the hub: slider limot rows and contact rows clamp in one island"""
    B, art, lim, jts = sd.star(8, seed=STAR_GROUND_SEED, contacts=True)
    (r,), _, _, _ = check(prec, B, world(), art, lim, stepper, jts)
    assert r.islands[0].m == sd.star_rows(art, lim)[0] + 4


CARRY_TICKS, CARRY_FMAX = 4, 0.03125          # (a float32 number: the reference of a float32 batch sees the same bound)


def toggled_limots(lim0, s, t):
    """the slider star's limots for tick t, every stop placed relative to the slider's position at the tick's start (0.05 m or more
    away): on even ticks a weak motor asked for +-3 m/s, which saturates at +fmax (k even) or -fmax (k odd); on odd ticks the same
    spoke is at its low stop (k even: hi = +inf) or its high stop (k odd: lo = -inf) with that motor -- the bound its row ended
    the tick before on is not there any more"""
    lim = lim0.copy()
    for k in range(len(lim)):
        up = k % 2 == 0
        if t % 2 == 0:
            sd.set_mode(lim[k], (-np.inf, np.inf, 3.0 if up else -3.0, CARRY_FMAX))
        elif up:
            sd.set_mode(lim[k], (s[k] + 0.05, s[k] + 1.0, 3.0, CARRY_FMAX))
        else:
            sd.set_mode(lim[k], (s[k] - 1.0, s[k] - 0.05, -3.0, CARRY_FMAX))
    return lim


@pytest.mark.parametrize("prec", PRECS)
def test_grid_solve_carries_its_active_set_over_slider_limots_whose_bounds_change(prec):
    """100 motorised sliders round a hub under dWorldStep, one island of 600 rows on the grid solve, which starts every tick from the
    active set the rows ended the last one with; dmxBatchSetHingeLimots per tick turns rows saturated at -fmax / +fmax into
    high-stop / low-stop rows and back.  Every tick is compared with the reference"""
    n = 100
    B, art, lim0 = sd.slider_star(n, seed=CARRY_SEED)
    run = Run(prec, B, world(), art, lim0, "exact")
    try:
        for t in range(CARRY_TICKS):
            s = run.w.slider_positions()[0]
            run.set_limots(toggled_limots(lim0, s, t))
            Bp, post = run.tick(NO_CONTACTS)
            r = compare(run, Bp, post, NO_CONTACTS)
            I, lam = r.islands[0], r.lams[0]
            rows = I.limot_rows
            if t % 2 == 0:
                assert all(lam[rows[k]] == (CARRY_FMAX if k % 2 == 0 else -CARRY_FMAX) for k in range(n))
            else:
                assert all((I.lo[rows[k]], I.hi[rows[k]]) == ((CARRY_FMAX, np.inf) if k % 2 == 0 else (-np.inf, -CARRY_FMAX)) for k in range(n))
        st = run.w.lcp_stats()
    finally:
        run.close()
    assert st["solves"] == CARRY_TICKS and (st["last_m"], st["last_nbd"]) == (6 * n, n)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
def test_small_tick_and_general_path_agree_bit_for_bit(prec, stepper):
    B, art, lim, jts = sd.small_world(WORLD_SEED)
    assert B.n == 48
    out = {}
    for mode in SMALL:
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


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
def test_small_world_against_the_reference(prec, stepper):
    B, art, lim, jts = sd.small_world(WORLD_SEED)
    check(prec, B, world(), art, lim, stepper, jts)


# ---------------------------------------------------------------------------------------------------------------------
# Chains a wrong sweep cannot pass (slider_dense.mixed_chain: all four kinds, rotated bodies, errors to correct, limots on hinges and
# sliders over every line of the table), one island each on either side of every boundary between the float32 QuickStep row forms
# an island with joint rows takes -- units keep it off the contact-as-unit forms (csrc/dmx_islands_dev.hpp, solve_island_wg_body):
#   up to WAVE_ISLAND_ROWS = 256 rows   one wavefront, the rows in registers; the single-launch tick takes such a world too
#   257 .. 1 024                        the register form, 256 threads
#   1 025 .. REGS_ROWS<float> = 3 072   the register form, 512 threads
#   above                               the streamed form
# and 40 rows on the lane-per-island form (a child process).  One more has ground contacts that clamp among the joint rows.
CHAIN_FORMS = {256: "one wavefront", 260: "registers, 256 threads", 1024: "registers, 256 threads", 1028: "registers, 512 threads",
               3072: "registers, 512 threads", 3076: "streamed"}
CHAIN_CASES = ["mixed_chain-40"] + [f"mixed_chain-{rows}" for rows in CHAIN_FORMS] + ["mixed_chain_on_ground-1028"]
FORM_CASES = {"lane per island": ["mixed_chain-40"], "single-launch tick": ["mixed_chain-256"]}
for _rows, _form in CHAIN_FORMS.items():
    FORM_CASES.setdefault(_form, []).append(f"mixed_chain-{_rows}")
FORM_CASES["registers, 512 threads"].append("mixed_chain_on_ground-1028")


def _chain_checks(r, rows, contacts=False):
    (I,), (lam,) = r.islands, r.lams
    assert I.m == rows and set(I.limot_lines) == {0, 1, 2, 3, 4}
    at = [k for k in I.limot_rows if np.isfinite(I.lo[k]) or np.isfinite(I.hi[k])]
    assert any(lam[k] in (I.lo[k], I.hi[k]) for k in at) and any(lam[k] not in (I.lo[k], I.hi[k]) for k in at)
    if contacts:
        fr = np.isfinite(I.hi) & (I.row_kind > 0)
        assert np.any(lam[I.row_kind == 0] == 0) and np.any(lam[I.row_kind == 0] > 0), "normal rows: loaded and at 0"
        assert np.any(lam[fr] == I.hi[fr]) and np.any(lam[fr] == I.lo[fr]), "friction rows at both bounds"
        assert I.m - I.n_art_rows == np.sum(I.row_kind >= 0) > 20


@pytest.mark.parametrize("rows", sorted(CHAIN_FORMS))
def test_quickstep_chain_of_all_kinds_on_every_row_form_f32(rows):
    B, art, lim, jts = sd.mixed_chain(rows)
    (r,), _, st, _ = check("float32", B, world(), art, lim, "quick", jts, small=B_.SMALL_TICK_OFF)
    _chain_checks(r, rows)
    assert (st["small"], st["general"]) == (0, 1), st


def test_quickstep_chain_of_all_kinds_on_the_single_launch_tick_f32():
    B, art, lim, jts = sd.mixed_chain(256)
    (r,), _, st, _ = check("float32", B, world(), art, lim, "quick", jts, small=B_.SMALL_TICK_AUTO)
    _chain_checks(r, 256)
    assert (st["small"], st["general"]) == (1, 0), st


def test_quickstep_chain_with_ground_contacts_that_clamp_f32():
    """1 028 rows, 512-thread register form: joint rows, limot rows and contact rows with friction in one island; normal rows end
    loaded and at 0, friction rows at both bounds (asserted on the reference), and nothing gates them"""
    B, art, lim, jts = sd.mixed_chain(1028, contacts=True)
    (r,), _, st, _ = check("float32", B, world(), art, lim, "quick", jts, small=B_.SMALL_TICK_OFF)
    _chain_checks(r, 1028, contacts=True)
    assert (st["small"], st["general"]) == (0, 1), st


def child_lane_per_island_chain_f32():
    """(run by test_chain_on_the_lane_per_island_form_f32 under DMX_BIG_ISLAND_ROWS=64) 40 rows of all four kinds on 9 bodies with
    the single-launch tick off: swept by one lane (row_sor in solve_islands)"""
    threshold = int(os.environ["DMX_BIG_ISLAND_ROWS"])
    B, art, lim, jts = sd.mixed_chain(40)
    (r,), _, st, _ = check("float32", B, world(), art, lim, "quick", jts, small=B_.SMALL_TICK_OFF)
    (I,) = r.islands
    assert I.m == 40 < threshold and len(I.slots) > 1 and {sd.HINGE, sd.BALL, sd.SLIDER, sd.FIXED} <= set(art["kind"].tolist())
    assert (st["small"], st["general"]) == (0, 1), st


def test_chain_on_the_lane_per_island_form_f32():
    """DMX_BIG_ISLAND_ROWS is read once per process: a child"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_slider as t; t.child_lane_per_island_chain_f32(); "
            "print('CHILD-OK')") % (here, os.path.dirname(here))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600,
                       env={**os.environ, "DMX_BIG_ISLAND_ROWS": "64"})
    assert p.returncode == 0 and "CHILD-OK" in p.stdout, (p.stdout[-2000:] + p.stderr[-3000:])


# every float32 QuickStep case `compare` sees: name -> () -> (Bodies, World, contact joints, joints, limots, ticks).
# tests/test_quick_band.py runs the float32 emulation of a float32 batch's rows and sweeps over them (quick_band.MEASURED["joint"])
def _case(B, art, lim, jts=NO_CONTACTS, ticks=1):
    return B, world(), jts, art, lim, ticks


F32_QUICK_CASES = {
    "one_body_per_mode": lambda: _case(*sd.one_body_per_mode(False, MODE_SEED)),
    "one_body_per_mode-swapped": lambda: _case(*sd.one_body_per_mode(True, MODE_SEED)),
    "one_body_fixed": lambda: _case(*sd.one_body(None, False, MODE_SEED, kind=sd.FIXED), ticks=2),
    "one_body_fixed-swapped": lambda: _case(*sd.one_body(None, True, MODE_SEED, kind=sd.FIXED), ticks=2),
    "cart_pole": lambda: _case(*sd.cart_pole(), ticks=3),
    "all_kinds_chain": lambda: _case(*sd.all_kinds_chain(CHAIN_SEED)),
    "star_on_ground-8": lambda: _case(*sd.star(8, seed=STAR_GROUND_SEED, contacts=True)),
    "small_world": lambda: _case(*sd.small_world(WORLD_SEED)),
}
for _n in (8, 40, 100):
    F32_QUICK_CASES[f"star-{_n}"] = lambda n=_n: _case(*sd.star(n, seed=STAR_SEEDS[n]))
for _kind, _mode in [(sd.SLIDER, "motor_free"), (sd.SLIDER, "low_stop_motor_into"), (sd.SLIDER, None), (sd.FIXED, None)]:
    F32_QUICK_CASES[f"two_bodies-{_kind}-{_mode}"] = lambda k=_kind, m=_mode: _case(*sd.two_bodies(k, m, kinematic=True, seed=TWO_SEED), ticks=2)
for _rows in [40] + sorted(CHAIN_FORMS):
    F32_QUICK_CASES[f"mixed_chain-{_rows}"] = lambda rows=_rows: _case(*sd.mixed_chain(rows))
F32_QUICK_CASES["mixed_chain_on_ground-1028"] = lambda: _case(*sd.mixed_chain(1028, contacts=True))


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("with_limots", [True, False])
def test_slider_positions_and_joint_errors_against_numpy(prec, with_limots):
    """1 000 random joints of all four kinds over 64 bodies, moved after the joints were made.  s and the errors are sums of a few
    products of numbers of a few units: 64 eps of the precision times the largest coordinate (the rate: times the largest
    velocity too); |2 e_v| is a product of three unit quaternions: 32 eps"""
    B, art, lim = sd.random_joints()
    rng = np.random.default_rng(5)
    B.pos += rng.normal(scale=0.3, size=B.pos.shape)
    B.quat += 0.2 * rng.normal(size=B.quat.shape)
    B.quat /= np.linalg.norm(B.quat, axis=1)[:, None]
    run = Run(prec, B, world(), art, lim if with_limots else None, "quick")
    try:
        s, sdot = run.w.slider_positions()
        pe, ae, mx = run.w.joint_errors()
        th, _ = run.w.hinge_angles()
        state = run.state()
    finally:
        run.close()
    _, _, ar, lr = as_precision(prec, run.W, NO_CONTACTS, art, lim)
    Bs = run.bodies(state)
    rs, rd = sd.positions(Bs, ar)
    rpe, rae = sd.errors(Bs, ar, lr if with_limots else None)
    eps = EPS32 if prec == "float32" else 2.2e-16
    size = max(1.0, np.max(np.abs(state[:, 0:3])) + np.max(np.abs(ar["anchor1"])) + np.max(np.abs(ar["anchor2"])))
    vmax = max(1.0, np.max(np.abs(state[:, 7:13])))
    print(f"{prec}: s error {np.max(np.abs(s - rs)) / eps:.1f} eps, rate {np.max(np.abs(sdot - rd)) / eps:.1f} eps, "
          f"pos_err {np.max(np.abs(pe - rpe)) / eps:.1f} eps, axis_err {np.max(np.abs(ae - rae)) / eps:.1f} eps")
    assert np.max(np.abs(s - rs)) <= 64 * eps * size
    assert np.max(np.abs(sdot - rd)) <= 64 * eps * size * vmax
    assert np.max(np.abs(pe - rpe)) <= 64 * eps * size
    assert np.max(np.abs(ae - rae)) <= 32 * eps
    assert abs(mx[0] - pe.max()) == 0 and abs(mx[1] - ae.max()) == 0
    slider = art["kind"] == sd.SLIDER
    active = np.array([k for (_, k), *_ in jd.canonical_arts(Bs, art)])
    off = np.ones(len(art), bool)
    off[active] = False
    assert np.all(s[~slider] == 0) and np.all(sdot[~slider] == 0) and np.all(s[off] == 0) and np.all(sdot[off] == 0) and off.sum() > 20
    assert np.all(th[art["kind"] != jd.HINGE] == 0)
    assert np.sum(np.abs(rs) > 0.05) > 300 and np.sum(rae > 0.05) > 300


def reference_weld_run(stepper, ticks):
    B, art, lim = sd.weld_chain(5)
    W = world()
    mp = ma = 0.0
    for _ in range(ticks):
        B = sd.step(B, W, NO_CONTACTS, art, lim, stepper).bodies
        pe, ae = sd.errors(B, art, lim)
        mp, ma = max(mp, pe.max()), max(ma, ae.max())
    return mp, ma


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
def test_a_chain_of_welds_hangs_from_the_world(prec, stepper):
    """five unit bodies welded in a row, the first to the world, sticking out level under gravity for 120 ticks: the joints'
    errors stay within twice the reference's own over a reference-only run"""
    ticks = 120
    ref_p, ref_a = reference_weld_run(stepper, ticks)
    assert ref_p > 0 and ref_a > 0
    B, art, lim = sd.weld_chain(5)
    run = Run(prec, B, world(), art, lim, stepper)
    try:
        mp = ma = 0.0
        for _ in range(ticks):
            run.w.step_joints(run.W.h, NO_CONTACTS.astype(B_.CONTACT_JOINT_DTYPE))
            _, _, mx = run.w.joint_errors()
            mp, ma = max(mp, mx[0]), max(ma, mx[1])
    finally:
        run.close()
    print(f"{prec} {stepper}: pos_err {mp:.4e} (reference {ref_p:.4e}), axis_err {ma:.4e} (reference {ref_a:.4e})")
    assert mp <= 2 * ref_p and ma <= 2 * ref_a


# ---------------------------------------------------------------------------------------------------------------------
def test_api_refuses_what_it_must():
    B, art, lim = sd.two_bodies(sd.SLIDER, "motor_free", kinematic=False)
    run = Run("float64", B, world(), art, lim, "quick")
    w = run.w
    try:
        bad = to_c(art, B_.JOINT_DTYPE)
        bad["kind"] = 7
        with pytest.raises(B_.DmxError) as e:
            w.set_joints(bad)
        assert e.value.code == EINVAL
        assert w.joint_count() == 1                                  # (the set is what it was)
        for kind, anchor, axis in ((B_.JOINT_SLIDER, (0.0, 1.0, 0.0), (0.0, 0.0, 0.0)), (B_.JOINT_SLIDER, (0.0, 1.0, 0.0), None), (7, (0.0, 1.0, 0.0), (1.0, 0.0, 0.0))):
            with pytest.raises(B_.DmxError) as e:
                w.joint_from_world(kind, 0, -1, anchor, axis)
            assert e.value.code == EINVAL
        got = w.joint_from_world(B_.JOINT_FIXED, 0, 1, (0.5, 2.1, 0.0), None)          # a fixed joint needs no axis
        ref = jd.from_world(B, sd.FIXED, 0, 1, (0.5, 2.1, 0.0))
        assert np.max(np.abs(got["anchor1"] - ref["anchor1"])) <= 1e-14 and np.max(np.abs(got["anchor2"] - ref["anchor2"])) <= 1e-14
        got = w.joint_from_world(B_.JOINT_SLIDER, 0, -1, (0.5, 2.1, 0.0), (0.0, 3.0, 0.0))
        ref = jd.from_world(B, sd.SLIDER, 0, -1, (0.5, 2.1, 0.0), (0.0, 1.0, 0.0))
        assert np.max(np.abs(got["axis1"] - ref["axis1"])) <= 1e-14 and np.array_equal(got["axis2"], (0.0, 1.0, 0.0))
        # the ticks that collide on the device refuse while a slider is set
        with pytest.raises(B_.DmxError) as e:
            w.step(H, 1)
        assert e.value.code == EINVAL
    finally:
        run.close()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
def test_slider_limots_none_of_which_is_present_change_nothing(prec, stepper):
    """a set with limots -- the identity for every zero pose, a vel without fmax -- none of which is present gives the same
    post-tick state, bit for bit, as the same set without limots, on the single-launch tick and on the general path"""
    B, art, lim, jts = sd.small_world(WORLD_SEED)
    lim = sd.default_limots(len(art))
    lim["vel"] = 2.0
    out = []
    for l in (None, lim):
        for mode in SMALL:
            run = Run(prec, B, world(), art, l, stepper, small=mode)
            try:
                for _ in range(2):
                    _, post = run.tick(jts)
                out.append(post)
            finally:
                run.close()
    assert all(np.array_equal(out[0], o) for o in out[1:])
