"""Every device copy of the rigid-body integrator on the populations of tests/integrator_reference.py: 4 133 isolated bodies (more
than eight workgroups of 256, a partial workgroup, a partial wavefront) of every inertia class, spin regime and forcing.

  1. / 2.  the float64 / float32 device is the float64 / float32 oracle bit for bit
  3.       every path gives the same bits as integrate_free with elision 0 (same precision, gyro mode, tick count, forcing)
  4.       on the bodies the float64 reference calls comparable, the float32 device is within the tolerance that
           tests/test_integrator_reference.py recorded ON THE CPU of the float64 device; no tolerance is taken from the device
  5. / 6.  nothing is NaN / Inf where the reference is finite; |q| = 1 within 4 eps on every path

The paths: free_body_step = tick_head + tick_tail (integrate_free; every elision mask, 1 and 7 ticks per launch, the out-of-place
first launch of a chunk and the in-place ones behind it, with and without external force / torque; per-body constants and -- batches
with ONE mass and one anisotropic inertia -- constants passed as kernel arguments), the same two functions called by step_plane_body
(a ground plane 1 km below) and by step_contacts (a static box 1 km away), each behind its own loads and before its own stores, and
the island path's stage_body + finish_body, the one other definition (step_joints without joints), which also serves the
single-launch tick of small worlds.  One tick runs on the `stress` population, 64 ticks on `flight` (the ranges in which the reference itself is
stable)."""
import functools

import numpy as np
import pytest

from __graft_entry__ import load_package
from tests import integrator_reference as ir

pkg = load_package()
B_ = pkg.batch
pytestmark = pytest.mark.gpu

H = ir.H
DTYPES = ("float32", "float64")
RUNS = (("stress", 1), ("flight", ir.N_TICKS))
PLANE = (0.0, 1.0, 0.0, -1000.0)
FAR_BOX = [((1.0, 1.0, 1.0), (-1000.0, 0.0, -1000.0), [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0])]
SMALL_N = 300


def _pop(kind, forced, variant="near", calm=False, uniform=None):
    """calm: horizontal velocities 1 / 32 (nobody leaves a safe zone); uniform: one mass and one inertia of that class for all"""
    pop = (ir.stress if kind == "stress" else ir.flight)(variant)
    if uniform:
        pop = pop.uniform(uniform, slow=kind != "stress")
    if calm:
        pop = pop.calm()
    return pop if forced else pop.without_forces()


def _device_run(pop, dtype, mode, ticks, setup=None, step=None, plane=None, statics=None, after=None):
    """the population on the device -> the state after `ticks` ticks; `step(w, ticks)` defaults to one dmxBatchStep call"""
    w = pkg.BatchWorld(pop.n, dtype=dtype, gravity=pop.gravity)
    try:
        w.set_gyro_mode(mode)
        if setup:
            setup(w)
        w.load_scene(pop.scene(dtype, plane, statics))
        if pop.forced.any():
            w.upload(B_.FORCE, pop.force); w.upload(B_.TORQUE, pop.torque)
        if step:
            step(w, ticks)
        else:
            w.step(H, ticks)
        w.synchronize()
        st = w.state()
        if after:
            after(w)
        if pop.forced.any():
            assert not w.download(B_.FORCE).any() and not w.download(B_.TORQUE).any(), "the accumulators were not cleared"
        return st
    finally:
        w.close()


def _free(elision, per_launch, proof):
    """integrate_free: `proof` on -- the collision proof's chunks, whose first launch is out of place (external forces then send the
    first tick through the exact path); off -- every launch in place, and external forces go through integrate_free's EXT form"""
    def setup(w):
        w.set_elision(elision); w.set_ticks_per_launch(per_launch); w.set_body_collisions(proof)
    return setup


@functools.lru_cache(maxsize=None)
def _baseline(kind, ticks, dtype, mode, forced, variant="near", calm=False, uniform=None):
    """integrate_free with elision 0, one tick per launch, every launch in place -- and the oracle on the same values"""
    pop = _pop(kind, forced, variant, calm, uniform)
    dev = _device_run(pop, dtype, mode, ticks, setup=_free(0, 1, False))
    orc = ir.oracle_run(pop, dtype, mode, ticks)
    for a in dev + orc:
        a.setflags(write=False)
    return dev, orc


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(got, want, pop, mode, path, against):
    """bit for bit; a failure names the path, the body with its values, and how far off it is in band units"""
    for name, a, b in zip(ir.FIELDS, got, want):
        assert a.dtype == b.dtype and a.shape == b.shape
        diff = (_bits(a) != _bits(b)).any(axis=1)
        if diff.any():
            i = int(np.flatnonzero(diff)[0])
            eps = ir.EPS32 if a.dtype == np.float32 else ir.EPS64
            dev = ir.in_band_units(got, want, pop, mode, eps)[name][i]
            raise AssertionError(f"{path} [{ir.MODE_NAME[mode]}, {a.dtype}]: {name} differs from {against} in its bits for {int(diff.sum())} "
                                 f"bodies; the first by {dev:.4g} eps x model: got {a[i]!r}, want {b[i]!r}\n" + pop.describe(i))


def _sound(got, kind, ticks, mode, forced, variant, pop, path):
    """5. and 6.: finite where the reference is, unit quaternions"""
    ref = ir.reference_run(kind, variant, mode, ticks, forced=forced)
    ok = ir.finite_rows(ref["state"]) if ticks == 1 else ref["comparable"]
    bad = ok & ~ir.finite_rows(got)
    assert not bad.any(), f"{path} [{ir.MODE_NAME[mode]}]: not finite where the reference is\n" + pop.describe(np.flatnonzero(bad)[0])
    ir.check_unit_quaternions(got[1], ok, pop, f"{path} [{ir.MODE_NAME[mode]}, {got[1].dtype}]")


def _every_case():
    for kind, ticks in RUNS:
        for dtype in DTYPES:
            for mode in ir.MODES:
                yield kind, ticks, dtype, mode


def _path_against_baseline(path, forced, n=None, calm=False, uniform=None, oracle_too=False, after_case=None, **run):
    """3.: the path's bits against integrate_free's, for every precision, gyro mode and tick count; after_case(w, ticks) sees the
    batch of every run before it is closed"""
    for kind, ticks, dtype, mode in _every_case():
        pop = _pop(kind, forced, "near", calm, uniform)
        base, orc = _baseline(kind, ticks, dtype, mode, forced, "near", calm, uniform)
        if n is not None:
            pop = pop.first(n)
            base = tuple(a[:n] for a in base)
        after = (lambda w, t=ticks: after_case(w, t)) if after_case else run.get("after")
        got = _device_run(pop, dtype, mode, ticks, after=after, **{k: v for k, v in run.items() if k != "after"})
        _same_bits(got, base, pop, mode, f"{path}, {ticks} tick(s)", "integrate_free (elision 0)")
        if oracle_too:
            _same_bits(got, orc, pop, mode, f"{path}, {ticks} tick(s)", "the oracle")
        ir.check_unit_quaternions(got[1], ir.finite_rows(got), pop, path)


# ------------------------------------------------------------------------------------------- 1. 2. 5. 6.: the baseline is the oracle
@pytest.mark.parametrize("forced", [True, False], ids=["forced", "unforced"])
@pytest.mark.parametrize("mode", ir.MODES, ids=lambda m: ir.MODE_NAME[m])
@pytest.mark.parametrize("dtype", DTYPES)
def test_integrate_free_is_the_oracle_bit_for_bit(dtype, mode, forced):
    for kind, ticks in RUNS:
        for variant in ir.VARIANTS:                                  # near, far, and near the origin without gravity
            pop = _pop(kind, forced, variant)
            dev, orc = _baseline(kind, ticks, dtype, mode, forced, variant)
            _same_bits(dev, orc, pop, mode, f"integrate_free (elision 0), {variant}, {ticks} tick(s)", "the oracle")
            _sound(dev, kind, ticks, mode, forced, variant, pop, "integrate_free")


# ------------------------------------------------------------------------------------------- 4.: float32 against float64, on the device
@pytest.mark.parametrize("variant", ["near", "far"])
@pytest.mark.parametrize("mode", ir.MODES, ids=lambda m: ir.MODE_NAME[m])
def test_float32_device_against_float64_device_within_the_cpu_tolerance(mode, variant):
    """one tick: k eps32 x condition model; 64 ticks: 4 x the CPU-measured maxima -- the numbers of tests/integrator_reference.py, which
    were fixed through the oracles against the float64 reference.  The float64 device stands in for the reference (it is within
    c eps64 of it, asserted here too).  Prints the maxima: they are the float32 oracle's of the CPU tests, the device being the oracle."""
    pop = _pop("stress", True, variant)
    ref = ir.reference_run("stress", variant, mode, 1)
    d32, _ = _baseline("stress", 1, "float32", mode, True, variant)
    d64, _ = _baseline("stress", 1, "float64", mode, True, variant)
    ir.check_one_tick(d64, ref["state"], pop, mode, "float64", "float64 device against the reference")
    fin = ir.finite_rows(ref["state"])
    d64f = tuple(np.where(fin[:, None], a, np.nan) for a in d64)            # finite rows of the reference only
    worst = ir.check_one_tick(d32, d64f, pop, mode, "float32", "float32 device against float64 device")
    print(f"1 tick {variant} {ir.MODE_NAME[mode]}: " + " ".join(f"{f}={v:.3g}" for f, v in worst.items()))
    pop = _pop("flight", True, variant)
    ref = ir.reference_run("flight", variant, mode, ir.N_TICKS)
    assert ref["excused"] <= ir.MAX_EXCUSED
    d32, _ = _baseline("flight", ir.N_TICKS, "float32", mode, True, variant)
    d64, _ = _baseline("flight", ir.N_TICKS, "float64", mode, True, variant)
    worst = ir.check_n_ticks(d32, d64, ref["comparable"], pop, variant, mode, "float32 device against float64 device")
    print(f"{ir.N_TICKS} ticks {variant} {ir.MODE_NAME[mode]}: " + str({c: {f: round(v, 2) for f, v in d.items()} for c, d in worst.items()}))


# ------------------------------------------------------------------------------------------- 3.: every path against the baseline
@pytest.mark.parametrize("per_launch", [1, 7])
@pytest.mark.parametrize("elision", [0, 1, 2, 3])
def test_integrate_free_in_place_with_and_without_external_forces(elision, per_launch):
    """no collision proof: every launch in place; forced bodies take the EXT instantiation in the first tick.  Mass and inertia
    differ from body to body here, so the constants are loaded whatever bit 1 of the mask says (the uniform batches are below)."""
    for forced in (True, False):
        _path_against_baseline(f"integrate_free elision {elision}, {per_launch} per launch, in place, forced {forced}", forced,
                               setup=_free(elision, per_launch, False))


def _chunk_stats(forced):
    """the collision proof held: no chunk was rolled back and replayed tick by tick.  Unforced: every tick a fast one.  Forced: the
    pending accumulators send the first tick the careful way (no pairs: integrate_free's EXT form, in place), the rest are fast."""
    def check(w, ticks):
        st = w.collision_stats()
        assert st["pair_ticks"] == 0
        want = (ticks - 1, 1) if forced else (ticks, 0)
        assert (st["fast_ticks"], st["careful_ticks"]) == want, (st, ticks)
    return check


@pytest.mark.parametrize("per_launch", [1, 7])
@pytest.mark.parametrize("elision", [0, 1, 2, 3])
def test_integrate_free_in_chunks_whose_first_launch_is_out_of_place(elision, per_launch):
    """the collision proof on, on the CALM populations (horizontal velocities of at most 0.05 m/s: in 64 ticks nobody leaves its
    0.1 m safe zone, so no chunk is rolled back -- the counters say so): a chunk's first launch writes the other slab, the ones
    behind it run in place, 7 ticks at a time where asked, and THEIR results are what is compared."""
    for forced in (False, True):
        _path_against_baseline(f"integrate_free elision {elision}, {per_launch} per launch, chunks, forced {forced}", forced, calm=True,
                               setup=_free(elision, per_launch, True), after_case=_chunk_stats(forced))


@pytest.mark.parametrize("per_launch", [1, 7])
@pytest.mark.parametrize("elision", [2, 3])
@pytest.mark.parametrize("cls", ["k3", "k30", "k1000"])
def test_integrate_free_with_uniform_constants_as_kernel_arguments(cls, elision, per_launch):
    """ONE mass (2) and ONE anisotropic inertia for all bodies: with bit 1 of the mask the batch passes them as kernel arguments
    (the OPT_UNI instantiations, the default kernel of uniform batches) -- here with random orientations, every spin regime, all
    three gyro modes, forces and torques; in place and in the collision proof's chunks; against elision 0 and against the oracle."""
    for forced in (True, False):
        what = f"integrate_free uniform {cls}, elision {elision}, {per_launch} per launch, forced {forced}"
        _path_against_baseline(what + ", in place", forced, uniform=cls, oracle_too=True, setup=_free(elision, per_launch, False))
        _path_against_baseline(what + ", chunks", forced, uniform=cls, calm=True, oracle_too=True, setup=_free(elision, per_launch, True),
                               after_case=_chunk_stats(forced))


def _no_contacts(w):
    assert w.last_contact_count() == 0
    assert w.collision_stats()["pair_ticks"] == 0


@pytest.mark.parametrize("forced", [True, False], ids=["forced", "unforced"])
def test_step_plane_with_the_plane_out_of_reach(forced):
    _path_against_baseline("step_plane", forced, plane=PLANE, after=_no_contacts)


@pytest.mark.parametrize("forced", [True, False], ids=["forced", "unforced"])
def test_step_contacts_with_the_static_box_out_of_reach(forced):
    _path_against_baseline("step_contacts", forced, statics=FAR_BOX, setup=lambda w: w.set_static_path(fused=True), after=_no_contacts)


_EMPTY = np.zeros(0, B_.CONTACT_JOINT_DTYPE)


def _step_joints(w, ticks):
    for _ in range(ticks):
        w.step_joints(H, _EMPTY)


@pytest.mark.parametrize("forced", [True, False], ids=["forced", "unforced"])
@pytest.mark.parametrize("stepper", ["quick", "exact"])
def test_island_path_without_joints(stepper, forced):
    def setup(w):
        w.set_small_tick(B_.SMALL_TICK_OFF)
        w.set_stepper(B_.STEPPER_EXACT if stepper == "exact" else B_.STEPPER_QUICK)

    def general(w):
        st = w.small_tick_stats()
        assert st["small"] == 0 and st["general"] > 0
    _path_against_baseline(f"island path ({stepper})", forced, setup=setup, step=_step_joints, after=general)


@pytest.mark.parametrize("forced", [True, False], ids=["forced", "unforced"])
def test_exact_tick_without_pairs_is_integrate_free_in_place(forced):
    """dmxBatchExactTick with no body in a pair: the pair search finds nothing and everybody is stepped by integrate_free, in place
    and unchecked, one launch per tick (NOT the island copy: step_joints above runs that one)"""
    def step(w, ticks):
        for _ in range(ticks):
            w.exact_tick(H)

    def careful(w, ticks):
        st = w.collision_stats()
        assert st["careful_ticks"] == ticks and st["pair_ticks"] == 0, st
    _path_against_baseline("exact tick", forced, step=step, after_case=careful)


@pytest.mark.parametrize("forced", [True, False], ids=["forced", "unforced"])
@pytest.mark.parametrize("stepper", ["quick", "exact"])
def test_small_world_tick(stepper, forced):
    """the first 300 bodies, one launch per tick: the small-tick counters say that the path was taken, every tick"""
    taken = []

    def setup(w):
        w.set_small_tick(B_.SMALL_TICK_AUTO)
        w.set_stepper(B_.STEPPER_EXACT if stepper == "exact" else B_.STEPPER_QUICK)

    def small(w):
        st = w.small_tick_stats()
        assert st["general"] == 0 and st["small"] in (1, ir.N_TICKS), st
        taken.append(st["small"])
    _path_against_baseline(f"small_world_tick ({stepper})", forced, n=SMALL_N, setup=setup, step=_step_joints, after=small)
    assert sorted(set(taken)) == [1, ir.N_TICKS]
