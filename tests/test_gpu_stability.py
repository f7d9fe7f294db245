"""Damping, the maximum angular speed and the contact correction scalars (include/dmx_batch.h, "damping") on the device, through
BatchWorld, against tests/stability_reference.py.

Every tick is compared with the reference stepped from the device's own pre-tick state, with the tolerances of
tests/test_gpu_solver_dense.py's `check` (and, for the scene with articulation joints, of tests/test_gpu_joints.py's `compare`):
float64 QuickStep 1e-10, float64 dWorldStep 1e-8, float32 dWorldStep 10 eps32 kappa(A), float32 QuickStep the band of
tests/quick_band.py with its K -- unchanged: damping multiplies a velocity by a number below one and the cap by max / |w| <= 1, one
or three more roundings of a quantity the band already scales with.  The threshold is the feature's one discontinuity, so every
compared tick must keep stability_reference.margin_ok, which is asserted.  The scenes are tests/stability_scenes.py's: one per
place the knobs live in the device code, with both sides of every knob in each (held by tests/test_stability_reference.py)."""
import numpy as np
import pytest

import autodisable_reference as ar
import feedback_dense as fd
import lcp_dense as ld
import quick_band as qb
import stability_reference as sr
import stability_scenes as sc
import test_gpu_joints as gj
import test_gpu_solver_dense as sd
from __graft_entry__ import load_package

pkg = load_package()
B_ = pkg.batch
pytestmark = pytest.mark.gpu

PRECS = ["float64", "float32"]
EINVAL = -3                  # DMX_EINVAL
AUTO, OFF = B_.SMALL_TICK_AUTO, B_.SMALL_TICK_OFF
CASES = [(n, st) for n in sc.SCENES for st in sc.SCENES[n]().steppers]
SMALL_CASES = [(n, st) for n, st in CASES if n in sc.SMALL_SCENES]
DEFAULT_TABLE = np.array([sr.DEFAULT_ENTRY])


def make_world(prec, s, stepper, small=None, knobs="scene", flags=None):
    """knobs: "scene" (the scene's), "never" (no call made), "reset" (the scene's set, then every value put back to its default)"""
    B, W = s.B, s.W
    w = B_.BatchWorld(B.n, prec, gravity=tuple(W.gravity))
    w.set_erp(W.erp); w.set_cfm(W.cfm); w.set_quickstep(W.iters, W.sor_w); w.set_gyro_mode(W.gyro)
    w.set_stepper(B_.STEPPER_EXACT if stepper == "exact" else B_.STEPPER_QUICK)
    if small is not None:
        w.set_small_tick(small)
    w.upload(B_.POS, B.pos); w.upload(B_.QUAT_RAW, B.quat); w.upload(B_.LVEL, B.lvel); w.upload(B_.AVEL, B.avel)
    w.upload(B_.MASS, B.mass); w.upload(B_.INERTIA, B.inertia)
    w.upload_body_flags(B.flags if flags is None else flags)
    if s.art is not None:
        w.set_joints(gj.to_c(s.art))
    if knobs != "never":
        w.upload_body_damping(s.knobs.table)
        w.set_contact_correction(s.knobs.surface_layer, s.knobs.max_correcting_vel)
    if knobs == "reset":
        w.set_damping(0.0, 0.0, 0.01, 0.01)
        w.set_max_angular_speed(np.inf)
        w.set_contact_correction(0.0, np.inf)
    return w


def compare(prec, stepper, r, Wr, post, live, joint_inputs=None):
    """sd.check from the reference Result on (as test_gpu_autodisable.compare_awake), with gj.compare's band when joints are set"""
    f32 = np.dtype(prec).itemsize == 4
    if f32 and stepper == "quick":
        K = qb.K["contact"]
        if joint_inputs is not None:
            qb.attach_joint_term(r, *joint_inputs)
            K = qb.K["joint"]
        worst = qb.assert_in_band(r, Wr, post, K, live)
        print(f"f32 QuickStep on the device: {worst:.2f} eps32 M_v (K = {K})")
        return
    t = (1e-10 if stepper == "quick" else 1e-8) if not f32 else 10 * sd.EPS32 * max([I.kappa() for I in r.islands] + [1.0])
    scale = ld.velocity_scale(r.bodies, Wr, live)
    err = ld.velocity_error(r.bodies, post[:, 7:10], post[:, 10:13], live)
    print(f"{prec} {stepper}: velocity error {err:.3e}, allowed {t:.1e} x {scale:.3e}")
    assert err <= t * scale, f"velocity error {err:.3e} > {t:.1e} x {scale:.3e}"
    eps = 4 * (sd.EPS32 if f32 else 2.2e-16)
    xerr = np.max(np.abs(post[live, 0:3] - r.bodies.pos[live]))
    assert xerr <= t * scale * Wr.h + eps * max(1.0, np.max(np.abs(r.bodies.pos[live]))), f"position error {xerr:.3e}"
    qerr = np.max(np.abs(post[live, 3:7] - r.bodies.quat[live]))
    assert qerr <= t * scale * Wr.h + eps, f"quaternion error {qerr:.3e}"
    return t


def reference_inputs(prec, s, jts):
    """world, contact joints, articulation joints and knobs in the values a batch of this precision holds"""
    if s.art is not None:
        Wr, jr, art = gj.as_precision(prec, s.W, jts, s.art)
    else:
        (Wr, jr), art = sd.as_precision(prec, s.W, jts), None
    return Wr, jr, art, s.knobs.as_precision(prec)


def run(prec, s, stepper, small=None, ticks=None, check=True, knobs="scene"):
    """-> (post states per tick, small-tick stats, lcp stats, reference Results)"""
    w = make_world(prec, s, stepper, small, knobs)
    try:
        mass = w.download(B_.MASS).astype(np.float64).reshape(-1)
        inertia = w.download(B_.INERTIA).astype(np.float64)
        Wr, jr, art, k = reference_inputs(prec, s, s.jts)
        out, refs = [], []
        for t in range(s.ticks if ticks is None else ticks):
            pre = w.download(B_.STATE).astype(np.float64)
            w.step_joints(s.W.h, s.jts.astype(B_.CONTACT_JOINT_DTYPE))
            w.synchronize()
            post = w.download(B_.STATE).astype(np.float64)
            out.append(post)
            for slot in (s.kinematic, s.slow):
                assert np.array_equal(post[slot, 7:13], pre[slot, 7:13]), f"tick {t}: slot {slot} must keep its velocity bits"
            if not check:
                continue
            Bp = ld.Bodies(pre[:, 0:3], pre[:, 3:7], pre[:, 7:10], pre[:, 10:13], mass, inertia, s.B.flags)
            r = sr.step(Bp, Wr, jr, stepper, k, art)
            assert sr.margin_ok(r), f"tick {t}: a speed within {sr.MARGIN} of its damping threshold"
            compare(prec, stepper, r, Wr, post, np.arange(s.B.n), None if art is None else (r.damped, Wr, jr, art))      # (the bodies the rows were built from)
            refs.append(r)
        return out, w.small_tick_stats(), w.lcp_stats(), refs
    finally:
        w.close()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,stepper", CASES)
def test_scene_tick_by_tick_against_the_reference(name, stepper, prec):
    s = sc.SCENES[name]()
    out, tick, lcp, refs = run(prec, s, stepper)
    n = len(out)
    # which form ran
    if name in sc.SMALL_SCENES:
        assert tick["small"] == n and tick["general"] == 0
    else:
        assert tick["small"] == 0 and tick["general"] == n
    if name.startswith("quick-") or name.startswith("exact-"):
        assert max(I.m for I in refs[0].islands) == int(name.split("-")[-1])
    if stepper == "exact":
        assert (lcp["solves"] > 0) == s.grid and lcp["fallback"] == 0
        if s.grid:
            big = max(refs[0].islands, key=lambda I: I.m)
            assert (lcp["last_m"], lcp["last_nu"], lcp["last_nbd"]) == (big.m, big.nu, big.nbd)
    # the knobs acted on the device: the fast spinner ends on its cap (to rounding)
    spinner = s.B.n - 4
    mx = s.knobs.as_precision(prec).table[spinner, sr.MAX_ANG_SPEED]
    assert abs(np.linalg.norm(out[0][spinner, 10:13]) - mx) <= 4 * sd.EPS32 * mx


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,stepper", SMALL_CASES)
def test_single_launch_tick_against_general_path(name, stepper, prec):
    """set_small_tick AUTO and OFF agree bit for bit over 8 ticks, the statistics naming the path"""
    s = sc.SCENES[name]()
    a, ta, _, _ = run(prec, s, stepper, AUTO, ticks=8, check=False)
    b, tb, _, _ = run(prec, s, stepper, OFF, ticks=8, check=False)
    assert ta["small"] == 8 and ta["general"] == 0
    assert tb["small"] == 0 and tb["general"] == 8 and tb["mode"] == 8
    for t, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), t


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("small", [AUTO, OFF])
@pytest.mark.parametrize("name,stepper", [("single-4", "quick"), ("single-8", "quick"), ("stack-2", "quick"), ("stack-2", "exact"), ("quick-260", "quick"),
                                          ("exact-lds-30", "exact"), ("exact-grid-300", "exact"), ("hinge-chain", "quick"), ("hinge-chain", "exact")])
def test_defaults_are_bit_identical(name, stepper, small, prec):
    """a world whose knobs were set and put back, and one that never touched them, against each other over 3 ticks: the latter
    makes no table, launches no damping pass and hands finish_body a null pointer -- the run of a library without the feature;
    and both differ from the run with the knobs on"""
    s = sc.SCENES[name]()
    never, _, _, _ = run(prec, s, stepper, small, ticks=3, check=False, knobs="never")
    reset, _, _, _ = run(prec, s, stepper, small, ticks=3, check=False, knobs="reset")
    on, _, _, _ = run(prec, s, stepper, small, ticks=3, check=False)
    for t in range(3):
        assert np.array_equal(never[t], reset[t]), t
    assert not np.array_equal(never[0], on[0])


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("small", [AUTO, OFF])
@pytest.mark.parametrize("stepper", ["quick", "exact"])
def test_with_auto_disable_asleep_islands_are_not_damped(stepper, small, prec):
    """flags, counters and statistics match autodisable_reference driven with the damped tick (stability_reference.step_autodisable);
    the slots of asleep islands keep every bit; the idle rule sees the post-step velocities"""
    s, p = sc.sleepy_scene()
    w = make_world(prec, s, stepper, small)
    try:
        w.set_auto_disable(p.lin, p.ang, p.idle_steps, p.idle_time)
        w.upload_body_flags(s.B.flags)                      # (the counters start from the values just set)
        mass = w.download(B_.MASS).astype(np.float64).reshape(-1)
        inertia = w.download(B_.INERTIA).astype(np.float64)
        Wr, jr, _, k = reference_inputs(prec, s, s.jts)
        slept_total = 0
        for t in range(s.ticks):
            pre = w.download(B_.STATE).astype(np.float64)
            flags = w.body_flags()
            st, tl = w.idle_counters()
            w.step_joints(s.W.h, s.jts.astype(B_.CONTACT_JOINT_DTYPE))
            post = w.download(B_.STATE).astype(np.float64)
            Bp = ld.Bodies(pre[:, 0:3], pre[:, 3:7], pre[:, 7:10], pre[:, 10:13], mass, inertia, flags)
            tk = sr.step_autodisable(Bp, Wr, jr, stepper, k, p, ar.Counters(s.B.n, p, st, tl))
            assert sr.margin_ok(tk.result) and ar.margin_ok(tk, p, s.W.h), t
            assert np.array_equal(w.body_flags(), tk.bodies.flags), t
            got_st, got_tl = w.idle_counters()
            assert np.array_equal(got_st, tk.counters.steps) and np.array_equal(got_tl, tk.counters.time), t
            left_out = [x for x in range(s.B.n) if x not in tk.stepped]
            assert len(left_out) >= 4 and np.array_equal(post[left_out], pre[left_out]), f"tick {t}: an asleep slot changed"
            assert np.all(post[tk.slept, 7:13] == 0.0)
            awake = np.array([x for x in tk.stepped if x not in tk.slept], int)
            compare(prec, stepper, tk.result, Wr, post, awake)
            slept_total += len(tk.slept)
            stats = w.auto_disable_stats()
            assert stats["islands_skipped"] == tk.skipped_islands and stats["slept"] == slept_total, (t, stats)
        assert slept_total >= 2, "damping was to bring the slow free bodies under the sleep thresholds"
    finally:
        w.close()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("small", [AUTO, OFF])
@pytest.mark.parametrize("name,stepper", [("stack-2", "quick"), ("exact-lds-30", "exact")])
def test_feedback_with_the_modified_right_hand_sides(name, stepper, small, prec):
    """J^T lambda of every contact against feedback_dense on the reference's tick, with test_gpu_feedback.py's rule: a velocity
    error dv is a force error m dv / h"""
    s = sc.SCENES[name]()
    w = make_world(prec, s, stepper, small)
    try:
        w.set_feedback(True)
        mass = w.download(B_.MASS).astype(np.float64).reshape(-1)
        inertia = w.download(B_.INERTIA).astype(np.float64)
        Wr, jr, _, k = reference_inputs(prec, s, s.jts)
        pre = w.download(B_.STATE).astype(np.float64)
        w.step_joints(s.W.h, s.jts.astype(B_.CONTACT_JOINT_DTYPE))
        post = w.download(B_.STATE).astype(np.float64)
        fc = w.contact_feedback(len(s.jts))
        Bp = ld.Bodies(pre[:, 0:3], pre[:, 3:7], pre[:, 7:10], pre[:, 10:13], mass, inertia, s.B.flags)
        r = sr.step(Bp, Wr, jr, stepper, k)
        assert sr.margin_ok(r)
        ref = fd.feedback(Bp, r, jr)
        f32 = np.dtype(prec).itemsize == 4
        t = (1e-10 if stepper == "quick" else 1e-8) if not f32 else 10 * sd.EPS32 * max([I.kappa() for I in r.islands] + [1.0])
        eps = sd.EPS32 if f32 else 2.2e-16
        vscale = ld.velocity_scale(r.bodies, Wr, np.arange(s.B.n))
        assert np.any(ref.contacts != 0)
        for n, I in enumerate(r.islands):
            mine = ref.contacts[ref.contact_island == n].reshape(-1, 4, 3)
            if not len(mine):
                continue
            fmax, tmax = np.max(np.abs(mine[:, 0::2])), np.max(np.abs(mine[:, 1::2]))
            Ff, Ft = max(fmax, np.max(Bp.mass[I.slots]) * vscale / Wr.h), max(tmax, np.max(Bp.inertia[I.slots]) * vscale / Wr.h)
            for c in np.nonzero(ref.contact_island == n)[0]:
                assert np.max(np.abs(fc[c][0::2] - ref.contacts[c][0::2])) <= t * Ff + 4 * eps * fmax, c
                assert np.max(np.abs(fc[c][1::2] - ref.contacts[c][1::2])) <= t * Ft + 4 * eps * tmax, c
    finally:
        w.close()


# ---------------------------------------------------------------------------------------------------------------------
def plain_world(prec="float32", n=8):
    w = B_.BatchWorld(n, prec)
    w.upload(B_.POS, np.column_stack([3.0 * np.arange(n), np.full(n, 2.0), np.zeros(n)]))
    w.upload(B_.QUAT_RAW, np.tile([1.0, 0, 0, 0], (n, 1)))
    w.upload(B_.LVEL, np.full((n, 3), 0.5)); w.upload(B_.AVEL, np.full((n, 3), 0.25))
    w.upload(B_.MASS, np.ones(n)); w.upload(B_.INERTIA, np.ones((n, 3)))
    return w


def refused(f, *a):
    with pytest.raises(B_.DmxError) as e:
        f(*a)
    assert e.value.code == EINVAL


@pytest.mark.parametrize("how", ["entry", "layer"])
def test_ticks_that_find_their_own_contacts_refuse(how):
    """step, step_range, exact_tick and chunk_tick return DMX_EINVAL and change nothing while one slot holds a non-default entry,
    or the layer is not zero; they run again after a reset"""
    w = plain_world()
    try:
        if how == "entry":
            t = np.tile(DEFAULT_TABLE, (1, 1))
            t[0, sr.ANG_SCALE] = 0.01
            w.upload_body_damping(t, first=5)
        else:
            w.set_contact_correction(0.001, np.inf)
        before = w.download(B_.STATE)
        h = 1.0 / 60.0
        refused(w.step, h, 1)
        refused(w.step_range, h, 0, 8)
        refused(w.exact_tick, h)
        refused(w.step_timed, h, 1)
        w.chunk_begin()
        refused(w.chunk_tick, h, True)
        refused(w.chunk_ticks, h, 2, True, True)
        w.chunk_end()
        w.chunk_rollback()
        assert np.array_equal(w.download(B_.STATE), before)
        w.step_joints(h, np.zeros(0, B_.CONTACT_JOINT_DTYPE))          # the joints tick honours them
        if how == "entry":
            w.upload_body_damping(DEFAULT_TABLE, first=5)
        else:
            w.set_contact_correction(0.0, np.inf)
        before = w.download(B_.STATE)
        w.step(h, 1)
        w.step_range(h, 0, 8)
        w.exact_tick(h)
        assert not np.array_equal(w.download(B_.STATE), before)
    finally:
        w.close()


@pytest.mark.parametrize("prec", PRECS)
def test_invalid_values_change_nothing_and_uploads_round_trip(prec):
    w = plain_world(prec)
    try:
        assert np.array_equal(w.body_damping().view(np.float64).reshape(-1, 5), np.tile(DEFAULT_TABLE, (8, 1)))      # never set: the defaults
        assert w.contact_correction() == (0.0, np.inf)
        rng = np.random.default_rng(1)
        t = np.column_stack([rng.uniform(0, 1, 8), rng.uniform(0, 1, 8), rng.uniform(0, 2, 8), rng.uniform(0, 2, 8), rng.uniform(0.1, 9, 8)])
        t[3] = sr.DEFAULT_ENTRY
        t[4, :2], t[5, :2], t[6, 2:4] = (0.0, 1.0), (1.0, 0.0), (0.0, 0.0)
        w.upload_body_damping(t[2:7], first=2)
        want = np.tile(DEFAULT_TABLE, (8, 1)); want[2:7] = t[2:7]
        assert np.array_equal(w.body_damping().view(np.float64).reshape(-1, 5), want)
        w.set_contact_correction(0.002, 3.0)
        for bad in ((-0.1, 0, 0, 0, 1), (1.5, 0, 0, 0, 1), (0, -1e-9, 0, 0, 1), (0, 1.0001, 0, 0, 1), (0, 0, -1, 0, 1), (0, 0, 0, -1, 1),
                    (0, 0, 0, 0, 0.0), (0, 0, 0, 0, -2.0), (np.nan, 0, 0, 0, 1), (0, 0, 0, np.nan, 1), (0, 0, 0, 0, np.nan)):
            both = np.array([sr.DEFAULT_ENTRY, bad])                  # (a valid entry ahead of the bad one is not taken either)
            refused(w.upload_body_damping, both, 0)
        refused(w.upload_body_damping, t, 1)                          # past the end
        for bad in ((-0.1, 0, 0.01, 0.01), (0, 2.0, 0.01, 0.01), (0, 0, -1.0, 0.01), (0, 0, 0.01, np.nan)):
            refused(w.set_damping, *bad)
        for bad in (0.0, -1.0, np.nan):
            refused(w.set_max_angular_speed, bad)
        for bad in ((-1e-3, 1.0), (np.inf, 1.0), (np.nan, 1.0), (0.0, 0.0), (0.0, -1.0), (0.0, np.nan)):
            refused(w.set_contact_correction, *bad)
        assert np.array_equal(w.body_damping().view(np.float64).reshape(-1, 5), want)
        assert w.contact_correction() == (0.002, 3.0)
        w.set_max_angular_speed(7.0)                                  # every slot's cap; the damping values stand
        want[:, 4] = 7.0
        assert np.array_equal(w.body_damping().view(np.float64).reshape(-1, 5), want)
        w.set_damping(0.1, 0.2, 0.3, 0.4)                             # ... and the other way round
        want[:, :4] = (0.1, 0.2, 0.3, 0.4)
        assert np.array_equal(w.body_damping().view(np.float64).reshape(-1, 5), want)
        assert w.body_damping()["max_angular_speed"][0] == 7.0 and w.body_damping().dtype == B_.BODY_DAMPING_DTYPE
    finally:
        w.close()
