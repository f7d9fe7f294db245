"""Auto-disable on the device (dmxBatchSetAutoDisable, DMX_BODY_AUTODISABLE / DMX_BODY_DISABLED) through BatchWorld, both
precisions, both steppers, against tests/autodisable_reference.py.

Every tick is compared with the reference stepped from the device's own pre-tick state, flags and counters.  Awake bodies: the
tolerances of tests/test_gpu_solver_dense.py's `check` (the same lines; that file is unchanged).  Flags, counters and statistics:
exactly.  Bodies left out of the tick: bit for bit.  The reference's margin conditions (autodisable_reference.margin_ok) are
asserted on every compared tick: they are what lets a float32 device and a float64 reference name the same sleeping tick."""
import numpy as np
import pytest

import autodisable_reference as ar
import autodisable_scenes as sc
import lcp_dense as ld
import quick_band as qb
import test_gpu_solver_dense as sd
from __graft_entry__ import load_package

pkg = load_package()
B_ = pkg.batch
pytestmark = pytest.mark.gpu

PRECS = ["float64", "float32"]
STEPPERS = ["quick", "exact"]
A, K, AD, DIS = sc.A, sc.K, sc.AD, sc.DIS


def compare_awake(prec, stepper, r, Wr, post, live):
    """`check` of tests/test_gpu_solver_dense.py from the reference Result on: the device's post-tick state of the stepped slots"""
    if not len(live):
        return
    f32 = np.dtype(prec).itemsize == 4
    if f32 and stepper == "quick":
        qb.assert_in_band(r, Wr, post, qb.K["contact"], live)
        return
    t = (1e-10 if stepper == "quick" else 1e-8) if not f32 else 10 * sd.EPS32 * max([I.kappa() for I in r.islands] + [1.0])
    scale = ld.velocity_scale(r.bodies, Wr, live)
    err = ld.velocity_error(r.bodies, post[:, 7:10], post[:, 10:13], live)
    assert err <= t * scale, f"velocity error {err:.3e} > {t:.1e} x {scale:.3e}"
    eps = 4 * (sd.EPS32 if f32 else 2.2e-16)
    xerr = np.max(np.abs(post[live, 0:3] - r.bodies.pos[live]))
    assert xerr <= t * scale * Wr.h + eps * max(1.0, np.max(np.abs(r.bodies.pos[live]))), f"position error {xerr:.3e}"
    qerr = np.max(np.abs(post[live, 3:7] - r.bodies.quat[live]))
    assert qerr <= t * scale * Wr.h + eps, f"quaternion error {qerr:.3e}"


def make_world(prec, scene, stepper, small=None, feature=True):
    B, W = scene.B, scene.W
    w = B_.BatchWorld(B.n, prec, gravity=tuple(W.gravity))
    w.set_erp(W.erp); w.set_cfm(W.cfm); w.set_quickstep(W.iters, W.sor_w); w.set_gyro_mode(W.gyro)
    w.set_stepper(B_.STEPPER_EXACT if stepper == "exact" else B_.STEPPER_QUICK)
    if small is not None:
        w.set_small_tick(small)
    if feature:
        p = scene.params
        w.set_auto_disable(p.lin, p.ang, p.idle_steps, p.idle_time)
    w.upload(B_.POS, B.pos); w.upload(B_.QUAT_RAW, B.quat); w.upload(B_.LVEL, B.lvel); w.upload(B_.AVEL, B.avel)
    w.upload(B_.MASS, B.mass); w.upload(B_.INERTIA, B.inertia)
    w.upload_body_flags(B.flags)
    if scene.links:
        w.set_joints([w.joint_from_world(B_.JOINT_HINGE, b1, b2, 0.5 * (B.pos[b1] + B.pos[b2]), (0.0, 0.0, 1.0)) for b1, b2 in scene.links])
    return w


def run_device(prec, scene, stepper, small=None, compare=True):
    """the scene on the device, tick by tick -> list of (state (n, 13) float64, flags, steps_left, time_left, stats, small stats,
    contact count) after every tick; with `compare`, each tick is held to the reference as the module's docstring says"""
    B, W, p = scene.B, scene.W, scene.params
    w = make_world(prec, scene, stepper, small)
    try:
        mass = w.download(B_.MASS).astype(np.float64).reshape(-1)
        inertia = w.download(B_.INERTIA).astype(np.float64)
        out, slept, woken = [], 0, 0
        for t in range(scene.ticks):
            if t in scene.uploads:
                w.upload_body_flags(scene.uploads[t])
            j = scene.joints(t)
            pre = w.download(B_.STATE).astype(np.float64)
            flags = w.body_flags()
            st, tl = w.idle_counters()
            w.step_joints(W.h, j.astype(B_.CONTACT_JOINT_DTYPE))
            post = w.download(B_.STATE).astype(np.float64)
            got = (post, w.body_flags(), *w.idle_counters(), w.auto_disable_stats(), w.small_tick_stats(), w.last_contact_count())
            out.append(got)
            if not compare:
                continue
            Wr, jr = sd.as_precision(prec, W, j)
            Bp = ld.Bodies(pre[:, 0:3], pre[:, 3:7], pre[:, 7:10], pre[:, 10:13], mass, inertia, flags)
            tk = ar.step(Bp, Wr, jr, stepper, p, ar.Counters(B.n, p, st, tl), scene.links, h_idle=W.h)
            assert ar.margin_ok(tk, p, W.h), f"tick {t}: the reference does not keep the margin conditions"
            assert np.array_equal(got[1], tk.bodies.flags), (t, got[1], tk.bodies.flags)
            assert np.array_equal(got[2], tk.counters.steps), (t, got[2], tk.counters.steps)
            assert np.array_equal(got[3], tk.counters.time), (t, got[3], tk.counters.time)
            left_out = [s for s in range(B.n) if s not in tk.stepped]
            assert np.array_equal(post[left_out], pre[left_out]), f"tick {t}: a slot the tick leaves out changed"
            assert np.all(post[tk.slept, 7:13] == 0.0), f"tick {t}: a body fell asleep with a velocity"
            compare_awake(prec, stepper, tk.result, Wr, post, np.array(tk.stepped, int))
            slept += len(tk.slept); woken += len(tk.woken)
            asleep = int(np.sum((tk.bodies.flags & (A | DIS)) == (A | DIS)))
            assert got[4] == {"asleep": asleep, "islands_skipped": tk.skipped_islands, "slept": slept, "woken": woken}, (t, got[4])
            assert got[6] == tk.contacts, (t, got[6], tk.contacts)
        return out
    finally:
        w.close()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("name", sorted(sc.SCENES))
def test_scene_tick_by_tick_against_the_reference(name, stepper, prec):
    scene = sc.SCENES[name](stepper)
    out = run_device(prec, scene, stepper)
    flags = out[-1][1]
    # what the CPU test holds the reference to, on the device's own flags (the per-tick comparison has tied the two together)
    if name.startswith("free-") and scene.B.n >= 8:
        assert not flags[4] & DIS and not flags[5] & DIS and not flags[6] & DIS and flags[0] & DIS and not flags[1] & DIS
    if name == "apex-sleeps":
        assert [bool(o[1][0] & DIS) for o in out] == [False] * 4 + [True] * 8
    if name == "apex-stays-awake":
        assert not any(o[1][0] & DIS for o in out)
    if name == "settling" and stepper == "exact":
        assert [int(np.sum(o[1] & DIS != 0)) for o in out] == [0] * 9 + [10] * 4
    if name == "settling" and stepper == "quick":
        assert [list(np.nonzero(o[1] & DIS)[0]) for o in out[9:]] == [[0]] * 4
    if name == "settling-loose":
        assert [int(np.sum(o[1] & DIS != 0)) for o in out] == [0] * 9 + [4] * 4
    if name == "waking":
        assert [o[4]["woken"] for o in out] == [0, 0, 0, 3, 3]
    assert out[-1][5]["small"] == scene.ticks                # these scenes are the single-launch tick's


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("name", ["free-65", "free-130", "settling", "waking"])
def test_small_tick_parity(name, stepper, prec):
    """SMALL_TICK_AUTO against SMALL_TICK_OFF: bit-identical state, flags and counters, the statistics naming the path"""
    scene = sc.SCENES[name](stepper)
    a = run_device(prec, scene, stepper, small=B_.SMALL_TICK_AUTO, compare=False)
    b = run_device(prec, scene, stepper, small=B_.SMALL_TICK_OFF, compare=False)
    assert a[-1][5]["small"] == scene.ticks and a[-1][5]["general"] == 0
    assert b[-1][5]["small"] == 0 and b[-1][5]["general"] == scene.ticks and b[-1][5]["mode"] == scene.ticks
    for t, (x, y) in enumerate(zip(a, b)):
        for k in (0, 1, 2, 3):
            assert np.array_equal(x[k], y[k]), (t, k)
        assert x[4] == y[4] and x[6] == y[6], t


def all_forms(stepper):
    """every solver form in one world, from cases tests/test_gpu_solver_dense.py already holds the solvers to: its mixed islands
    (slots 0 and 1: one body with 4 and with 3 contacts; 2..6: an island for a workgroup; 7..86: 960 rows -- under dWorldStep past
    the LDS solve, the grid's), its one-body islands of 1..8 contacts (87..94) and five free bodies (95..99).  idle_steps = 1 and
    thresholds far above every speed: every body with the bit sleeps at the end of its first tick, whichever form stepped it.
    Slot 1 and the last slot are without the bit"""
    parts = [sd.mixed_islands_case()] + [sd.single_case(nc) for nc in range(1, 9)]
    Bs, js, off = [], [], 0
    for k, (B, j) in enumerate(parts):
        B.pos[:, 0] += 100.0 * k
        j = j.copy(); j["pos"][:, 0] += 100.0 * k
        j["body1"] += off; j["body2"] = np.where(j["body2"] >= 0, j["body2"] + off, -1)
        Bs.append(B); js.append(j); off += B.n
    rng = np.random.default_rng(77)
    Bs.append(sc.bodies(np.column_stack([np.arange(5) * 2.0, np.full(5, 50.0), np.zeros(5)]), rng.normal(size=(5, 3))))
    B = ld.Bodies(*[np.vstack([getattr(b, f) for b in Bs]) for f in ("pos", "quat", "lvel", "avel")],
                  np.concatenate([b.mass for b in Bs]), np.vstack([b.inertia for b in Bs]))
    B.flags[:] = A | AD
    B.flags[1] = A; B.flags[-1] = A
    j = np.concatenate(js)
    return sc.Scene(B, sd.world("float32"), ar.Params(lin=1e3, ang=1e3, idle_steps=1, idle_time=0.0), 3, joints=lambda t: j)


N_ISLANDS = 4 + 8 + 5


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
def test_every_solver_form_in_one_tick_and_the_large_island_asleep(stepper, prec):
    scene = all_forms(stepper)
    n = scene.B.n
    assert n == 100
    out = run_device(prec, scene, stepper)
    flags = out[0][1]
    with_bit = np.array([s for s in range(n) if s not in (1, n - 1)])
    assert np.all(flags[with_bit] & DIS) and not flags[1] & DIS and not flags[n - 1] & DIS
    assert np.all(out[0][0][with_bit, 7:13] == 0.0)
    assert out[0][5]["general"] == 1           # (960 rows: not the single-launch tick's)
    # ticks 1, 2: every island but the two without the bit is left out
    assert out[1][4]["islands_skipped"] == N_ISLANDS - 2 and out[2][4]["islands_skipped"] == N_ISLANDS - 2
    assert out[1][6] == 3 and out[2][6] == 3                  # slot 1's three contacts are all that count
    assert out[2][5]["small"] == 2             # ... and what is left is the single-launch tick's (its mirror filled whole at tick 1)


@pytest.mark.parametrize("prec", PRECS)
def test_asleep_large_island_costs_no_solve_and_reports_zero_feedback(prec):
    scene = all_forms("exact")
    n = scene.B.n
    w = make_world(prec, scene, "exact")
    try:
        w.set_feedback(True)
        j = scene.joints(0).astype(B_.CONTACT_JOINT_DTYPE)
        w.step_joints(scene.W.h, j)
        solves = w.lcp_stats()["solves"]
        assert solves == 1 and w.last_contact_count() == len(j)
        fb = w.contact_feedback()
        big = np.nonzero((j["body1"] >= 7) & (j["body1"] <= 86))[0]
        assert len(big) == 320 and np.any(fb[big] != 0.0)
        state = w.download(B_.STATE)
        for _ in range(2):
            w.step_joints(scene.W.h, j)
            assert w.lcp_stats()["solves"] == solves
            assert w.auto_disable_stats()["islands_skipped"] == N_ISLANDS - 2 and w.last_contact_count() == 3
            fb = w.contact_feedback()
            assert np.all(fb[j["body1"] != 1] == 0.0) and np.any(fb[j["body1"] == 1] != 0.0)
        after = w.download(B_.STATE)
        keep = [s for s in range(n) if s not in (1, n - 1)]
        assert np.array_equal(after[keep], state[keep])
    finally:
        w.close()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("small", [B_.SMALL_TICK_AUTO, B_.SMALL_TICK_OFF])
def test_uploads_and_counters(prec, small):
    p = ar.Params(lin=0.1, ang=0.1, idle_steps=4, idle_time=0.0)
    lvel = np.zeros((3, 3)); lvel[:, 0] = (0.05, 0.05, 3.0)
    scene = sc.Scene(sc.bodies(np.zeros((3, 3)), lvel, flags=[A | AD, A | AD, A]), sc.world(gravity=(0, 0, 0)), p, 1)
    w = make_world(prec, scene, "quick", small)
    none = np.zeros(0, B_.CONTACT_JOINT_DTYPE)
    try:
        assert w.auto_disable() == (0.1, 0.1, 4, 0.0)
        for _ in range(2):
            w.step_joints(sc.H, none)
        assert list(w.idle_counters()[0]) == [2, 2, 4]
        w.upload_body_flags(w.body_flags())                   # unchanged: the counters stand
        assert list(w.idle_counters()[0]) == [2, 2, 4]
        for _ in range(2):
            w.step_joints(sc.H, none)
        assert list(w.body_flags()) == [A | AD | DIS, A | AD | DIS, A] and list(w.idle_counters()[0]) == [0, 0, 4]
        assert np.all(w.download(B_.LVEL)[:2] == 0.0)
        w.upload_body_flags([A | AD, A | AD | DIS, A | DIS])      # 0: DISABLED cleared -> reset; 1: as it was; 2: asleep by hand
        assert list(w.idle_counters()[0]) == [4, 0, 4]
        before = w.download(B_.STATE)
        w.step_joints(sc.H, none)
        after = w.download(B_.STATE)
        assert np.array_equal(after[1:], before[1:]) and after[2, 7] == np.dtype(prec).type(3.0)      # left out, velocities untouched
        assert list(w.body_flags()) == [A | AD, A | AD | DIS, A | DIS] and list(w.idle_counters()[0]) == [3, 0, 4]
        assert w.auto_disable_stats() == {"asleep": 2, "islands_skipped": 2, "slept": 2, "woken": 0}
        w.upload_body_flags([A | AD, A | AD, A | AD])             # 2: AUTODISABLE clear -> set resets too (it stood at 4 anyway); 1: reset
        assert list(w.idle_counters()[0]) == [3, 4, 4]
        w.set_auto_disable(0.1, 0.1, 7, 2.5 * sc.H)               # resets every slot's
        st, tl = w.idle_counters()
        assert list(st) == [7, 7, 7] and list(tl) == [2.5 * sc.H] * 3
        for bad in ((-1.0, 0.1, 1, 0.0), (0.1, -1.0, 1, 0.0), (0.1, 0.1, -1, 0.0), (0.1, 0.1, 1, -1.0), (float("nan"), 0.1, 1, 0.0)):
            with pytest.raises(B_.DmxError):
                w.set_auto_disable(*bad)
        assert w.auto_disable() == (0.1, 0.1, 7, 2.5 * sc.H)
    finally:
        w.close()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("name", ["free-130", "settling"])
def test_feature_off_is_bit_identical(name, stepper, prec):
    """the same scene without the bit: bit-identical to a run in which dmxBatchSetAutoDisable was never called; nothing sleeps"""
    scene = sc.SCENES[name](stepper)
    scene.B.flags &= np.uint8(~(AD | DIS) & 0xff)
    states = []
    for feature in (True, False):
        w = make_world(prec, scene, stepper, feature=feature)
        try:
            for t in range(scene.ticks):
                w.step_joints(scene.W.h, scene.joints(t).astype(B_.CONTACT_JOINT_DTYPE))
            states.append(w.download(B_.STATE))
            assert w.auto_disable_stats() == {"asleep": 0, "islands_skipped": 0, "slept": 0, "woken": 0}
            assert np.array_equal(w.body_flags(), scene.B.flags)
        finally:
            w.close()
    assert np.array_equal(states[0], states[1])


@pytest.mark.parametrize("bit", [AD, DIS])
def test_ticks_that_find_their_own_contacts_refuse_the_new_bits(bit):
    w = B_.BatchWorld(4, "float32", gravity=(0.0, -9.8, 0.0))
    try:
        w.upload(B_.POS, np.column_stack([np.arange(4) * 3.0, np.full(4, 5.0), np.zeros(4)]))
        w.upload_body_flags([A, A | bit, A, A])
        before = w.download(B_.STATE)
        with pytest.raises(B_.DmxError):
            w.step(sc.H, 1)
        assert np.array_equal(w.download(B_.STATE), before)
        w.upload_body_flags([A, A, A, A])
        w.step(sc.H, 1)
        assert not np.array_equal(w.download(B_.STATE), before)
    finally:
        w.close()
