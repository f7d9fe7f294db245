"""The extended contact surface (mu2, fdir1, motion1 / 2 / N, slip1 / 2) on the device, against the dense float64 restatement of the
definition (tests/surface_dense.py): dmxBatchStepJointsSurface, both steppers, both precisions, from the device's own downloaded
pre-tick state.

Scene builders, the run / check pattern, tolerances and the float32 margin gate are those of tests/test_gpu_friction.py (velocities
relative to max(|v_ref|, g h)):
  * float64 QuickStep 1e-10, float64 dWorldStep 1e-8;
  * float32 10 eps32 kappa(A), twice that where an island is solved in two passes (it has a pyramid row);
  * float32 QuickStep is compared only where the reference's clamp margin is above 1e-3 of the island's largest |lambda|: asserted,
    never used to skip -- the seeds at the foot of the file were chosen on the CPU, with the reference alone, so that it holds.
Every comparison case cycles the nine kinds of MIX over its contacts."""
import os
import subprocess
import sys

import numpy as np
import pytest

import autodisable_reference as adr
import feedback_dense as fbd
import lcp_dense as ld
import surface_dense as sf
import test_gpu_friction as gf
import test_gpu_solver_dense as sd
from __graft_entry__ import load_package

pkg = load_package()
B_ = pkg.batch
pytestmark = pytest.mark.gpu

H = sd.H
EPS32 = sd.EPS32
PRECS = ["float64", "float32"]
INF = np.inf
# (mode, mu, surface fields): FDIR1|MU2 box (0.5 / 0.2); the same with APPROX1; MU2 with mu2 = 0; mu = 0 with mu2 = 0.5;
# FDIR1|MOTION1|MOTION2; MOTIONN; SLIP1|SLIP2 with mu = inf; mu = inf with a finite mu2; a plain contact
MIX = [(sf.FDIR1 | sf.MU2, 0.5, dict(mu2=0.2)),
       (sf.FDIR1 | sf.MU2 | sf.APPROX1, 0.5, dict(mu2=0.2)),
       (sf.MU2, 0.5, dict(mu2=0.0)),
       (sf.MU2, 0.0, dict(mu2=0.5)),
       (sf.FDIR1 | sf.MOTION1 | sf.MOTION2, 0.5, dict(motion1=0.3, motion2=-0.2)),
       (sf.MOTIONN, 0.5, dict(motionN=0.1)),
       (sf.SLIP1 | sf.SLIP2, INF, dict(slip1=0.02, slip2=0.05)),
       (sf.MU2, INF, dict(mu2=0.3)),
       (0, 0.5, dict())]
# fields no bit selects carry values that would show if they were read
UNREAD = dict(mu2=7.0, motion1=5.0, motion2=-5.0, motionN=3.0, slip1=0.9, slip2=0.8)


def mix(jts, idx=None, start=0):
    """give the contacts `idx` (default: all) the nine kinds of MIX in turn -> (joints, surfaces); fdir1 is a unit vector
    orthogonal to the contact's normal"""
    jts = jts.copy()
    srf = sf.surfaces(len(jts), **UNREAD)
    srf["fdir1"] = (9.0, 9.0, 9.0)
    for k, i in enumerate(range(len(jts)) if idx is None else idx):
        mode, mu, fields = MIX[(k + start) % len(MIX)]
        jts["mode"][i] = int(jts["mode"][i]) | mode
        jts["mu"][i] = mu
        for name, v in fields.items():
            srf[name][i] = v
        if mode & sf.FDIR1:
            n = jts["normal"][i] / np.linalg.norm(jts["normal"][i])
            d = np.cross(n, (0.3, 0.5, 0.8))
            srf["fdir1"][i] = d / np.linalg.norm(d)
    return jts, srf


def as_precision(prec, W, jts, srf):
    Wr, jr = sd.as_precision(prec, W, jts)
    if np.dtype(prec).itemsize == 8:
        return Wr, jr, srf
    s2 = srf.copy()
    for f in s2.dtype.names:
        s2[f] = np.asarray(srf[f], np.float32).astype(np.float64)
    return Wr, jr, s2


def run(prec, B, W, jts, srf, stepper, small=B_.SMALL_TICK_OFF, feedback=False, order=None, expect_error=False, prime=None):
    """one dmxBatchStepJointsSurface tick (srf = None: dmxBatchStepJoints) -> (pre-tick Bodies as the device held them, post-tick
    state (n, 13), stats, contact feedback or None).  expect_error: the call must fail with DMX_EINVAL and leave the state -- and,
    with `prime` (joints, surfaces of a tick made first, feedback on), the feedback that tick left -- untouched"""
    w = B_.BatchWorld(B.n, prec, gravity=tuple(W.gravity))
    try:
        w.set_erp(W.erp); w.set_cfm(W.cfm); w.set_quickstep(W.iters, W.sor_w); w.set_gyro_mode(W.gyro)
        w.set_stepper(B_.STEPPER_EXACT if stepper == "exact" else B_.STEPPER_QUICK)
        w.set_small_tick(small)
        w.set_feedback(feedback or prime is not None)
        w.upload(B_.POS, B.pos); w.upload(B_.QUAT_RAW, B.quat); w.upload(B_.LVEL, B.lvel); w.upload(B_.AVEL, B.avel)
        w.upload(B_.MASS, B.mass); w.upload(B_.INERTIA, B.inertia)
        w.upload_body_flags(B.flags)
        before = None
        if prime is not None:
            w.step_joints(W.h, prime[0].astype(B_.CONTACT_JOINT_DTYPE), prime[1])
            before = w.contact_feedback()
            assert np.any(before != 0)
        if order is not None:
            w.set_row_order(order, 7)
        mass = w.download(B_.MASS).astype(np.float64).reshape(-1)
        inertia = w.download(B_.INERTIA).astype(np.float64)
        pre = w.download(B_.STATE).astype(np.float64)
        Bp = ld.Bodies(pre[:, 0:3], pre[:, 3:7], pre[:, 7:10], pre[:, 10:13], mass, inertia, B.flags)
        cs = None if srf is None else srf.astype(B_.CONTACT_SURFACE_DTYPE)
        if expect_error:
            with pytest.raises(B_.DmxError) as e:
                w.step_joints(W.h, jts.astype(B_.CONTACT_JOINT_DTYPE), cs)
            assert e.value.code == -3                  # DMX_EINVAL
            w.synchronize()
            assert np.array_equal(w.download(B_.STATE).astype(np.float64), pre), "a refused tick changed the state"
            if before is not None:
                assert np.array_equal(w.contact_feedback(len(prime[0])), before), "a refused tick changed the last feedback"
            return Bp, pre, dict(w.lcp_stats(), tick=w.small_tick_stats()), None
        w.step_joints(W.h, jts.astype(B_.CONTACT_JOINT_DTYPE), cs)
        w.synchronize()
        post = w.download(B_.STATE)
        fb = w.contact_feedback() if feedback else None
        return Bp, post, dict(w.lcp_stats(), tick=w.small_tick_stats()), fb
    finally:
        w.close()


def tolerance(prec, stepper, r):
    """the issue's tolerances; float32 QuickStep asserts the margin gate"""
    if np.dtype(prec).itemsize == 8:
        return 1e-10 if stepper == "quick" else 1e-8
    t = 10 * EPS32 * max([I.kappa() for I in r.islands] + [1.0])
    if stepper == "exact":
        return 2 * t if any(I.pyramid.any() for I in r.islands) else t
    for I, lam, margin in zip(r.islands, r.lams, r.margins):
        if I.m:
            print(f"margin {margin:.3e} of max |lambda| {np.max(np.abs(lam)):.3e}")
            assert margin > 1e-3 * np.max(np.abs(lam)), "f32 QuickStep case too close to a clamp to compare"
    return t


def check(prec, B, W, jts, srf, stepper, small=B_.SMALL_TICK_OFF, feedback=False):
    """device against surface_dense; -> (reference Result, stats, device post-tick state as the device holds it)"""
    Bp, post_raw, stats, fb = run(prec, B, W, jts, srf, stepper, small, feedback)
    post = post_raw.astype(np.float64)
    Wr, jr, sr = as_precision(prec, W, jts, srf)
    r = sf.step(Bp, Wr, jr, sr, stepper)
    t = tolerance(prec, stepper, r)
    f32 = np.dtype(prec).itemsize == 4
    live = np.nonzero(Bp.flags & ld.ALIVE)[0]
    scale = ld.velocity_scale(r.bodies, Wr, live)
    err = ld.velocity_error(r.bodies, post[:, 7:10], post[:, 10:13], live)
    print(f"{prec} {stepper}: velocity error {err:.3e}, bound {t:.1e} x {scale:.3e}")
    assert err <= t * scale, f"velocity error {err:.3e} > {t:.1e} x {scale:.3e}"
    eps = 4 * (EPS32 if f32 else 2.2e-16)
    xerr = np.max(np.abs(post[live, 0:3] - r.bodies.pos[live]))
    assert xerr <= t * scale * Wr.h + eps * max(1.0, np.max(np.abs(r.bodies.pos[live]))), f"position error {xerr:.3e}"
    if feedback:
        want = fbd.feedback(Bp, r, jr).contacts
        fscale = max(np.max(np.abs(want)), 1e-30)
        ferr = np.max(np.abs(fb - want))
        print(f"feedback error {ferr:.3e} of {fscale:.3e}")
        assert ferr <= t * fscale, f"feedback error {ferr:.3e} > {t:.1e} x {fscale:.3e}"
    return r, stats, post_raw


world = gf.world
pressed = gf.pressed


# ---------------------------------------------------------------------------------------------------------------------
# one body (an extended tick's one-body islands take the lane's row form)
def one_body(nc, extra=0, seed=None):
    """one body on the ground with nc mixed contacts and `extra` frictionless ones behind them"""
    rng = np.random.default_rng(SEED_ONE_BODY[(nc, extra)] if seed is None else seed)
    B, jts = sd.chain(1, nc + extra, 0.5, rng, speed=0.05)
    B.lvel[0] = (0.4, -1.0, 0.3)
    jts, srf = mix(jts, range(nc))
    jts["mu"][nc:] = 0.0
    return B, jts, srf


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", ["quick", "exact"])
@pytest.mark.parametrize("nc", [1, 4, 5, 8])
def test_one_body(prec, stepper, nc):
    B, jts, srf = one_body(nc)
    check(prec, B, world(prec), jts, srf, stepper)


# two boxes, the upper on the lower, the lower on the ground, the ground contacts given as (body, world) or as (world, body)
def stack(order, seed=None):
    rng = np.random.default_rng(SEED_STACK if seed is None else seed)
    B, jts = sd.chain(2, 9, 0.5, rng, speed=0.05)
    B.lvel[:, 0] += (3.0, -3.0)
    pressed(B)
    jts, srf = mix(jts)
    if order == "world_first":                 # dJointAttach(c, 0, body): the sides exchanged, the normal reversed
        for j in jts:
            if j["body2"] < 0:
                j["body1"], j["body2"], j["normal"] = -1, j["body1"], -j["normal"]
    return B, jts, srf


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", ["quick", "exact"])
@pytest.mark.parametrize("order", ["body_first", "world_first"])
def test_two_box_stack(prec, stepper, order):
    B, jts, srf = stack(order)
    r, _, post = check(prec, B, world(prec), jts, srf, stepper)
    if order == "world_first":
        # no motion changes sign with the order of the sides: the same tick, bit for bit
        Bb, jb, sb = stack("body_first")
        assert np.array_equal(run(prec, Bb, world(prec), jb, sb, stepper)[1], post)


# ---------------------------------------------------------------------------------------------------------------------
# QuickStep islands at the kernels' thresholds: a kinematic slab at rest (slot 0) carrying one-body scenes side by side, as
# test_gpu_friction.hub_island -- every satellite's rows are those of its one-body scene, so the reference's clamp margin is that
# scene's however many there are, and the slab makes them one island
def hub_island(m):
    """one island of exactly m rows: m = 27 k + 3 a + b -- k satellites of nine contacts (the whole mix), and one of a mixed contacts
    with b frictionless ones behind them"""
    k, r = divmod(m, 27)
    a, b = divmod(r, 3)
    parts = [(9, 0)] * k + ([(a, b)] if r else [])
    pos, quat, lvel, avel, mass, inertia, js, ss = [[0.0, -0.5, 0.0]], [[1.0, 0, 0, 0]], [[0.0, 0, 0]], [[0.0, 0, 0]], [5.0], [[1.0, 1, 1]], [], []
    for s, (nc, extra) in enumerate(parts):
        B, j, srf = one_body(nc, extra)
        shift = np.array([3.0 * (s % 16), 0.0, 3.0 * (s // 16)])
        j["pos"] += shift
        j["body1"], j["body2"] = s + 1, 0
        pos.append(B.pos[0] + shift); quat.append(B.quat[0]); lvel.append(B.lvel[0]); avel.append(B.avel[0])
        mass.append(B.mass[0]); inertia.append(B.inertia[0]); js.append(j); ss.append(srf)
    flags = np.full(len(pos), ld.ALIVE, np.uint8)
    flags[0] |= ld.KINEMATIC
    return ld.Bodies(pos, quat, lvel, avel, mass, inertia, flags), np.concatenate(js), np.concatenate(ss)


@pytest.mark.parametrize("prec,m", [("float64", 255), ("float64", 256), ("float64", 257), ("float64", 258), ("float32", 255), ("float32", 256),
                                    ("float32", 257), ("float32", 258), ("float32", 3072), ("float32", 3073), ("float64", 1536), ("float64", 1537)])
def test_quickstep_island_thresholds(prec, m):
    """WAVE_ISLAND_ROWS (256 / 257) and its neighbours, REGS_ROWS<float> (3 072 / 3 073), REGS_ROWS<double> (1 536 / 1 537)"""
    B, jts, srf = hub_island(m)
    r, _, _ = check(prec, B, world(prec), jts, srf, "quick")
    assert len(r.islands) == 1 and r.islands[0].m == m


@pytest.mark.parametrize("prec,m", [("float32", 257), ("float32", 3073)])
def test_workgroup_forms_and_the_lane_form_agree_bit_for_bit(prec, m, tmp_path):
    """the same island by a workgroup and, in a child process with DMX_BIG_ISLAND_ROWS out of reach, by one lane (row_sor over the
    row table): one arithmetic, the same bits"""
    B, jts, srf = hub_island(m)
    _, wg, _, _ = run(prec, B, world(prec), jts, srf, "quick")
    out = str(tmp_path / "lane.npy")
    here = os.path.dirname(os.path.abspath(__file__))
    p = subprocess.run([sys.executable, os.path.abspath(__file__), prec, str(m), out], capture_output=True, text=True, timeout=600,
                       env={**os.environ, "DMX_BIG_ISLAND_ROWS": "1000000", "PYTHONPATH": os.pathsep.join([os.path.dirname(here), here])})
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-2500:]
    assert np.array_equal(np.load(out), wg)


# ---------------------------------------------------------------------------------------------------------------------
# dWorldStep: the one-workgroup LDS solve, its boundary, the grid solve
def exact_island(nc, seed):
    rng = np.random.default_rng(seed)
    B, jts = sd.chain(max(1, nc // 3), nc, 0.5, rng, speed=0.1)
    return (pressed(B),) + mix(jts)


def mix_rows(nc):
    """(m, nbd) of nc contacts with the mix: three rows each; mu = inf leaves two rows unbounded, mu = inf with a finite mu2 one"""
    nu = sum({6: 2, 7: 1}.get(k % len(MIX), 0) for k in range(nc))
    return 3 * nc, 3 * nc - nu


@pytest.mark.parametrize("prec", PRECS)
def test_exact_four_contacts(prec):
    B, jts, srf = exact_island(4, 3)
    r, st, _ = check(prec, B, world(prec), jts, srf, "exact")
    assert st["solves"] == 0


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("which", ["last", "over"])
def test_exact_lds_boundary(prec, which):
    """the last contact count whose island fits lcp_lds_fits and the first that does not (the grid solve: the counter moves)"""
    rb = np.dtype(prec).itemsize
    nc = 1
    while sd.lds_fits(rb, *mix_rows(nc)):
        nc += 1
    nc = nc - 1 if which == "last" else nc
    B, jts, srf = exact_island(nc, nc)
    r, st, _ = check(prec, B, world(prec), jts, srf, "exact")
    big = max(r.islands, key=lambda I: I.m)
    assert (big.m, big.nbd) == mix_rows(nc)
    assert (st["solves"] > 0) == (which == "over")
    if which == "over":
        assert (st["last_m"], st["last_nu"], st["last_nbd"]) == (big.m, big.nu, big.nbd)


@pytest.mark.parametrize("prec", PRECS)
def test_exact_grid_pressed_chain_of_70_contacts(prec):
    """70 contacts, 210 rows >= DMX_LCP_GRID_ROWS (192): the grid solve, two passes"""
    B, jts, srf = exact_island(70, 70)
    r, st, _ = check(prec, B, world(prec), jts, srf, "exact")
    assert st["solves"] == 1 and st["last_m"] == 210 and st["fallback"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# forms agree, feedback, auto-disable, no change without a bit, refusals
def stack_and_one():
    B, jts, srf = stack("body_first")
    B1, j1, s1 = one_body(4)
    B2 = ld.Bodies(np.vstack([B.pos, B1.pos + (5, 0, 0)]), np.vstack([B.quat, B1.quat]), np.vstack([B.lvel, B1.lvel]),
                   np.vstack([B.avel, B1.avel]), np.concatenate([B.mass, B1.mass]), np.vstack([B.inertia, B1.inertia]))
    j1["body1"] = 2
    j1["pos"][:, 0] += 5
    return B2, np.concatenate([jts, j1]), np.concatenate([srf, s1])


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", ["quick", "exact"])
def test_single_launch_tick_and_general_path_agree(prec, stepper):
    """QuickStep: the single-launch tick honours the extended surface, same bits as the general path.  dWorldStep: an extended tick
    takes the general path whole and counts under lds_fit; the same contacts without surfaces stay on the single-launch path"""
    B, jts, srf = stack_and_one()
    W = world(prec)
    _, off, st_off, _ = run(prec, B, W, jts, srf, stepper, small=B_.SMALL_TICK_OFF)
    _, on, st_on, _ = run(prec, B, W, jts, srf, stepper, small=B_.SMALL_TICK_AUTO)
    assert np.array_equal(off, on)
    assert st_off["tick"]["small"] == 0 and st_off["tick"]["mode"] == 1
    if stepper == "quick":
        assert st_on["tick"]["small"] == 1 and st_on["tick"]["general"] == 0
    else:
        assert st_on["tick"]["small"] == 0 and st_on["tick"]["general"] == 1 and st_on["tick"]["lds_fit"] == 1
        plain = jts.copy()
        plain["mode"] &= ~(sf.SURFACE_EXT | sf.APPROX1)
        _, _, st_plain, _ = run(prec, B, W, plain, srf, stepper, small=B_.SMALL_TICK_AUTO)
        assert st_plain["tick"]["small"] == 1


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", ["quick", "exact"])
@pytest.mark.parametrize("small", [B_.SMALL_TICK_OFF, B_.SMALL_TICK_AUTO])
def test_feedback_is_jt_lambda_and_changes_nothing(prec, stepper, small):
    B, jts, srf = stack("world_first")
    W = world(prec)
    _, _, with_fb = check(prec, B, W, jts, srf, stepper, small=small, feedback=True)
    _, without, _, _ = run(prec, B, W, jts, srf, stepper, small=small, feedback=False)
    assert np.array_equal(with_fb, without)


AD, DIS = B_.BODY_AUTODISABLE, B_.BODY_DISABLED


def four_stack_on_a_slip_surface():
    """four unit boxes at rest on top of each other, four contacts per face, every contact with SLIP1|SLIP2 (mu = 0.5): gravity
    presses, nothing slides, and the stack falls asleep when its counters run out"""
    nb = 4
    pos = np.column_stack([np.zeros(nb), 0.5 + np.arange(nb), np.zeros(nb)])
    B = ld.Bodies(pos, np.tile([1.0, 0, 0, 0], (nb, 1)), np.zeros((nb, 3)), np.zeros((nb, 3)), np.ones(nb), np.full((nb, 3), 1.0 / 6.0),
                  np.full(nb, ld.ALIVE | AD, np.uint8))
    out = []
    for k in range(nb):
        for dx, dz in ((-0.5, -0.5), (0.5, -0.5), (0.5, 0.5), (-0.5, 0.5)):
            out.append(((dx, float(k), dz), (0.0, 1.0, 0.0), 0.0, k, k - 1, sf.SLIP1 | sf.SLIP2, 0.5, 0, 0, 0, 0))
    jts = np.array(out, ld.JOINT_DTYPE)
    return B, jts, sf.surfaces(len(jts), slip1=0.01, slip2=0.02)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper,small", [("quick", B_.SMALL_TICK_OFF), ("quick", B_.SMALL_TICK_AUTO), ("exact", B_.SMALL_TICK_AUTO)])
def test_auto_disable_over_a_settled_stack_on_a_slip_surface(prec, stepper, small):
    """auto-disable on, extended ticks: the flags and the counters are those of the reference's rule (tests/autodisable_reference.py)
    applied to surface_dense's velocities, exactly; once asleep, the island is left out and the tick is no longer extended"""
    B, jts, srf = four_stack_on_a_slip_surface()
    W = world(prec)
    # (QuickStep's twenty sweeps leave the resting stack speeds of 0.02 to 0.05, growing from tick to tick: thresholds well above them)
    params = adr.Params(lin=0.2, ang=0.2, idle_steps=3)
    cnt = adr.Counters(B.n, params)
    w = B_.BatchWorld(B.n, prec, gravity=tuple(W.gravity))
    try:
        w.set_erp(W.erp); w.set_cfm(W.cfm); w.set_quickstep(W.iters, W.sor_w)
        w.set_stepper(B_.STEPPER_EXACT if stepper == "exact" else B_.STEPPER_QUICK)
        w.set_small_tick(small)
        w.set_auto_disable(params.lin, params.ang, params.idle_steps, params.idle_time)
        w.upload(B_.POS, B.pos); w.upload(B_.QUAT_RAW, B.quat); w.upload(B_.LVEL, B.lvel); w.upload(B_.AVEL, B.avel)
        w.upload(B_.MASS, B.mass); w.upload(B_.INERTIA, B.inertia)
        w.upload_body_flags(B.flags)
        flags = B.flags.copy()
        for t in range(5):
            pre = w.download(B_.STATE).astype(np.float64)
            Bp = ld.Bodies(pre[:, 0:3], pre[:, 3:7], pre[:, 7:10], pre[:, 10:13], B.mass, B.inertia, flags)
            w.step_joints(W.h, jts.astype(B_.CONTACT_JOINT_DTYPE), srf.astype(B_.CONTACT_SURFACE_DTYPE))
            w.synchronize()
            asleep = bool(flags[0] & DIS)
            if not asleep:
                Wr, jr, sr = as_precision(prec, W, jts, srf)
                r = sf.step(Bp, Wr, jr, sr, stepper)
                for s in range(B.n):
                    lv, av = r.bodies.lvel[s], r.bodies.avel[s]
                    # the comparison is honest only while no speed is near its threshold (autodisable_reference.margin_ok's rule)
                    assert np.sqrt(lv @ lv) < 0.9 * params.lin and np.sqrt(av @ av) < 0.9 * params.ang
                    _, _, f, cnt.steps[s], cnt.time[s] = adr.idle_rule(lv, av, int(flags[s]), cnt.steps[s], cnt.time[s], params, Wr.h)
                    flags[s] = f
            got = w.body_flags()
            assert np.array_equal(got, flags), (t, got, flags)
            st = w.auto_disable_stats()
            assert st["asleep"] == int(np.sum((flags & DIS) != 0)) and st["islands_skipped"] == (1 if asleep else 0), (t, st)
            steps, time = w.idle_counters()
            assert np.array_equal(steps, cnt.steps) and np.array_equal(time, cnt.time)
        assert np.all(flags & DIS)                    # it did fall asleep (tick 3), and two ticks were skipped
        post = w.download(B_.STATE).astype(np.float64)
        assert np.all(post[:, 7:13] == 0.0)
    finally:
        w.close()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", ["quick", "exact"])
@pytest.mark.parametrize("small", [B_.SMALL_TICK_OFF, B_.SMALL_TICK_AUTO])
def test_no_change_without_a_bit_and_without_surfaces(prec, stepper, small):
    """surfaces with no bit set: the bits and the path of dmxBatchStepJoints (nothing of the surfaces is read).  Bits set in the
    mode through plain dmxBatchStepJoints: the same bits as the same contacts without them"""
    B, jts, srf = stack_and_one()
    W = world(prec)
    plain = jts.copy()
    plain["mode"] &= ~sf.SURFACE_EXT
    _, a, st_a, _ = run(prec, B, W, plain, None, stepper, small=small)
    _, b, st_b, _ = run(prec, B, W, plain, srf, stepper, small=small)
    assert np.array_equal(a, b) and st_a == st_b
    _, c, st_c, _ = run(prec, B, W, jts, None, stepper, small=small)
    assert np.array_equal(a, c) and st_a == st_c
    # ... and a tick that does read them is another tick
    _, d, _, _ = run(prec, B, W, jts, srf, stepper, small=small)
    assert not np.array_equal(a, d)


BAD = [("mu2", np.nan, sf.MU2), ("fdir1", (np.nan, 0.0, 1.0), sf.FDIR1), ("fdir1", (0.0, INF, 1.0), sf.FDIR1), ("motion1", np.nan, sf.MOTION1),
       ("motion1", INF, sf.MOTION1), ("motion2", -INF, sf.MOTION2), ("motionN", np.nan, sf.MOTIONN), ("slip1", -1e-3, sf.SLIP1),
       ("slip1", np.nan, sf.SLIP1), ("slip2", INF, sf.SLIP2), ("slip2", -1.0, sf.SLIP2)]


@pytest.mark.parametrize("field,value,bit", BAD)
def test_a_bad_field_that_is_read_is_refused_and_one_that_is_not_read_is_not(field, value, bit):
    B, jts, srf = stack("body_first")
    W = world("float64")
    bad = srf.copy()
    bad[field][3] = value
    marked = jts.copy()
    marked["mode"][3] |= bit
    run("float64", B, W, marked, bad, "quick", expect_error=True, prime=(jts, srf))
    unread = jts.copy()
    unread["mode"][3] &= ~bit
    run("float64", B, W, unread, bad, "quick")


def test_in_a_float32_batch_a_field_is_judged_as_the_device_will_hold_it():
    """a finite double above float's largest is an infinity in a float32 batch: refused there, accepted in a float64 batch"""
    B, jts, srf = stack("body_first")
    for field, bit in (("slip1", sf.SLIP1), ("motion2", sf.MOTION2), ("fdir1", sf.FDIR1)):
        bad = srf.copy()
        bad[field][3] = 1e39
        marked = jts.copy()
        marked["mode"][3] |= bit
        run("float32", B, world("float32"), marked, bad, "quick", expect_error=True, prime=(jts, srf))
        if field == "slip1":                  # (a row as good as absent; the other two would only make absurd velocities)
            run("float64", B, world("float64"), marked, bad, "quick")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", ["quick", "exact"])
def test_a_stray_bit_above_odes_in_the_callers_mode_changes_nothing(prec, stepper):
    """bit 0x10000 of the staged mode is the host's own mark (mu_1 = 0 < mu_2); set in the caller's mode it must not reach the kernels"""
    B, jts, srf = stack("body_first")
    W = world(prec)
    stray = jts.copy()
    stray["mode"] |= 0x10000
    _, a, _, _ = run(prec, B, W, jts, srf, stepper)
    _, b, _, _ = run(prec, B, W, stray, srf, stepper)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("prec", PRECS)
def test_ode_row_order_is_refused_under_quickstep_only(prec):
    B, jts, srf = stack("body_first")
    jts["mode"] &= ~sf.APPROX1                  # (no pyramid row: the refusal is the extended tick's own)
    W = world(prec)
    run(prec, B, W, jts, srf, "quick", order=B_.ORDER_ODE, expect_error=True, prime=(jts, srf))
    _, a, _, _ = run(prec, B, W, jts, srf, "exact", order=B_.ORDER_ODE)
    _, b, _, _ = run(prec, B, W, jts, srf, "exact")
    assert np.array_equal(a, b)
    plain = jts.copy()
    plain["mode"] &= ~(sf.SURFACE_EXT | sf.APPROX1)
    run(prec, B, W, plain, srf, "quick", order=B_.ORDER_ODE)          # not an extended tick: accepted as before


# seeds chosen on the CPU, with the reference alone, so that float32 QuickStep's margin gate holds (tolerance() asserts it);
# by (mixed contacts, frictionless contacts behind them) of the one-body scene
SEED_ONE_BODY = {(1, 0): 1, (4, 0): 3, (5, 0): 26, (8, 0): 66, (9, 0): 71, (4, 1): 3, (4, 2): 5, (7, 0): 56, (7, 1): 56, (8, 1): 66}
SEED_STACK = 56


if __name__ == "__main__":          # the child of test_workgroup_forms_and_the_lane_form_agree_bit_for_bit
    _prec, _m, _out = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    _B, _jts, _srf = hub_island(_m)
    np.save(_out, run(_prec, _B, world(_prec), _jts, _srf, "quick")[1])
