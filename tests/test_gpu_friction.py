"""Friction that scales with the normal force (DMX_CONTACT_APPROX1) on the device, against the dense float64 reference
(tests/friction_dense.py): dmxBatchStepJoints, both steppers, both precisions, from the device's own downloaded pre-tick state.

Tolerances and gates are those of tests/test_gpu_solver_dense.py (velocities relative to max(|v_ref|, g h)):
  * float64 QuickStep 1e-10, float64 dWorldStep 1e-8;
  * float32 QuickStep 10 eps32 kappa(A), compared only where the reference's clamp margin -- the distance to the MOVING bound
    included -- is above 1e-3 of the island's largest |lambda| (asserted);
  * float32 dWorldStep 2 x 10 eps32 kappa(A): two solves, and pass B's bounds carry pass A's error (the solution of a box LCP is
    Lipschitz in its bounds).
Every comparison case carries the same mix of contacts: pyramid (both bits, mu = 0.5), box (mu = 0.5 without a bit), direction 1
only, direction 2 only, and mu = inf with both bits.  Scene builders are test_gpu_solver_dense's."""
import os
import subprocess
import sys

import numpy as np
import pytest

import feedback_dense as fbd
import friction_dense as fd
import lcp_dense as ld
import test_gpu_solver_dense as sd
from __graft_entry__ import load_package

pkg = load_package()
B_ = pkg.batch
pytestmark = pytest.mark.gpu

H = sd.H
EPS32 = sd.EPS32
MIX = [(fd.APPROX1, 0.5), (0, 0.5), (fd.APPROX1_1, 0.5), (fd.APPROX1_2, 0.5), (fd.APPROX1, np.inf)]
PRECS = ["float64", "float32"]


def mix(jts, idx=None, start=0):
    """give the contacts `idx` (default: all) the five kinds of MIX in turn"""
    jts = jts.copy()
    for k, i in enumerate(range(len(jts)) if idx is None else idx):
        mode, mu = MIX[(k + start) % len(MIX)]
        jts["mode"][i] = int(jts["mode"][i]) | mode
        jts["mu"][i] = mu
    return jts


def run(prec, B, W, jts, stepper, small=B_.SMALL_TICK_OFF, feedback=False, order=None, expect_error=False):
    """one dmxBatchStepJoints tick -> (pre-tick Bodies as the device held them, post-tick state (n, 13), stats, contact feedback or
    None).  expect_error: the call must fail with DMX_EINVAL and leave the state untouched (-> the same tuple, post = the state)"""
    w = B_.BatchWorld(B.n, prec, gravity=tuple(W.gravity))
    try:
        w.set_erp(W.erp); w.set_cfm(W.cfm); w.set_quickstep(W.iters, W.sor_w); w.set_gyro_mode(W.gyro)
        w.set_stepper(B_.STEPPER_EXACT if stepper == "exact" else B_.STEPPER_QUICK)
        w.set_small_tick(small)
        if order is not None:
            w.set_row_order(order, 7)
        w.set_feedback(feedback)
        w.upload(B_.POS, B.pos); w.upload(B_.QUAT_RAW, B.quat); w.upload(B_.LVEL, B.lvel); w.upload(B_.AVEL, B.avel)
        w.upload(B_.MASS, B.mass); w.upload(B_.INERTIA, B.inertia)
        w.upload_body_flags(B.flags)
        mass = w.download(B_.MASS).astype(np.float64).reshape(-1)
        inertia = w.download(B_.INERTIA).astype(np.float64)
        pre = w.download(B_.STATE).astype(np.float64)
        Bp = ld.Bodies(pre[:, 0:3], pre[:, 3:7], pre[:, 7:10], pre[:, 10:13], mass, inertia, B.flags)
        if expect_error:
            with pytest.raises(B_.DmxError) as e:
                w.step_joints(W.h, jts.astype(B_.CONTACT_JOINT_DTYPE))
            assert e.value.code == -3                  # DMX_EINVAL
            w.synchronize()
            assert np.array_equal(w.download(B_.STATE).astype(np.float64), pre), "a refused tick changed the state"
            return Bp, pre, dict(w.lcp_stats(), tick=w.small_tick_stats()), None
        w.step_joints(W.h, jts.astype(B_.CONTACT_JOINT_DTYPE))
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
        return 2 * t
    for I, lam, margin in zip(r.islands, r.lams, r.margins):
        if I.m:
            print(f"margin {margin:.3e} of max |lambda| {np.max(np.abs(lam)):.3e}")
            assert margin > 1e-3 * np.max(np.abs(lam)), "f32 QuickStep case too close to a clamp to compare"
    return t


def check(prec, B, W, jts, stepper, small=B_.SMALL_TICK_OFF, feedback=False, pyramid=True):
    """device against friction_dense; -> (reference Result, stats, device post-tick state as the device holds it)"""
    Bp, post_raw, stats, fb = run(prec, B, W, jts, stepper, small, feedback)
    post = post_raw.astype(np.float64)
    Wr, jr = sd.as_precision(prec, W, jts)
    r = fd.step(Bp, Wr, jr, stepper)
    assert any(I.pyramid.any() for I in r.islands) == pyramid
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


def world(prec, **kw):
    return sd.world(prec, **kw)


def pressed(B):
    """every body of a chain pressing into the one below: normal rows stay loaded"""
    B.lvel[:, 1] -= 1.0 + 0.1 * np.arange(B.n)
    return B


# ---------------------------------------------------------------------------------------------------------------------
# QuickStep: one body (the lane's row form takes the one-body forms' islands in such a tick)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("nc", [1, 4, 5, 8])
def test_quickstep_one_body(prec, nc):
    rng = np.random.default_rng(SEED_ONE_BODY[nc])
    B, jts = sd.chain(1, nc, 0.5, rng, speed=0.05)
    B.lvel[0] = (0.4, -1.0, 0.3)
    check(prec, B, world(prec), mix(jts), "quick")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("nc", [1, 4, 8])
def test_exact_one_body(prec, nc):
    rng = np.random.default_rng(SEED_ONE_BODY[nc])
    B, jts = sd.chain(1, nc, 0.5, rng, speed=0.05)
    B.lvel[0] = (0.4, -1.0, 0.3)
    check(prec, B, world(prec), mix(jts), "exact")


# two boxes, the upper on the lower, the lower on the ground: (body, body), (-1, body) and a kinematic lower box
def stack(order, kinematic, seed):
    rng = np.random.default_rng(seed)
    B, jts = sd.chain(2, 8, 0.5, rng, speed=0.05)
    B.lvel[:, 0] += (3.0, -3.0)           # the boxes slide against each other and the ground: most friction rows decisively at a bound
    pressed(B)
    jts = mix(jts)
    if order == "world_first":                 # dJointAttach(c, 0, body): the sides exchanged, the normal reversed
        for j in jts:
            if j["body2"] < 0:
                j["body1"], j["body2"], j["normal"] = -1, j["body1"], -j["normal"]
    if kinematic:                              # (contacts of the kinematic box with the ground would be rows between two immovable sides)
        B.flags[0] |= ld.KINEMATIC
        jts = jts[jts["body2"] >= 0]
    return B, jts


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", ["quick", "exact"])
@pytest.mark.parametrize("order,kinematic", [("body_first", False), ("world_first", False), ("body_first", True)])
def test_two_box_stack(prec, stepper, order, kinematic):
    B, jts = stack(order, kinematic, SEED_STACK[kinematic])
    check(prec, B, world(prec), jts, stepper)


# ---------------------------------------------------------------------------------------------------------------------
# QuickStep islands at the kernels' thresholds.  press_chain keeps every normal row loaded; its first five contacts carry the mix
# (the rest stay frictionless: m != 3 nc, the row-unit forms), so that float32 stays clear of a clamp
def threshold_island(m, all_three=False, seed=None):
    """an island of exactly m rows: five mixed three-row contacts and m - 15 one-row ones; all_three: every other contact has
    three rows too (mu = inf with the bits: never clamps), m must be a multiple of 3"""
    if all_three:
        assert m % 3 == 0
        B, jts = sd.press_chain(m // 3, np.random.default_rng(m if seed is None else seed))
        jts["mu"] = np.inf
        jts["mode"] = fd.APPROX1
    else:
        B, jts = sd.press_chain(m - 10, np.random.default_rng(m))
    return B, mix(jts, range(5))


def hub_island(m):
    """one island of exactly m rows that float32 can be held to: a kinematic slab at rest (slot 0) carrying one-body scenes of
    test_quickstep_one_body -- sd.chain(1, nc, ...) with the mix, their ground contacts re-attached to the slab -- side by side.  The
    slab's inverse mass is zero, so every satellite's rows are those of its one-body scene and the reference's clamp margin is that
    scene's, however many there are; the slab makes them one island, every row on a level of its own.  m = 15 k + r: k satellites of
    five contacts (the whole mix, three rows each), and for r = 3, 12, 13 one of one contact, of four, of four and a frictionless one"""
    k, r = divmod(m, 15)
    assert r in (0, 3, 12, 13)
    parts = [5] * k + {0: [], 3: [1], 12: [4], 13: [4, 0]}[r]
    pos, quat, lvel, avel, mass, inertia, js = [[0.0, -0.5, 0.0]], [[1.0, 0, 0, 0]], [[0.0, 0, 0]], [[0.0, 0, 0]], [5.0], [[1.0, 1, 1]], []
    for s, nc in enumerate(parts):
        B, j = sd.chain(1, max(nc, 1), 0.5, np.random.default_rng(SEED_ONE_BODY[max(nc, 1)]), speed=0.05)
        B.lvel[0] = (0.4, -1.0, 0.3)
        j = mix(j) if nc else j
        if not nc:
            j["mu"] = 0.0
        shift = np.array([3.0 * (s % 16), 0.0, 3.0 * (s // 16)])
        j["pos"] += shift
        j["body1"], j["body2"] = s + 1, 0
        pos.append(B.pos[0] + shift); quat.append(B.quat[0]); lvel.append(B.lvel[0]); avel.append(B.avel[0])
        mass.append(B.mass[0]); inertia.append(B.inertia[0]); js.append(j)
    flags = np.full(len(pos), ld.ALIVE, np.uint8)
    flags[0] |= ld.KINEMATIC
    return ld.Bodies(pos, quat, lvel, avel, mass, inertia, flags), np.concatenate(js)


@pytest.mark.parametrize("m", [255, 258, 3072, 3073])
def test_quickstep_f32_at_the_thresholds_on_a_hub(m):
    """float32 against the reference, the margin gate asserted, where press_chain's reference fails it: every contact on three rows
    at 255 / 258 rows (the shape the contact-unit forms take in a tick without pyramid rows) and REGS_ROWS<float> at 3 072 / 3 073"""
    B, jts = hub_island(m)
    r, _, _ = check("float32", B, world("float32"), jts, "quick")
    assert len(r.islands) == 1 and r.islands[0].m == m
    if m in (255, 258):
        assert m == 3 * len(jts)


@pytest.mark.parametrize("prec,m", [("float64", 256), ("float64", 257), ("float32", 256), ("float32", 257),
                                    ("float64", 1536), ("float64", 1537), ("float32", 1025), ("float64", 3072), ("float64", 3073)])
def test_quickstep_island_thresholds(prec, m):
    """WAVE_ISLAND_ROWS (256 / 257), REGS_ROWS<double> (1 536 / 1 537) and the 512-thread register form (float32, above 1 024 rows):
    the wavefront's and the workgroup's row-unit forms with the normal rows' multipliers in LDS, and past the register form the
    sweep over the row table.  REGS_ROWS<float> (3 072 / 3 073) is compared in float64 here -- the reference's margin on these
    islands is 4e-4 and 1e-4 of the largest |lambda|, under the gate, wherever the five mixed contacts sit -- and in float32 on the
    hub island above and bit for bit against the lane form below"""
    B, jts = threshold_island(m)
    r, _, _ = check(prec, B, world(prec), jts, "quick")
    assert r.islands[0].m == m


@pytest.mark.parametrize("m", [255, 258])
def test_quickstep_all_three_rows(m):
    """every contact on three rows around WAVE_ISLAND_ROWS: the shape the contact-unit forms take in a tick without pyramid rows.
    float64 on the pressed chain, whose reference fails float32's margin gate (a normal row of the all-friction chain always ends
    within 3e-5 of zero); float32 at the same row counts: test_quickstep_f32_at_the_thresholds_on_a_hub"""
    B, jts = threshold_island(m, all_three=True)
    r, _, _ = check("float64", B, world("float64"), jts, "quick")
    assert r.islands[0].m == m == 3 * len(jts)


@pytest.mark.parametrize("prec,m", [("float32", 257), ("float32", 3072), ("float32", 3073), ("float64", 1536), ("float64", 1537)])
def test_workgroup_forms_and_the_lane_form_agree_bit_for_bit(prec, m, tmp_path):
    """the same island by a workgroup (the register forms with the multipliers in LDS; past REGS_ROWS the sweep over the row table)
    and, in a child process with DMX_BIG_ISLAND_ROWS out of reach, by one lane (row_sor over the row table, the form
    tests/test_friction_harness.py holds to the reference on the host): one arithmetic, the same bits"""
    B, jts = threshold_island(m)
    _, wg, _, _ = run(prec, B, world(prec), jts, "quick")
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
    return pressed(B), mix(jts)


def mix_mus(nc):
    return np.array([MIX[k % len(MIX)][1] for k in range(nc)])


@pytest.mark.parametrize("prec", PRECS)
def test_exact_four_contacts(prec):
    B, jts = exact_island(4, 3)
    r, st, _ = check(prec, B, world(prec), jts, "exact")
    assert st["solves"] == 0


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("which", ["last", "over"])
def test_exact_lds_boundary(prec, which):
    """the last contact count whose island fits lcp_lds_fits and the first that does not (the grid solve: the counter moves)"""
    rb = np.dtype(prec).itemsize
    nc = 1
    while sd.lds_fits(rb, *sd.rows_of(mix_mus(nc))[::2]):
        nc += 1
    nc = nc - 1 if which == "last" else nc
    B, jts = exact_island(nc, nc)
    r, st, _ = check(prec, B, world(prec), jts, "exact")
    big = max(r.islands, key=lambda I: I.m)
    assert (st["solves"] > 0) == (which == "over")
    if which == "over":
        assert (st["last_m"], st["last_nu"], st["last_nbd"]) == (big.m, big.nu, big.nbd)


@pytest.mark.parametrize("prec", PRECS)
def test_exact_grid_pressed_chain_of_70_contacts(prec):
    """70 contacts, 210 rows >= DMX_LCP_GRID_ROWS (192): the grid solve, two passes"""
    B, jts = exact_island(70, 70)
    r, st, _ = check(prec, B, world(prec), jts, "exact")
    assert st["solves"] == 1 and st["last_m"] == 210 and st["fallback"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# the slope: a known answer through the device
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", ["quick", "exact"])
@pytest.mark.parametrize("mass", [1.0, 100.0])
def test_slope_through_the_device(prec, stepper, mass):
    g = 9.8
    f32 = np.dtype(prec).itemsize == 4
    for tan_theta, slides in ((0.3, False), (0.8, True)):
        theta = np.arctan(tan_theta)
        B, W, jts = fd.slope_scene(mass, theta, 0.5, fd.APPROX1, g=g, h=H)
        W.cfm = 0.0
        W.iters, W.sor_w = 20, 1.0
        _, post, _, _ = run(prec, B, W, jts, stepper)
        v = post.astype(np.float64)[0, 7:10]
        want = H * g * (np.sin(theta) - 0.5 * np.cos(theta)) if slides else 0.0
        # one body, three decoupled rows: the tick is exact up to rounding in both steppers
        tol = (100 * EPS32 if f32 else 1e-9) * g * H
        assert abs(v[0] - want) <= tol and abs(v[2]) <= tol, (v, want)
    # without the bit the cap is mu newtons: the two masses slide differently
    B, W, jts = fd.slope_scene(mass, np.arctan(0.8), 0.5, 0, g=g, h=H)
    W.cfm = 0.0
    _, post, _, _ = run(prec, B, W, jts, stepper)
    want = H * (g * np.sin(np.arctan(0.8)) - 0.5 / mass)
    assert abs(post.astype(np.float64)[0, 7] - want) <= (100 * EPS32 if f32 else 1e-9) * g * H


# ---------------------------------------------------------------------------------------------------------------------
# forms agree, feedback, no change without the bit, refusals
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", ["quick", "exact"])
def test_single_launch_tick_and_general_path_agree(prec, stepper):
    """QuickStep: the single-launch tick honours pyramid rows, same bits as the general path.  dWorldStep: a tick with a pyramid
    row takes the general path whole and counts under lds_fit; without one it stays on the single-launch path"""
    B, jts = stack("body_first", False, SEED_STACK[False])
    one = sd.chain(1, 3, 0.5, np.random.default_rng(2), speed=0.05)
    B2 = ld.Bodies(np.vstack([B.pos, one[0].pos + (5, 0, 0)]), np.vstack([B.quat, one[0].quat]), np.vstack([B.lvel, [[0.3, -1.0, 0.2]]]),
                   np.vstack([B.avel, one[0].avel]), np.concatenate([B.mass, one[0].mass]), np.vstack([B.inertia, one[0].inertia]))
    j1 = mix(one[1])
    j1["body1"] = 2
    j1["pos"][:, 0] += 5
    jj = np.concatenate([jts, j1])
    W = world(prec)
    _, off, st_off, _ = run(prec, B2, W, jj, stepper, small=B_.SMALL_TICK_OFF)
    _, on, st_on, _ = run(prec, B2, W, jj, stepper, small=B_.SMALL_TICK_AUTO)
    assert np.array_equal(off, on)
    assert st_off["tick"]["small"] == 0 and st_off["tick"]["mode"] == 1
    if stepper == "quick":
        assert st_on["tick"]["small"] == 1 and st_on["tick"]["general"] == 0
    else:
        assert st_on["tick"]["small"] == 0 and st_on["tick"]["general"] == 1 and st_on["tick"]["lds_fit"] == 1
        plain = jj.copy()
        plain["mode"] &= ~fd.APPROX1
        _, _, st_plain, _ = run(prec, B2, W, plain, stepper, small=B_.SMALL_TICK_AUTO)
        assert st_plain["tick"]["small"] == 1


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", ["quick", "exact"])
@pytest.mark.parametrize("small", [B_.SMALL_TICK_OFF, B_.SMALL_TICK_AUTO])
def test_feedback_is_jt_lambda_and_changes_nothing(prec, stepper, small):
    B, jts = stack("world_first", False, SEED_STACK[False])
    W = world(prec)
    _, _, with_fb = check(prec, B, W, jts, stepper, small=small, feedback=True)
    _, without, _, _ = run(prec, B, W, jts, stepper, small=small, feedback=False)
    assert np.array_equal(with_fb, without)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", ["quick", "exact"])
def test_no_change_without_a_pyramid_row(prec, stepper):
    """bit 0x4000 (ODE's rolling friction) and the bits together with mu = inf or mu = 0 make no pyramid row: the same bits as
    without them, and as lcp_dense"""
    rng = np.random.default_rng(12)
    B, jts = sd.chain(3, 9, rng.choice([0.0, 0.5, np.inf], 9), rng, speed=0.3)
    pressed(B)
    marked = jts.copy()
    marked["mode"] |= fd.APPROX1_N
    marked["mode"] = np.where(marked["mu"] == 0.5, marked["mode"], marked["mode"] | fd.APPROX1)
    W = world(prec)
    _, a, _, _ = run(prec, B, W, jts, stepper)
    _, b, _, _ = run(prec, B, W, marked, stepper)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("prec", PRECS)
def test_ode_row_order_is_refused_under_quickstep_only(prec):
    B, jts = stack("body_first", False, SEED_STACK[False])
    W = world(prec)
    run(prec, B, W, jts, "quick", order=B_.ORDER_ODE, expect_error=True)
    _, a, _, _ = run(prec, B, W, jts, "exact", order=B_.ORDER_ODE)
    _, b, _, _ = run(prec, B, W, jts, "exact")
    assert np.array_equal(a, b)
    plain = jts.copy()
    plain["mode"] &= ~fd.APPROX1
    run(prec, B, W, plain, "quick", order=B_.ORDER_ODE)          # no pyramid row: accepted as before


def test_a_refused_tick_leaves_the_last_feedback_served():
    B, jts = stack("body_first", False, SEED_STACK[False])
    W = world("float64")
    w = B_.BatchWorld(B.n, "float64", gravity=tuple(W.gravity))
    try:
        w.set_cfm(W.cfm)
        w.set_feedback(True)
        w.upload(B_.POS, B.pos); w.upload(B_.QUAT_RAW, B.quat); w.upload(B_.LVEL, B.lvel); w.upload(B_.AVEL, B.avel)
        w.upload(B_.MASS, B.mass); w.upload(B_.INERTIA, B.inertia)
        w.step_joints(W.h, jts.astype(B_.CONTACT_JOINT_DTYPE))
        before = w.contact_feedback()
        assert np.any(before != 0)
        w.set_row_order(B_.ORDER_ODE, 7)
        with pytest.raises(B_.DmxError):
            w.step_joints(W.h, jts.astype(B_.CONTACT_JOINT_DTYPE))
        assert np.array_equal(w.contact_feedback(len(jts)), before)
    finally:
        w.close()


@pytest.mark.parametrize("prec", PRECS)
def test_device_collided_tick_refuses_a_pyramid_surface(prec):
    scene = pkg.scenes.box_grid(4, 4, seed=1, y_range=(0.6, 1.5), spin=True, box_mass=True).astype(prec)
    w = B_.BatchWorld(scene.n, dtype=prec)
    try:
        w.load_scene(scene)
        w.set_surface(B_.CONTACT_BOUNCE | B_.CONTACT_APPROX1, 0.5)
        before = w.download(B_.STATE)
        for call in (lambda: w.step(H, 1), lambda: w.step_timed(H, 1), lambda: w.exact_tick(H), lambda: w.step_range(H, 0, scene.n)):
            with pytest.raises(B_.DmxError):
                call()
        w.synchronize()
        assert np.array_equal(w.download(B_.STATE), before)
        w.set_surface(B_.CONTACT_BOUNCE | B_.CONTACT_APPROX1, float("inf"))      # unbounded whatever the bits say
        w.step(H, 2)
        w.synchronize()
        marked = w.download(B_.STATE)
    finally:
        w.close()
    w = B_.BatchWorld(scene.n, dtype=prec)
    try:
        w.load_scene(scene)
        w.set_surface(B_.CONTACT_BOUNCE, float("inf"))
        w.step(H, 2)
        w.synchronize()
        assert np.array_equal(w.download(B_.STATE), marked)
    finally:
        w.close()


# seeds chosen on the CPU, with the reference alone, so that float32 QuickStep's margin gate holds (tolerance() asserts it)
SEED_ONE_BODY = {1: 1, 4: 1, 5: 5, 8: 5}
SEED_STACK = {False: 53, True: 1}          # by `kinematic`


if __name__ == "__main__":          # the child of test_workgroup_forms_and_the_lane_form_agree_bit_for_bit
    _prec, _m, _out = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    _B, _jts = threshold_island(_m)
    np.save(_out, run(_prec, _B, world(_prec), _jts, "quick")[1])
