"""Ball and hinge joints through dmxBatchSetJoints / dmxBatchStepJoints (both steppers, both precisions, the general path and the
single-launch tick) against the dense float64 reference with joint rows (tests/joint_dense.py).

As in test_gpu_solver_dense.py every case uploads a synthetic state, a set of articulation joints and a list of contact
joints, takes a tick (or a few) and compares each with the reference restarted from the device's own pre-tick state.  Cases
aim at the kernel choices an island makes once it holds joint rows: a one-body island that must not go to the one-body
kernels, islands without a single bounded row on the LDS solve and on the grid solve, mixed islands, the one-wavefront and
workgroup SOR forms on either side of 256 rows, and many small islands next to free bodies and contact-only singles.

Tolerances are that file's (velocities): float64 QuickStep 1e-10 and float64 dWorldStep 1e-8, relative to max(|v_ref|, g h);
float32 dWorldStep 10 eps32 kappa(A) with kappa from the reference -- a case whose float32 tolerance exceeded 1e-3 would not be a
test (asserted), and topologies are chosen for that: 8-link chains (kappa ~ 1e2) and stars round a heavy hub (kappa ~ 3); float32
QuickStep the per-body band of tests/quick_band.py with the joint rows' term, K = quick_band.K["joint"] measured on the CPU
(tests/test_quick_band.py), no gate and no admission rule -- and, so that no case is held to less than before, the old allowance
10 eps32 kappa(A) as a second ceiling wherever the old rule admits the tick (quick_band.assert_in_old_allowance; it is no gate:
a tick it does not admit is held to the band alone).  Every float32 QuickStep case is listed in F32_QUICK_CASES, which
tests/test_quick_band.py runs the float32 emulation over; CHAIN_CASES are the ones a dropped sweep cannot pass."""
import os
import subprocess
import sys

import numpy as np
import pytest

import joint_dense as jd
import lcp_dense as ld
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
DEVICE_WORST = {"joint": 0.0}            # the largest device deviation of this process, in eps32 M_v (printed by compare)


def world(**kw):
    return ld.World(cfm=1e-5, **kw)


def as_precision(prec, W, jts, art):
    """world parameters, contact and joint fields as the device holds them (rounded to float32 in a float32 batch)"""
    if np.dtype(prec).itemsize == 8:
        return W, jts, art
    r = lambda x: float(np.float32(x))
    W2 = ld.World(h=r(W.h), gravity=np.asarray(W.gravity, np.float32).astype(np.float64), erp=r(W.erp), cfm=r(W.cfm),
                  iters=W.iters, sor_w=r(W.sor_w), gyro=W.gyro)
    j2, a2 = jts.copy(), art.copy()
    for f in ("pos", "normal", "depth", "mu", "bounce", "bounce_vel", "soft_erp", "soft_cfm"):
        j2[f] = np.asarray(jts[f], np.float32).astype(np.float64)
    for f in ("anchor1", "anchor2", "axis1", "axis2"):
        a2[f] = np.asarray(art[f], np.float32).astype(np.float64)
    return W2, j2, a2


def to_c(art):
    out = np.zeros(len(art), B_.JOINT_DTYPE)
    for f in B_.JOINT_DTYPE.names:
        out[f] = art[f]
    return out


class Run:
    """a batch with a state and a joint set uploaded; tick() steps once and returns (pre-tick Bodies, post state (n, 13))"""

    def __init__(self, prec, B, W, art, stepper, small=None):
        self.prec, self.B, self.W, self.art, self.stepper = prec, B, W, art, stepper
        w = self.w = B_.BatchWorld(B.n, prec, gravity=tuple(W.gravity))
        w.set_erp(W.erp); w.set_cfm(W.cfm); w.set_quickstep(W.iters, W.sor_w); w.set_gyro_mode(W.gyro)
        w.set_stepper(B_.STEPPER_EXACT if stepper == "exact" else B_.STEPPER_QUICK)
        if small is not None:
            w.set_small_tick(small)
        w.upload(B_.POS, B.pos); w.upload(B_.QUAT_RAW, B.quat); w.upload(B_.LVEL, B.lvel); w.upload(B_.AVEL, B.avel)
        w.upload(B_.MASS, B.mass); w.upload(B_.INERTIA, B.inertia)
        w.upload_body_flags(B.flags)
        w.set_joints(to_c(art))
        self.mass = w.download(B_.MASS).astype(np.float64).reshape(-1)
        self.inertia = w.download(B_.INERTIA).astype(np.float64)

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
    Wr, jr, ar = as_precision(prec, run.W, jts, run.art)
    r = jd.step(Bp, Wr, jr, ar, stepper)
    f32 = np.dtype(prec).itemsize == 4
    live = np.nonzero(Bp.flags & ld.ALIVE)[0]
    dead = np.nonzero(~(Bp.flags & ld.ALIVE).astype(bool))[0]
    if len(dead):
        assert np.array_equal(post[dead], np.column_stack([Bp.pos, Bp.quat, Bp.lvel, Bp.avel])[dead]), "a dead slot changed"
    if f32 and stepper == "quick":
        qb.attach_joint_term(r, Bp, Wr, jr, ar)
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


NO_CONTACTS = np.zeros(0, ld.JOINT_DTYPE)


def check(prec, B, W, art, stepper, jts=NO_CONTACTS, ticks=1, small=None):
    """-> (the reference's Result per tick, lcp stats, small-tick stats, final state)"""
    run = Run(prec, B, W, art, stepper, small)
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
def one_body(kind, seed=3):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=4)
    B = ld.Bodies([[0.4, 1.0, -0.2]], [q / np.linalg.norm(q)], [[0.2, -0.1, 0.3]], [[0.5, 1.5, -0.7]], [1.3], [[0.4, 0.7, 0.9]])
    art = np.array([jd.from_world(B, kind, 0, -1, (0.0, 1.5, 0.0), (0.2, 1.0, 0.1))], jd.ART_DTYPE)
    return B, art


def two_bodies(first_is_world_side=False, kinematic=False, seed=5):
    rng = np.random.default_rng(seed)
    quat = rng.normal(size=(2, 4))
    quat /= np.linalg.norm(quat, axis=1)[:, None]
    B = ld.Bodies([[0.0, 2.0, 0.0], [1.0, 2.2, 0.1]], quat, rng.normal(scale=0.4, size=(2, 3)), rng.normal(scale=0.4, size=(2, 3)),
                  [1.0, 1.7], rng.uniform(0.3, 1.0, (2, 3)))
    if kinematic:
        B.flags[0] |= ld.KINEMATIC
        B.lvel[0], B.avel[0] = (0.5, 0.2, -0.3), (0.0, 1.0, 0.5)
    if first_is_world_side:
        art = np.array([jd.from_world(B, jd.BALL, -1, 1, (0.5, 2.1, 0.0))], jd.ART_DTYPE)
    else:
        art = np.array([jd.from_world(B, jd.BALL, 0, 1, (0.5, 2.1, 0.0))], jd.ART_DTYPE)
    art["anchor1"] += 0.01                       # start with an error, so that c is not zero
    return B, art


def chain_on_ground():
    """8 links from the world, bending from straight down to horizontal, the last two also pressed onto the ground by contacts
    with finite mu, infinite mu and mu = 0: an island that mixes joint rows with every kind of contact row (nbd > 0).  Bent,
    because a straight chain held at both ends has a redundant row along its axis (kappa(A) ~ 1 / cfm)"""
    B, art = jd.hanging_chain(8, bend=np.pi / 2)
    lift = 1.0 - B.pos[7][1]
    B.pos[:, 1] += lift                          # the last link's centre at y = 1
    art["anchor2"][0][1] += lift                 # (the world side of the first joint moves with it)
    B.lvel[6:] = (1.0, -1.0, 0.5)                # pressing down and sliding: normal rows loaded, bounded friction saturated
    jts = np.array([(B.pos[7] + (0.0, -0.5, 0.0), (0.0, 1.0, 0.0), 0.01, 7, -1, 0, 0.5, 0, 0, 0, 0),
                    (B.pos[6] + (0.0, -0.5, 0.1), (0.0, -1.0, 0.0), 0.02, -1, 6, 0, np.inf, 0, 0, 0, 0),
                    (B.pos[7] + (0.1, 0.0, 0.5), (0.0, 0.6, -0.8), 0.01, 7, -1, 0, 0.0, 0, 0, 0, 0)], ld.JOINT_DTYPE)
    return B, art, jts


def star_on_ground(n):
    """the star with 4 frictionless ground contacts under its hub, which moves down.  The normals lean, and not symmetrically:
    four parallel normals, or four that are one another's images under quarter turns about y, span three directions only
    and make kappa(A) ~ 1 / cfm"""
    B, art = jd.star(n)
    B.lvel[0] = (0.0, -1.0, 0.0)
    pts = [(2.0, -0.5, 0.0), (0.0, -0.5, 2.0), (-2.0, -0.5, 0.0), (0.0, -0.5, -2.0)]
    nrm = np.array([(0.5, 1.0, 0.0), (0.0, 1.0, 0.5), (0.0, 1.0, 0.5), (0.5, 1.0, 0.0)])
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    jts = np.array([(B.pos[0] + p, n, 0.01, 0, -1, 0, 0.0, 0, 0, 0, 0) for p, n in zip(pts, nrm)], ld.JOINT_DTYPE)
    return B, art, jts


def pendulum_pairs(npairs=40, nfree=5, nsingle=6, seed=11):
    """npairs two-body pendulums (world - ball - body - hinge - body), free bodies, and bodies resting on ground contacts alone"""
    rng = np.random.default_rng(seed)
    n = 2 * npairs + nfree + nsingle
    pos = np.column_stack([3.0 * np.arange(n), np.full(n, 3.0), np.zeros(n)])
    quat = rng.normal(size=(n, 4))
    quat /= np.linalg.norm(quat, axis=1)[:, None]
    B = ld.Bodies(pos, quat, rng.normal(scale=0.3, size=(n, 3)), rng.normal(scale=0.3, size=(n, 3)), rng.uniform(0.5, 2.0, n),
                  rng.uniform(0.3, 1.0, (n, 3)))
    art = []
    for p in range(npairs):
        a, b = 2 * p, 2 * p + 1
        B.pos[b] = B.pos[a] + (0.0, -1.0, 0.0)
        art.append(jd.from_world(B, jd.BALL, a, -1, B.pos[a] + (0.0, 0.5, 0.0)))
        art.append(jd.from_world(B, jd.HINGE, b, a, B.pos[a] + (0.0, -0.5, 0.0), (0.0, 0.0, 1.0)))
    first = 2 * npairs + nfree
    jts = []
    for s in range(first, n):
        B.lvel[s] = (0.1, -1.0, 0.0)
        # one contact with friction, then frictionless ones whose normals lean: no redundant rows
        for c in range(1 + (s - first) % 3):
            nrm = np.array([0.4 * c, 1.0, 0.3 * (c - 1) * c])
            jts.append((B.pos[s] + (0.3 * c, -0.5, 0.2 * c), nrm / np.linalg.norm(nrm), 0.01, s, -1, 0, 0.0 if c else np.inf, 0, 0, 0, 0))
    return B, np.array(art, jd.ART_DTYPE), np.array(jts, ld.JOINT_DTYPE)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("kind", [jd.BALL, jd.HINGE])
@pytest.mark.parametrize("small", [B_.SMALL_TICK_OFF, B_.SMALL_TICK_AUTO])
def test_one_body_on_a_joint_to_the_world(prec, stepper, kind, small):
    """a one-body island of 3 (ball) or 5 (hinge) rows: not the one-body kernels' island, which know contacts only -- on the
    general path (its own solve_singles / solve_singles_lds launches) and on the single-launch tick"""
    B, art = one_body(kind)
    (r,), _, st, _ = check(prec, B, world(), art, stepper, ticks=1, small=small)
    assert r.islands[0].m == (3 if kind == jd.BALL else 5)
    assert (st["small"], st["general"]) == ((1, 0) if small == B_.SMALL_TICK_AUTO else (0, 1))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("case", ["plain", "body1_is_world", "kinematic"])
def test_two_bodies_on_a_ball_joint(prec, stepper, case):
    """two bodies; body1 = -1 with a live body2 (the sides are exchanged); one side kinematic and moving"""
    B, art = two_bodies(first_is_world_side=case == "body1_is_world", kinematic=case == "kinematic")
    check(prec, B, world(), art, stepper, ticks=2)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
def test_chain_with_ground_contacts(prec, stepper):
    B, art, jts = chain_on_ground()
    (r,), _, _, _ = check(prec, B, world(), art, stepper, jts)
    I = r.islands[0]
    assert (I.m, I.n_art_rows) == (24 + 3 + 3 + 1, 24) and I.nbd == 3 + 1 + 1


@pytest.mark.parametrize("prec", PRECS)
def test_chain_without_contacts_has_no_bounded_row(prec):
    """the exact solve of an island whose rows can all never clamp: an empty Schur complement on the LDS solve"""
    B, art = jd.hanging_chain(8, horizontal=True)
    (r,), st, _, _ = check(prec, B, world(), art, "exact")
    assert (r.islands[0].m, r.islands[0].nbd) == (24, 0) and st["solves"] == 0


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("contacts", [False, True])
def test_star_of_100_takes_the_grid_solve(prec, contacts):
    """300 joint rows: past the LDS fit in both precisions (288 rows in f32, 192 in f64), with no bounded row at all, and with
    4 ground contacts on the hub"""
    if contacts:
        B, art, jts = star_on_ground(100)
    else:
        (B, art), jts = jd.star(100), NO_CONTACTS
    (r,), st, _, _ = check(prec, B, world(), art, "exact", jts)
    I = r.islands[0]
    assert I.n_art_rows == 300 and st["solves"] == 1
    assert (st["last_m"], st["last_nu"], st["last_nbd"]) == (I.m, I.nu, I.nbd)
    assert I.nbd == (4 if contacts else 0)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", [64, 90])
def test_quickstep_star_on_either_side_of_the_wave_form(prec, n):
    """192 and 270 rows: the one-wavefront SOR form and the workgroup forms (WAVE_ISLAND_ROWS = 256)"""
    B, art = jd.star(n)
    (r,), _, _, _ = check(prec, B, world(), art, "quick")
    assert r.islands[0].m == 3 * n


@pytest.mark.parametrize("prec", PRECS)
def test_quickstep_star_with_contacts(prec):
    """300 joint rows and 4 bounded ones: a mixed island above WAVE_ISLAND_ROWS on the workgroup SOR forms"""
    B, art, jts = star_on_ground(100)
    (r,), _, _, _ = check(prec, B, world(), art, "quick", jts)
    assert (r.islands[0].m, r.islands[0].nbd) == (304, 4)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
def test_many_small_islands(prec, stepper):
    """40 two-body pendulums next to free bodies and contact-only one-body islands in the same tick"""
    B, art, jts = pendulum_pairs()
    res, _, _, _ = check(prec, B, world(), art, stepper, jts)
    ms = sorted(I.m for I in res[0].islands)
    assert ms.count(8) == 40 and ms.count(0) == 5


# ---------------------------------------------------------------------------------------------------------------------
# Chains a wrong sweep cannot pass (joint_dense.ball_hinge_chain: rotated bodies, errors to correct, slow to converge), one island
# each, on the QuickStep row forms an island with joint rows takes -- units keep an island off the contact-as-unit forms
# (csrc/dmx_islands_dev.hpp, solve_island_wg_body): the lane-per-island form (a child process), the one-wavefront form up to
# WAVE_ISLAND_ROWS = 256 rows on the single-launch tick and on the general path, and just past it the 256-thread register form.
# tests/test_gpu_hinge_limot.py and tests/test_gpu_slider.py hold the forms further up.
CHAIN_CASES = ["ball_hinge_chain-40", "ball_hinge_chain-256", "ball_hinge_chain-260"]
FORM_CASES = {"lane per island": ["ball_hinge_chain-40"], "single-launch tick": ["ball_hinge_chain-256"],
              "one wavefront": ["ball_hinge_chain-256"], "registers, 256 threads": ["ball_hinge_chain-260"]}


@pytest.mark.parametrize("rows,small", [(256, B_.SMALL_TICK_AUTO), (256, B_.SMALL_TICK_OFF), (260, B_.SMALL_TICK_AUTO)])
def test_quickstep_chain_of_balls_and_hinges_f32(rows, small):
    """256 rows: the one-wavefront form, on the single-launch tick and on the general path; 260: the single-launch tick refuses
    the island (more rows than one wavefront holds) and the general path runs the 256-thread register form"""
    B, art = jd.ball_hinge_chain(rows)
    (r,), _, st, _ = check("float32", B, world(), art, "quick", small=small)
    assert [I.m for I in r.islands] == [rows] and r.islands[0].nbd == 0
    on_small = small == B_.SMALL_TICK_AUTO and rows <= 256
    assert (st["small"], st["general"]) == ((1, 0) if on_small else (0, 1)), st
    if small == B_.SMALL_TICK_AUTO and not on_small:
        assert st["sor_rows"] == 1, st


def child_lane_per_island_chain_f32():
    """(run by test_chain_on_the_lane_per_island_form_f32 under DMX_BIG_ISLAND_ROWS=64) a chain of 40 rows on 10 bodies with the
    single-launch tick off: the general path gives an island a workgroup only from that many rows on, so this one is swept by
    one lane (row_sor in solve_islands), as one-body islands on a joint always are"""
    threshold = int(os.environ["DMX_BIG_ISLAND_ROWS"])
    B, art = jd.ball_hinge_chain(40)
    (r,), _, st, _ = check("float32", B, world(), art, "quick", small=B_.SMALL_TICK_OFF)
    (I,) = r.islands
    assert I.m == 40 < threshold and len(I.slots) == 10
    assert (st["small"], st["general"]) == (0, 1), st


def test_chain_on_the_lane_per_island_form_f32():
    """DMX_BIG_ISLAND_ROWS is read once per process: a child"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_joints as t; t.child_lane_per_island_chain_f32(); "
            "print('CHILD-OK')") % (here, os.path.dirname(here))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600,
                       env={**os.environ, "DMX_BIG_ISLAND_ROWS": "64"})
    assert p.returncode == 0 and "CHILD-OK" in p.stdout, (p.stdout[-2000:] + p.stderr[-3000:])


# every float32 QuickStep case `compare` sees: name -> () -> (Bodies, World, contact joints, joints, limots (none here), ticks).
# tests/test_quick_band.py runs the float32 emulation of a float32 batch's rows and sweeps over them (quick_band.MEASURED["joint"])
def _case(B, art, jts=NO_CONTACTS, ticks=1):
    return B, world(), jts, art, None, ticks


F32_QUICK_CASES = {
    "one_body-ball": lambda: _case(*one_body(jd.BALL)), "one_body-hinge": lambda: _case(*one_body(jd.HINGE)),
    "two_bodies-plain": lambda: _case(*two_bodies(), ticks=2),
    "two_bodies-body1_is_world": lambda: _case(*two_bodies(first_is_world_side=True), ticks=2),
    "two_bodies-kinematic": lambda: _case(*two_bodies(kinematic=True), ticks=2),
    "chain_on_ground": lambda: _case(*chain_on_ground()),
    "star-64": lambda: _case(*jd.star(64)), "star-90": lambda: _case(*jd.star(90)),
    "star_on_ground-100": lambda: _case(*star_on_ground(100)),
    "pendulum_pairs": lambda: _case(*pendulum_pairs()),
}
for _rows in (40, 256, 260):
    F32_QUICK_CASES[f"ball_hinge_chain-{_rows}"] = lambda rows=_rows: _case(*jd.ball_hinge_chain(rows))


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("scene", ["chain", "pairs"])
def test_small_tick_and_general_path_agree_bit_for_bit(prec, stepper, scene):
    B, art, jts = chain_on_ground() if scene == "chain" else pendulum_pairs()
    out = {}
    for mode in (B_.SMALL_TICK_OFF, B_.SMALL_TICK_AUTO):
        run = Run(prec, B, world(), art, stepper, small=mode)
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
DRIFT_TICKS, DRIFT_H = 240, 1.0 / 120.0
# the float64 reference's own largest anchor separation over a reference-only run of the drift scene (measured on the CPU by
# reference_drift(); asserted below to 1 %, so the figure cannot go stale)
REFERENCE_DRIFT = 6.09e-3


def reference_drift():
    B, art = jd.hanging_chain(8, horizontal=True)
    W = world(h=DRIFT_H)
    worst = 0.0
    for _ in range(DRIFT_TICKS):
        B = jd.step(B, W, NO_CONTACTS, art, "exact").bodies
        worst = max(worst, float(np.max(jd.errors(B, art)[0])))
    return worst


@pytest.mark.parametrize("prec", PRECS)
def test_chain_released_horizontally_does_not_drift_apart(prec):
    """The 8-link chain released horizontally, 240 ticks at h = 1/120 with dWorldStep.  Every tick is compared with the
    reference within the per-tick tolerance, and the run's largest dmxBatchJointErrors position error stays within twice the
    float64 reference's own largest anchor separation over a reference-only run of the same scene: REFERENCE_DRIFT = 6.09e-3
    (the semi-implicit integration of a swinging chain separates the anchors by first order in h; ERP 0.2 pulls them back).  The
    product follows the reference tick by tick within rounding, so anything beyond that factor is a defect."""
    ref = reference_drift()
    assert abs(ref - REFERENCE_DRIFT) <= 0.01 * REFERENCE_DRIFT, f"the reference's drift is {ref:.4e}"
    B, art = jd.hanging_chain(8, horizontal=True)
    run = Run(prec, B, world(h=DRIFT_H), art, "exact")
    try:
        worst = 0.0
        for _ in range(DRIFT_TICKS):
            Bp, post = run.tick(NO_CONTACTS)
            compare(run, Bp, post, NO_CONTACTS)
            worst = max(worst, run.w.joint_errors()[2][0])
    finally:
        run.close()
    print(f"{prec}: largest joint position error {worst:.4e}, the reference's {ref:.4e}")
    assert worst <= 2 * ref


@pytest.mark.parametrize("prec", PRECS)
def test_joint_errors_against_numpy(prec):
    B, art, jts = pendulum_pairs(npairs=70)                    # 140 joints: more than one wavefront, fewer than a block
    extra = jd.arts(3, kind=jd.HINGE, anchor1=(0.3, 0.1, 0.0), axis1=(0, 1, 0), axis2=(1, 0, 0))
    extra["body1"], extra["body2"] = [-1, 2, 0], [-1, 2, 1]    # two inactive ones (they report 0) and a hinge badly off
    art = np.concatenate([art, extra])
    run = Run(prec, B, world(), art, "quick")
    try:
        for _ in range(3):
            run.tick(jts)
        pe, ae, mx = run.w.joint_errors()
        state = run.state()
    finally:
        run.close()
    _, _, ar = as_precision(prec, run.W, jts, art)
    rp, ra = jd.errors(run.bodies(state), ar)
    eps = EPS32 if prec == "float32" else 2.2e-16
    tol = 32 * eps * (np.max(np.abs(state[:, 0:3])) + max(np.max(np.abs(art["anchor1"])), np.max(np.abs(art["anchor2"]))))
    assert np.max(np.abs(pe - rp)) <= tol and np.max(np.abs(ae - ra)) <= 32 * eps
    assert mx == (np.max(pe), np.max(ae))
    assert pe[-3] == 0 and pe[-2] == 0 and ae[-3] == 0 and ae[-1] > 0 and np.all(ae[:-3][art["kind"][:-3] == jd.BALL] == 0)


def test_ticks_that_do_not_know_joints_say_so():
    B, art = two_bodies()
    run = Run("float32", B, world(), art, "quick")
    w = run.w
    try:
        assert w.joint_count() == 1
        for call in (lambda: w.step(H, 1), lambda: w.exact_tick(H), lambda: w.step_timed(H, 1), lambda: w.chunk_tick(H)):
            with pytest.raises(B_.DmxError) as e:
                call()
            assert e.value.code == EINVAL
        w.set_row_order(B_.ORDER_ODE)
        with pytest.raises(B_.DmxError) as e:
            w.step_joints(H, NO_CONTACTS)
        assert e.value.code == EINVAL
        w.set_stepper(B_.STEPPER_EXACT)                        # dWorldStep never uses the order: nothing to refuse
        w.step_joints(H, NO_CONTACTS)
        w.synchronize()
        assert w.last_contact_count() == 0                      # (joints are not contacts)
        w.set_stepper(B_.STEPPER_QUICK)
        w.set_joints(None)                                      # dmxBatchSetJoints(b, 0, NULL): everything works again
        assert w.joint_count() == 0
        w.step_joints(H, NO_CONTACTS)
        w.set_row_order(B_.ORDER_CREATION)
        w.step(H, 1)
        w.exact_tick(H)
        w.synchronize()
        with pytest.raises(B_.DmxError):
            w.set_joints(jd.arts(1, kind=7))                    # not a kind the library knows
    finally:
        run.close()


def test_joint_from_world_matches_the_reference():
    B, _ = two_bodies()
    run = Run("float64", B, world(), jd.arts(0), "quick")
    try:
        got = run.w.joint_from_world(B_.JOINT_HINGE, 0, 1, (0.5, 2.1, 0.0), (0.0, 2.0, 0.0))
        to_world_side = run.w.joint_from_world(B_.JOINT_BALL, -1, 1, (0.5, 2.1, 0.0))
    finally:
        run.close()
    ref = jd.from_world(B, jd.HINGE, 0, 1, (0.5, 2.1, 0.0), (0.0, 1.0, 0.0))
    for f in ("anchor1", "anchor2", "axis1", "axis2"):
        assert np.max(np.abs(got[f] - ref[f])) <= 1e-14, f
    assert (got["kind"], got["body1"], got["body2"]) == (jd.HINGE, 0, 1)
    assert np.array_equal(to_world_side["anchor1"], (0.5, 2.1, 0.0)) and to_world_side["body1"] == -1
