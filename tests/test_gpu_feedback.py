"""Feedback -- the force and torque every joint and contact joint applied in a tick -- through dmxBatchSetFeedback /
dmxBatchJointFeedback / dmxBatchContactFeedback / dmxBatchFeedbackDevice (both steppers, both precisions, the general path and the
single-launch tick), against tests/feedback_dense.py on top of the dense float64 reference (tests/slider_dense.py).

Run, the scenes and their seeds are test_gpu_hinge_limot.py's and test_gpu_slider.py's, imported: those seeds already meet that
file's conditioning, stop-margin and clamp-margin rules.  Every case asserts, per tick,
  (a) the feedback agrees with the reference restarted from the device's own pre-tick state;
  (b) every two-body joint and contact applies zero net wrench (on the device's numbers);
  (c) the bodies' post-tick state is bit-identical with feedback on and off;
  (d) dmxBatchFeedbackDevice's arrays hold what the host getters return;
and which path ran, from the existing counters.

The tolerance of (a) follows from the project's velocity rule: a velocity error dv is a force error m dv / h, so
|fb - fb_ref| <= t F + 4 eps (largest component), with t exactly test_gpu_hinge_limot.compare's (float64 QuickStep 1e-10, float64
dWorldStep 1e-8, float32 10 eps32 kappa(A), asserted <= 1e-3) and, per island, F = max(the reference's force components,
m_max velocity_scale / h) for forces and max(the reference's torque components, I_max velocity_scale / h) for torques.

(b): f1 + f2 = 0 holds exactly (the two linear blocks of a row are each other's negatives and are summed in the same order).  The
torques: contacts, lock, hinge and slider rows act about one point, so their net torque is rounding only -- at most 6 rows x 2 sides,
each arm and product a few roundings: 64 eps of the largest term; a ball unit's arms go to the two anchors, which are apart by the
joint's error p_2 - p_1, so a ball, hinge or fixed joint leaves (p_1 - p_2) x f, bounded by pos_err |f| with the reference's pos_err."""
import ctypes as C

import numpy as np
import pytest

import feedback_dense as fd
import joint_dense as jd
import lcp_dense as ld
import slider_dense as sd
import test_gpu_hinge_limot as hl
import test_gpu_slider as sl
from __graft_entry__ import load_package

pkg = load_package()
B_ = pkg.batch
pytestmark = pytest.mark.gpu

EPS32 = hl.EPS32
PRECS, STEPPERS = hl.PRECS, hl.STEPPERS
EINVAL = hl.EINVAL
NO_CONTACTS = hl.NO_CONTACTS
Run, world, as_precision = hl.Run, hl.world, hl.as_precision
SMALL = sl.SMALL
AUTO, OFF = B_.SMALL_TICK_AUTO, B_.SMALL_TICK_OFF
_hip = None


def read_device(addr, n, prec):
    """n reals of the batch's precision at a device address (host-mapped memory has one too)"""
    global _hip
    if _hip is None:
        _hip = C.CDLL(None)                      # the HIP runtime is already in the process
    buf = np.empty(n, prec)
    if n:
        assert addr
        assert _hip.hipMemcpy(C.c_void_p(buf.ctypes.data), C.c_void_p(addr), C.c_size_t(buf.nbytes), 2) == 0      # device to host
    return buf.astype(np.float64)


def island_scales(r, ref, Bp, vscale, h):
    """-> per island of the reference (F for forces, F for torques, largest component)"""
    out = []
    for n, I in enumerate(r.islands):
        fbs = [ref.joints[ref.joint_island == n].reshape(-1, 4, 3), ref.contacts[ref.contact_island == n].reshape(-1, 4, 3)]
        fmax = max([np.max(np.abs(x[:, 0::2]), initial=0.0) for x in fbs])
        tmax = max([np.max(np.abs(x[:, 1::2]), initial=0.0) for x in fbs])
        m_max, i_max = np.max(Bp.mass[I.slots]), np.max(Bp.inertia[I.slots])
        out.append((max(fmax, m_max * vscale / h), max(tmax, i_max * vscale / h), fmax, tmax))
    return out


def check_against_reference(prec, stepper, W, Bp, jts, art, lim, fj, fc, worst):
    """(a) and (b) for one tick; -> the reference's Result"""
    r, Wr, t = sl.reference_tick(prec, stepper, W, Bp, jts, art, lim)
    _, jr, ar, lr = as_precision(prec, W, jts, art, lim)
    ref = fd.feedback(Bp, r, jr, ar, lr)
    eps = EPS32 if np.dtype(prec).itemsize == 4 else 2.2e-16
    live = np.nonzero(Bp.flags & ld.ALIVE)[0]
    vscale = ld.velocity_scale(r.bodies, Wr, live)
    scales = island_scales(r, ref, Bp, vscale, Wr.h)
    ratio = 0.0
    for got, want, isl in ((fj, ref.joints, ref.joint_island), (fc, ref.contacts, ref.contact_island)):
        for k in range(len(want)):
            if isl[k] < 0:
                assert np.all(got[k] == 0), "an inactive joint or a dropped contact joint reports zeros"
                continue
            Ff, Ft, fmax, tmax = scales[isl[k]]
            for rows, F, big in ((slice(0, 4, 2), Ff, fmax), (slice(1, 4, 2), Ft, tmax)):
                err = np.max(np.abs(got[k][rows] - want[k][rows]))
                allowed = t * F + 4 * eps * big
                ratio = max(ratio, err / allowed)
    print(f"{prec} {stepper}: feedback error / allowed = {ratio:.3e} (t = {t:.2e})")
    worst[0] = max(worst[0], ratio)
    assert ratio <= 1.0, f"feedback error is {ratio:.3f} of what the velocity rule allows"
    # world sides report zeros, kinematic sides do not
    for k, a in enumerate(ar):
        if ref.joint_island[k] >= 0:
            for side, rows in (("body1", slice(0, 2)), ("body2", slice(2, 4))):
                if a[side] < 0:
                    assert np.all(fj[k][rows] == 0)
    # (b) zero net wrench about the origin
    pe, _ = sd.errors(Bp, ar, lr) if len(ar) else (np.zeros(0), None)
    for k, a in enumerate(ar):
        if ref.joint_island[k] >= 0 and a["body1"] >= 0 and a["body2"] >= 0:
            f, tq, big = fd.net_wrench(Bp, int(a["body1"]), int(a["body2"]), fj[k])
            assert np.all(f == 0), f"joint {k}: f1 + f2 = {f}"
            slack = pe[k] * np.max(np.abs(fj[k][0])) * np.sqrt(3.0) if a["kind"] != sd.SLIDER else 0.0
            assert np.max(np.abs(tq)) <= 64 * eps * big + slack, f"joint {k}: net torque {tq}, largest term {big}"
    for k, j in enumerate(jr):
        if ref.contact_island[k] >= 0 and int(j["body1"]) >= 0 and int(j["body2"]) >= 0:
            f, tq, big = fd.net_wrench(Bp, int(j["body1"]), int(j["body2"]), fc[k])
            assert np.all(f == 0) and np.max(np.abs(tq)) <= 64 * eps * big, f"contact {k}: net wrench {f} {tq}"
    return r


def run_case(prec, stepper, B, art, lim, jts=NO_CONTACTS, ticks=1, small=None, W=None):
    """a world with feedback on and its twin with it off, tick by tick; -> (the reference's Result per tick, lcp stats and
    small-tick stats of the world with feedback on, the same of its twin, [joint feedback, contact feedback] of the last tick)"""
    W = world() if W is None else W
    on, off = Run(prec, B, W, art, lim, stepper, small), Run(prec, B, W, art, lim, stepper, small)
    worst = [0.0]
    try:
        on.w.set_feedback(True)
        res = []
        for _ in range(ticks):
            Bp, post = on.tick(jts)
            _, post_off = off.tick(jts)
            fj, fc = on.w.joint_feedback(), on.w.contact_feedback(len(jts))
            assert np.array_equal(post, post_off), "(c) the state differs with feedback on"
            dj, dc = on.w.feedback_device()
            assert np.array_equal(read_device(dj, 12 * len(art), prec).reshape(-1, 4, 3), fj), "(d) joints"
            assert np.array_equal(read_device(dc, 12 * len(jts), prec).reshape(-1, 4, 3), fc), "(d) contacts"
            assert np.all(np.isfinite(fj)) and np.all(np.isfinite(fc))
            res.append(check_against_reference(prec, stepper, W, Bp, jts, art, lim, fj, fc, worst))
        return res, (on.w.lcp_stats(), on.w.small_tick_stats()), (off.w.lcp_stats(), off.w.small_tick_stats()), (Bp, post, fj, fc)
    finally:
        on.close()
        off.close()


def path_is(stats, small, ticks=1):
    """the same path with feedback on and off: the single-launch tick or the general one"""
    for _, st in stats:
        assert (st["small"], st["general"]) == ((ticks, 0) if small == AUTO else (0, ticks)), st


def same_path(on, off, small, ticks=1):
    """a world that may be too large for the single-launch tick: with the tick switched off it took the general path, left to the
    batch it took one of the two, and either way the same one with feedback on and off"""
    (_, a), (_, b) = on, off
    assert (a["small"], a["general"]) == (b["small"], b["general"]) and a["small"] + a["general"] == ticks, (a, b)
    if small == OFF:
        assert a["small"] == 0, a


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("swapped", [False, True])
@pytest.mark.parametrize("small", SMALL)
def test_one_body_on_a_slider_every_line_of_the_table(prec, stepper, swapped, small):
    """6-row islands, one per line of the limot's table, given as (body, world) and as (world, body): the joint's force lands on
    the side the body was given as, the world side reports zeros"""
    B, art, lim = sd.one_body_per_mode(swapped, sl.MODE_SEED)
    (r,), on, off, (_, _, fj, _) = run_case(prec, stepper, B, art, lim, small=small)
    path_is((on, off), small)
    body, wside = (slice(2, 4), slice(0, 2)) if swapped else (slice(0, 2), slice(2, 4))
    assert np.all(fj[:, wside] == 0) and np.all(np.any(fj[:, body] != 0, axis=(1, 2)))
    # a motor against a stop: the part of the joint's force along the axis is the limot row's multiplier (the shifted bound included)
    k = list(sd.MODES).index("low_stop_leaving")
    u = sd.rate_blocks(B, art[k])[1 if swapped else 0][:3]
    assert r.lams[k][5] == 0.5 and abs(fj[k][2 if swapped else 0] @ u - 0.5) <= (1e-5 if prec == "float32" else 1e-7)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("swapped", [False, True])
@pytest.mark.parametrize("small", SMALL)
def test_one_body_fixed_to_the_world(prec, stepper, swapped, small):
    B, art, lim = sd.one_body(None, swapped, sl.MODE_SEED, kind=sd.FIXED)
    _, on, off, _ = run_case(prec, stepper, B, art, lim, ticks=2, small=small)
    path_is((on, off), small, 2)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("kind,mode", [(sd.SLIDER, "low_stop_motor_into"), (sd.FIXED, None)])
@pytest.mark.parametrize("small", SMALL)
def test_a_kinematic_side_reports_its_share(prec, stepper, kind, mode, small):
    """two bodies, the first kinematic: its inverse mass is zero, its block of J is not"""
    B, art, lim = sd.two_bodies(kind, mode, kinematic=True, seed=sl.TWO_SEED)
    _, on, off, (_, _, fj, _) = run_case(prec, stepper, B, art, lim, ticks=2, small=small)
    path_is((on, off), small, 2)
    assert np.any(fj[0][0] != 0) and np.array_equal(fj[0][0], -fj[0][2])


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("small", SMALL)
def test_one_island_with_all_four_kinds(prec, stepper, small):
    B, art, lim = sd.all_kinds_chain(sl.CHAIN_SEED)
    (r,), on, off, _ = run_case(prec, stepper, B, art, lim, small=small)
    assert r.islands[0].m == 27
    path_is((on, off), small)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("small", SMALL)
def test_small_world_of_joints_contacts_and_free_bodies(prec, stepper, small):
    """48 bodies, 28 joints and 8 contact joints in 24 islands, three ticks: several islands per tick, one-body contact islands
    (which the single-launch tick's tail steps in their row form while feedback is on) and joints given as (world, body)"""
    B, art, lim, jts = sd.small_world(sl.WORLD_SEED)
    _, on, off, (_, _, fj, fc) = run_case(prec, stepper, B, art, lim, jts, ticks=3, small=small)
    path_is((on, off), small, 3)
    assert np.all(fc[:, 2:] == 0) and np.all(fc[:, 0, 1] >= 0) and np.any(fc[:, 0, 1] > 0)      # (ground contacts push up or have let go; the ground reports zeros)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("small", SMALL)
def test_star_on_ground_contacts(prec, stepper, small):
    B, art, lim, jts = sd.star(8, seed=sl.STAR_GROUND_SEED, contacts=True)
    (r,), on, off, _ = run_case(prec, stepper, B, art, lim, jts, small=small)
    path_is((on, off), small)
    assert r.islands[0].m == sd.star_rows(art, lim)[0] + 4


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", [40, 100])
@pytest.mark.parametrize("small", SMALL)
def test_star_under_dworldstep_over_three_ticks(prec, n, small):
    """bounded rows through the LDS solve (40 spokes in float32) and the grid solve (40 in float64, 100: 600 rows), whose write-back
    leaves lambda in the rows; three ticks, so that the grid solve starts from a carried active set"""
    B, art, lim, jts = sd.star(n, seed=sl.STAR_SEEDS[n])
    ticks = 3
    _, on, off, _ = run_case(prec, "exact", B, art, lim, jts, ticks=ticks, small=small)
    same_path(on, off, small, ticks)
    grid = n == 100 or prec == "float64"
    for lcp, st in (on, off):
        if st["general"] == ticks:
            assert lcp["solves"] == (ticks if grid else 0)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", [8, 40, 100])
@pytest.mark.parametrize("small", SMALL)
def test_star_under_quickstep(prec, n, small):
    """QuickStep's one-wavefront form (8 spokes: 47 rows; 40: 240 rows) and the workgroup's rows in registers (100: 587 rows)"""
    B, art, lim, jts = sd.star(n, seed=sl.STAR_SEEDS[n])
    _, on, off, _ = run_case(prec, "quick", B, art, lim, jts, small=small)
    same_path(on, off, small)


# ---------------------------------------------------------------------------------------------------------------------
def resting_bodies(counts=(1, 4, 5, 8), seed=2):
    """one body per entry of counts, each on that many contacts with static geometry (friction rows unbounded) and an island of its
    own: QuickStep's one-body forms' ranges, 1..4 contacts in registers and 5..8 in LDS"""
    rng = np.random.default_rng(seed)
    n = len(counts)
    quat = rng.normal(size=(n, 4))
    quat /= np.linalg.norm(quat, axis=1)[:, None]
    B = ld.Bodies(np.column_stack([0.8 * np.arange(n) - 1.2, np.full(n, 0.5), 0.1 * rng.normal(size=n)]), quat,
                  np.column_stack([0.2 * rng.normal(size=n), np.full(n, -1.0), 0.2 * rng.normal(size=n)]), 0.3 * rng.normal(size=(n, 3)),
                  rng.uniform(0.8, 1.6, n), rng.uniform(0.3, 0.8, (n, 3)))
    jts = []
    for s, c in enumerate(counts):
        for k in range(c):
            a = 2.0 * np.pi * (k + 0.3 * s) / c
            nrm = np.array([0.15 * np.cos(a), 1.0, 0.15 * np.sin(a)])
            sides = (s, -1) if k % 2 == 0 else (-1, s)          # (every other one as dJointAttach(c, 0, body) gives it: normal reversed)
            nrm = nrm / np.linalg.norm(nrm) * (1.0 if sides[0] >= 0 else -1.0)
            jts.append((B.pos[s] + (0.4 * np.cos(a), -0.5, 0.4 * np.sin(a)), nrm, 0.01, sides[0], sides[1], 0, np.inf, 0, 0, 0, 0))
    return B, np.array(jts, ld.JOINT_DTYPE)


# (cfm 1e-2: up to 24 rows on one body's six degrees of freedom are redundant, and kappa(A) ~ |A| h / cfm must leave float32's
#  10 eps32 kappa under 1e-3)
RESTING_CFM = 1e-2


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("small", SMALL)
def test_one_body_islands_of_1_4_5_and_8_static_contacts(prec, stepper, small):
    """the islands solve_singles and solve_singles_lds step without a row table when feedback is off; on, they take the row form.
    Contacts given as (body, 0) and as (0, body): the force is reported on the side the body was given as"""
    B, jts = resting_bodies()
    none = np.zeros(0, jd.ART_DTYPE)
    _, on, off, (_, _, _, fc) = run_case(prec, stepper, B, none, None, jts, ticks=2, small=small, W=world(cfm=RESTING_CFM))
    path_is((on, off), small, 2)
    given_first = jts["body1"] >= 0
    assert np.all(fc[given_first, 2:] == 0) and np.all(fc[~given_first, :2] == 0)
    assert np.all(np.any(fc[given_first, 0] != 0, axis=1)) and np.all(np.any(fc[~given_first, 2] != 0, axis=1))


def stack(n, seed=4):
    """n bodies in a column, each on the one below through one contact joint with friction (the lowest on the ground): one island
    of 3 n rows, three per contact throughout"""
    rng = np.random.default_rng(seed)
    quat = np.tile([1.0, 0.0, 0.0, 0.0], (n, 1))
    B = ld.Bodies(np.column_stack([0.02 * rng.normal(size=n), 0.5 + np.arange(n), 0.02 * rng.normal(size=n)]), quat,
                  np.column_stack([0.1 * rng.normal(size=n), np.full(n, -0.5), 0.1 * rng.normal(size=n)]), 0.1 * rng.normal(size=(n, 3)),
                  rng.uniform(0.8, 1.2, n), rng.uniform(0.15, 0.2, (n, 3)))
    jts = [(B.pos[s] + (0.0, -0.5, 0.0), (0.0, 1.0, 0.0), 0.005, s, s - 1, 0, np.inf, 0, 0, 0, 0) for s in range(n)]
    return B, np.array(jts, ld.JOINT_DTYPE)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", [20, 100])
@pytest.mark.parametrize("small", SMALL)
def test_quickstep_islands_of_contacts_only(prec, n, small):
    """contact-only islands with friction throughout: 60 rows -- the one-wavefront form, which builds such rows in registers when
    feedback is off and in the row table when it is on -- and 300 rows, the workgroup's register form (contacts as units in float32).
    The scenes are made here (stack): tests/test_gpu_large_island.py's own go through dmxBatchStep, which finds its contacts itself
    and produces no feedback, so they cannot be imported for this."""
    B, jts = stack(n)
    none = np.zeros(0, jd.ART_DTYPE)
    _, on, off, (_, _, _, fc) = run_case(prec, "quick", B, none, None, jts, W=world(cfm=RESTING_CFM), small=small)
    same_path(on, off, small)
    assert np.all(fc[:, 0, 1] > 0) and np.array_equal(fc[1:, 0], -fc[1:, 2])


def pairs_beside_a_stack(n_pairs=1025, n_stack=100, seed=6):
    """a stack of n_stack bodies (one island of 3 n_stack rows) and n_pairs islands of two bodies meeting in one contact with
    friction: more islands with two bodies or more than the workgroup's register form takes in one launch (1 024), so that the
    stack's rows -- more than one wavefront holds -- are streamed by its workgroup"""
    B, jts = stack(n_stack)
    rng = np.random.default_rng(seed)
    n = 2 * n_pairs
    pos = np.zeros((n, 3))
    pos[0::2] = np.column_stack([3.0 + 1.5 * (np.arange(n_pairs) % 32), np.full(n_pairs, 1.0), 1.5 * (np.arange(n_pairs) // 32)])
    pos[1::2] = pos[0::2] + (0.0, 1.0, 0.0)
    lvel = 0.1 * rng.normal(size=(n, 3))
    lvel[1::2, 1] -= 0.5
    P = ld.Bodies(pos, np.tile([1.0, 0.0, 0.0, 0.0], (n, 1)), lvel, 0.1 * rng.normal(size=(n, 3)), rng.uniform(0.8, 1.2, n), rng.uniform(0.15, 0.2, (n, 3)))
    pj = np.array([(P.pos[2 * k] + (0.0, 0.5, 0.0), (0.0, 1.0, 0.0), 0.005, B.n + 2 * k + 1, B.n + 2 * k, 0, np.inf, 0, 0, 0, 0) for k in range(n_pairs)],
                  ld.JOINT_DTYPE)
    Bm = ld.Bodies(np.vstack([B.pos, P.pos]), np.vstack([B.quat, P.quat]), np.vstack([B.lvel, P.lvel]), np.vstack([B.avel, P.avel]),
                   np.concatenate([B.mass, P.mass]), np.vstack([B.inertia, P.inertia]))
    return Bm, np.concatenate([jts, pj])


@pytest.mark.parametrize("prec", PRECS)
def test_quickstep_streamed_rows_of_a_large_island_among_many(prec):
    """the workgroup form that streams an island's rows level by level and stores lambda with every row update (a scene made here,
    pairs_beside_a_stack, for the reason test_quickstep_islands_of_contacts_only gives)"""
    B, jts = pairs_beside_a_stack()
    none = np.zeros(0, jd.ART_DTYPE)
    (r,), on, off, _ = run_case(prec, "quick", B, none, None, jts, W=world(cfm=RESTING_CFM))
    assert sum(1 for I in r.islands if len(I.slots) > 1) > 1024 and max(I.m for I in r.islands) == 300
    for _, st in (on, off):
        assert (st["small"], st["general"], st["bodies"]) == (0, 1, 1)


@pytest.mark.parametrize("prec", PRECS)
def test_ode_row_order_with_contact_joints_only(prec):
    """DMX_ORDER_ODE: QuickStep's sequential sweeps in ODE's shuffled orders.  The dense reference does not shuffle, so there is
    nothing for (a) to compare with here: it is replaced by each body's own balance, which holds whatever the order: m (v' - v) / h = m g + the feedback forces on it, and
    the same for the torques with the body's world inertia (no gyroscopic term: the scene's gyro mode is off).  v' = v + h (...) is a
    handful of roundings of v, the sums a few per row: 8 (1 + rows on the body) eps of the largest term"""
    B, jts = resting_bodies()
    B2, j2 = stack(6)
    B2.pos[:, 0] += 3.0
    j2["pos"][:, 0] += 3.0
    j2["body1"] += B.n
    j2["body2"][1:] += B.n
    Bm = ld.Bodies(np.vstack([B.pos, B2.pos]), np.vstack([B.quat, B2.quat]), np.vstack([B.lvel, B2.lvel]), np.vstack([B.avel, B2.avel]),
                   np.concatenate([B.mass, B2.mass]), np.vstack([B.inertia, B2.inertia]))
    jts = np.concatenate([jts, j2])
    none = np.zeros(0, jd.ART_DTYPE)
    W = world(cfm=RESTING_CFM)
    on, off = Run(prec, Bm, W, none, None, "quick"), Run(prec, Bm, W, none, None, "quick")
    eps = EPS32 if prec == "float32" else 2.2e-16
    try:
        for r in (on, off):
            r.w.set_row_order(B_.ORDER_ODE, 7)
        on.w.set_feedback(True)
        for _ in range(2):
            Bp, post = on.tick(jts)
            _, post_off = off.tick(jts)
            assert np.array_equal(post, post_off), "(c)"
            fc = on.w.contact_feedback(len(jts))
            _, dc = on.w.feedback_device()
            assert np.array_equal(read_device(dc, 12 * len(jts), prec).reshape(-1, 4, 3), fc), "(d)"
            g = np.asarray(W.gravity, np.float32 if prec == "float32" else np.float64).astype(np.float64)
            worst = 0.0
            for s in range(Bm.n):
                f, tq, rows = Bp.mass[s] * g, np.zeros(3), 0
                for k, j in enumerate(jts):
                    for side, blk in (("body1", 0), ("body2", 2)):
                        if j[side] == s:
                            f, tq, rows = f + fc[k][blk], tq + fc[k][blk + 1], rows + 3
                R = ld.quat_to_R(Bp.quat[s])
                Iw = R @ np.diag(Bp.inertia[s]) @ R.T
                df = Bp.mass[s] * (post[s, 7:10] - Bp.lvel[s]) / W.h - f
                dt = Iw @ (post[s, 10:13] - Bp.avel[s]) / W.h - tq
                bigf = max(np.max(np.abs(f)), Bp.mass[s] * np.max(np.abs(post[s, 7:10])) / W.h, np.max(np.abs(fc[:, 0::2])))
                bigt = max(np.max(np.abs(tq)), np.max(Bp.inertia[s]) * np.max(np.abs(post[s, 10:13])) / W.h, np.max(np.abs(fc[:, 1::2])))
                worst = max(worst, np.max(np.abs(df)) / (8 * (1 + rows) * eps * bigf), np.max(np.abs(dt)) / (8 * (1 + rows) * eps * bigt))
            print(f"{prec}: body balance error / allowed = {worst:.3e}")
            assert worst <= 1.0
        for r in (on, off):
            st = r.w.small_tick_stats()
            assert st["small"] == 0 and st["row_order"] == 2, st
    finally:
        on.close()
        off.close()


# ---------------------------------------------------------------------------------------------------------------------
def test_getters_refuse_what_they_must():
    B, jts = resting_bodies()
    run = Run("float64", B, world(), np.zeros(0, jd.ART_DTYPE), None, "quick")
    w = run.w

    def refused(f, *a):
        with pytest.raises(B_.DmxError) as e:
            f(*a)
        assert e.value.code == EINVAL

    try:
        refused(w.contact_feedback, len(jts))              # feedback is off
        refused(w.joint_feedback)
        refused(w.feedback_device)
        run.tick(jts)
        refused(w.contact_feedback, len(jts))              # still off: the tick left none
        w.set_feedback(True)
        refused(w.contact_feedback, len(jts))              # no tick since it was switched on
        refused(w.joint_feedback)
        refused(w.feedback_device)
        run.tick(jts)
        assert w.contact_feedback(len(jts)).shape == (len(jts), 4, 3) and w.joint_feedback().shape == (0, 4, 3)
        assert np.array_equal(w.contact_feedback(), w.contact_feedback(len(jts)))          # (the binding remembers the last tick's n)
        refused(w.contact_feedback, len(jts) - 1)          # a wrong n
        refused(w.contact_feedback, 0)
        w.step(hl.H, 1)                                    # a tick that finds its own contacts produces none
        refused(w.contact_feedback, len(jts))
        refused(w.feedback_device)
        run.tick(jts[:3])
        assert np.any(w.contact_feedback(3) != 0)
        refused(w.contact_feedback, len(jts))
        w.set_feedback(False)
        refused(w.contact_feedback, 3)
    finally:
        run.close()


def test_a_new_joint_set_drops_the_last_ticks_feedback():
    """the last tick's feedback has one entry per joint of the set it was made with: after dmxBatchSetJoints, with fewer joints or
    with more, the getters refuse it (joint_feedback() sizes its result by joint_count(), the new set) until a tick has been made"""
    B, art, lim = sd.one_body_per_mode(False, sl.MODE_SEED)
    run = Run("float64", B, world(), art, lim, "quick")
    w = run.w
    try:
        w.set_feedback(True)
        run.tick(NO_CONTACTS)
        assert w.joint_feedback().shape == (len(art), 4, 3)
        for keep in (1, len(art)):             # (fewer; and after a tick with one joint, more)
            w.set_joints(hl.to_c(art[:keep], B_.JOINT_DTYPE))
            assert w.joint_count() == keep
            for f in (w.joint_feedback, w.contact_feedback, w.feedback_device):
                with pytest.raises(B_.DmxError) as e:
                    f()
                assert e.value.code == EINVAL
            run.tick(NO_CONTACTS)
            fj = w.joint_feedback()
            assert fj.shape == (keep, 4, 3) and np.all(np.any(fj[:, :2] != 0, axis=(1, 2)))
    finally:
        run.close()
