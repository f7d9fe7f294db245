"""dmxBatchStepJoints (both steppers, both precisions) against the dense float64 reference (tests/lcp_dense.py).

Every case builds a synthetic joint list -- the solver takes any contacts, none come from a collider -- uploads a state, makes
one step_joints call and downloads the result; the reference runs from the device's own pre-tick state (downloaded, cast to
float64), so only the tick itself is compared.  Cases aim at the kernel choices an island's row count makes (singles, the
wavefront / workgroup SOR forms, the one-workgroup LDS exact solve, the grid solve) and at the row semantics no oracle test
reaches (per-contact mu / bounce / soft ERP / soft CFM, bounded friction, kinematic bodies).

Tolerances (velocities, relative to max(|v_ref|, g h); positions the same times h, plus the rounding of x + h v):
  * float64 QuickStep 1e-10: the same sweeps in the same order, only the summation order differs;
  * float64 dWorldStep 1e-8: two exact methods on one positive definite system;
  * float32 dWorldStep c eps32 kappa(A), c = 10: a backward-stable solve in float32 of a system with condition number kappa
    (computed by the reference per island);
  * float32 QuickStep: the band of tests/quick_band.py, per body -- K eps32 M_v with M_v = |v| + h |M^-1 f| + h |M^-1 J^T| |lambda|
    from the reference's own lambda, K = quick_band.K["contact"] measured on the CPU (tests/test_quick_band.py); rows at
    their bounds included, no gate (the clamp is non-expansive).  Every float32 QuickStep case is built by a function listed
    in F32_QUICK_CASES, which tests/test_quick_band.py runs the float32 emulation of the reference's sweeps over.
The DMX_* knobs are read once per process: cases that need one run in a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import lcp_dense as ld
import quick_band as qb
from __graft_entry__ import load_package

pkg = load_package()
B_ = pkg.batch
pytestmark = pytest.mark.gpu

H = 1.0 / 60.0
EPS32 = float(np.finfo(np.float32).eps)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def lds_fits(real_bytes, m, nbd, lim=150 * 1024):
    """csrc/dmx_lcp.hip lcp_lds_fits: whether an island's exact solve fits one workgroup's LDS"""
    if m + 1 > (288 if real_bytes == 4 else 192):
        return False
    nu = m - nbd
    reals = (m + 1) * (m + 2) // 2 + (nbd + 1) * (nbd + 2) // 2 + 4 * nbd + nu + max(nu, 2 * nbd) + 8
    return ((reals * real_bytes + 15) // 16) * 16 + (3 * m + 3 * nbd + 16) * 4 <= lim


def rows_of(mus):
    """(m, nu, nbd) of contacts with these mu: 1 row with mu = 0, 3 otherwise, 2 of them unbounded with mu = inf"""
    mus = np.asarray(mus, np.float64)
    m = int(np.sum(np.where(mus > 0, 3, 1)))
    nu = int(2 * np.sum(np.isinf(mus)))
    return m, nu, m - nu


def lds_boundary(real_bytes, make):
    """the first row count whose island (contacts make(m)) does not fit the LDS solve; the one before it still fits"""
    m = 1
    while lds_fits(real_bytes, m, rows_of(make(m))[2]):
        m += 1
    return m


# ---------------------------------------------------------------------------------------------------------------------
def chain(nb, n_contacts, mu, rng, static_first=True, mode=ld.CONTACT_BOUNCE, speed=0.3, aniso=True, mass=(0.5, 2.0)):
    """nb bodies in a chain along y (slot k rests on k - 1, slot 0 on static ground), n_contacts contacts spread round-robin
    over the links; `mu` a number or a per-contact array.  Contact points within 0.6 of body1's centre, normals within
    ~25 degrees of the link's axis, depths in [0, 0.05]."""
    pos = np.column_stack([rng.uniform(-0.05, 0.05, nb), 0.5 + np.arange(nb), rng.uniform(-0.05, 0.05, nb)])
    quat = np.array([_unit(rng.normal(size=4)) for _ in range(nb)])
    B = ld.Bodies(pos, quat, rng.normal(scale=speed, size=(nb, 3)), rng.normal(scale=speed, size=(nb, 3)),
                  rng.uniform(*mass, nb), rng.uniform(0.2, 1.0, (nb, 3)) if aniso else np.ones((nb, 3)))
    links = ([(0, -1)] if static_first else []) + [(k, k - 1) for k in range(1, nb)]
    mus = np.broadcast_to(np.asarray(mu, np.float64), (n_contacts,))
    out = []
    for c in range(n_contacts):
        b1, b2 = links[c % len(links)]
        axis = B.pos[b1] - B.pos[b2] if b2 >= 0 else np.array([0.0, 1.0, 0.0])
        n = _unit(_unit(axis) + 0.4 * _unit(rng.normal(size=3)))
        p = B.pos[b1] + 0.6 * rng.uniform(0.2, 1.0) * _unit(rng.normal(size=3))
        out.append((p, n, rng.uniform(0, 0.05), b1, b2, mode, mus[c], 0.2, 0.1, 0.0, 0.0))
    return B, np.array(out, ld.JOINT_DTYPE)


def contacts_for_rows(m, mu):
    """contacts (with their mu) that make exactly m rows: m // 3 three-row contacts and m % 3 one-row ones (mu = 0);
    mu = "mix": contacts with mu 0.4, inf and 0 in turn, one-row contacts at the end to make up m"""
    if mu == 0:
        return np.zeros(m)
    if isinstance(mu, str):
        out, rows = [], 0
        for k in range(m):
            nxt = (0.4, np.inf, 0.0)[k % 3]
            if rows + (3 if nxt > 0 else 1) > m:
                break
            out.append(nxt)
            rows += 3 if nxt > 0 else 1
        return np.concatenate([out, np.zeros(m - rows)])
    return np.concatenate([np.full(m // 3, mu), np.zeros(m % 3)])


def press_chain(m, rng):
    """m rows of frictionless contacts, three per link of a chain of ceil(m / 3) bodies along y; each contact's normal is
    tilted 34 degrees from the chain's axis, the three of a link 120 degrees apart, and every body moves down faster than the
    one below it.  No row is redundant and every normal row stays loaded: the reference's clamp margin is ~1e-2 of the
    largest lambda."""
    nb = -(-m // 3)
    pos = np.column_stack([np.zeros(nb), 0.5 + np.arange(nb), np.zeros(nb)])
    lv = np.zeros((nb, 3))
    lv[:, 1] = -(1.0 + 0.1 * np.arange(nb))
    B = ld.Bodies(pos, np.tile([1.0, 0, 0, 0], (nb, 1)), lv, np.zeros((nb, 3)), rng.uniform(0.8, 1.2, nb),
                  rng.uniform(0.3, 0.5, (nb, 3)))
    out = []
    for c in range(m):
        k = c // 3
        a = 2 * np.pi * (c % 3) / 3 + 0.3 * k
        d = np.array([np.cos(a), 0.0, np.sin(a)])
        n = np.array([0.0, np.cos(0.6), 0.0]) + d * np.sin(0.6)
        out.append((np.array([0.0, float(k), 0.0]) + 0.3 * d, n, 0.01, k, k - 1 if k else -1, 0, 0.0, 0, 0, 0, 0))
    return B, np.array(out, ld.JOINT_DTYPE)


def device_tick(prec, B, W, jts, stepper, ticks=1, between=None, small=None):
    """-> list per tick of (pre-tick Bodies as the device held them, the tick's joints, post-tick state (n,13), lcp stats after
    the tick, with the small tick's counters under "tick").  `between(t, jts)` gives tick t's joints, or (joints, flags): the
    flags are uploaded before the tick and are the ones the pre-tick Bodies carry from then on.  `small`: set_small_tick"""
    dt = np.dtype(prec)
    w = B_.BatchWorld(B.n, prec, gravity=tuple(W.gravity))
    try:
        w.set_erp(W.erp); w.set_cfm(W.cfm); w.set_quickstep(W.iters, W.sor_w); w.set_gyro_mode(W.gyro)
        w.set_stepper(B_.STEPPER_EXACT if stepper == "exact" else B_.STEPPER_QUICK)
        if small is not None:
            w.set_small_tick(small)
        w.upload(B_.POS, B.pos); w.upload(B_.QUAT_RAW, B.quat); w.upload(B_.LVEL, B.lvel); w.upload(B_.AVEL, B.avel)
        w.upload(B_.MASS, B.mass); w.upload(B_.INERTIA, B.inertia)
        w.upload_body_flags(B.flags)
        mass = w.download(B_.MASS).astype(np.float64).reshape(-1)
        inertia = w.download(B_.INERTIA).astype(np.float64)
        out = []
        flags = B.flags
        for t in range(ticks):
            j = between(t, jts) if between else jts
            if isinstance(j, tuple):
                j, flags = j
                w.upload_body_flags(flags)
            pre = w.download(B_.STATE).astype(np.float64)
            Bp = ld.Bodies(pre[:, 0:3], pre[:, 3:7], pre[:, 7:10], pre[:, 10:13], mass, inertia, flags)
            w.step_joints(W.h, j.astype(B_.CONTACT_JOINT_DTYPE))
            w.synchronize()
            post = w.download(B_.STATE).astype(np.float64)
            out.append((Bp, j, post, dict(w.lcp_stats(), tick=w.small_tick_stats())))
        return out
    finally:
        w.close()


def as_precision(prec, W, jts):
    """the world parameters and joint fields as the device holds them (rounded to float32 in a float32 batch)"""
    if np.dtype(prec).itemsize == 8:
        return W, jts
    r = lambda x: float(np.float32(x))
    W2 = ld.World(h=r(W.h), gravity=np.asarray(W.gravity, np.float32).astype(np.float64), erp=r(W.erp), cfm=r(W.cfm),
                  iters=W.iters, sor_w=r(W.sor_w), gyro=W.gyro)
    j2 = jts.copy()
    for f in ("pos", "normal", "depth", "mu", "bounce", "bounce_vel", "soft_erp", "soft_cfm"):
        j2[f] = np.asarray(jts[f], np.float32).astype(np.float64)
    return W2, j2


DEVICE_WORST = {"contact": 0.0}          # the largest device deviation of this process, in eps32 M_v (printed by check)


def check(prec, B, W, jts, stepper, tol=None, ticks=1, between=None, small=None):
    """run the device and compare every tick with the reference (from the device's pre-tick state, with the flags then in
    force); -> list of (reference Result, lcp stats); the Result carries the device's post-tick state as `.device`"""
    res = []
    for Bp, j, post, stats in device_tick(prec, B, W, jts, stepper, ticks, between, small):
        Wr, jr = as_precision(prec, W, j)
        r = ld.step(Bp, Wr, jr, stepper)
        f32 = np.dtype(prec).itemsize == 4
        live = np.nonzero(Bp.flags & ld.ALIVE)[0]
        if f32 and stepper == "quick" and tol is None:
            worst = qb.assert_in_band(r, Wr, post, qb.K["contact"], live)
            DEVICE_WORST["contact"] = max(DEVICE_WORST["contact"], worst)
            print(f"f32 QuickStep on the device: {worst:.2f} eps32 M_v (K = {qb.K['contact']}; largest so far "
                  f"{DEVICE_WORST['contact']:.2f})")
        else:
            if tol is not None:
                t = tol
            elif not f32:
                t = 1e-10 if stepper == "quick" else 1e-8
            else:
                t = 10 * EPS32 * max([I.kappa() for I in r.islands] + [1.0])
            scale = ld.velocity_scale(r.bodies, Wr, live)
            err = ld.velocity_error(r.bodies, post[:, 7:10], post[:, 10:13], live)
            assert err <= t * scale, f"velocity error {err:.3e} > {t:.1e} x {scale:.3e}"
            eps = 4 * (EPS32 if f32 else 2.2e-16)
            xerr = np.max(np.abs(post[live, 0:3] - r.bodies.pos[live]))
            assert xerr <= t * scale * Wr.h + eps * max(1.0, np.max(np.abs(r.bodies.pos[live]))), f"position error {xerr:.3e}"
            qerr = np.max(np.abs(post[live, 3:7] - r.bodies.quat[live]))
            assert qerr <= t * scale * Wr.h + eps, f"quaternion error {qerr:.3e}"
        dead = np.nonzero(~(Bp.flags & ld.ALIVE).astype(bool))[0]
        if len(dead):
            pre_dead = np.column_stack([Bp.pos, Bp.quat, Bp.lvel, Bp.avel])[dead]
            assert np.array_equal(post[dead], pre_dead), "a dead slot changed"
        r.device = post
        res.append((r, stats))
    return res


PRECS = ["float64", "float32"]


def world(prec, **kw):
    """cfm 1e-5 in both precisions (dWorldCreate's float32 default): with float64's 1e-10 a few coplanar contacts make
    kappa(A) ~ 1e10 and no float64 solve, the reference's included, is certifiable at 1e-12"""
    return ld.World(cfm=1e-5, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# a. singles
def single_case(nc):
    rng = np.random.default_rng(100 + nc)
    B, jts = chain(1, nc, np.inf, rng, speed=0.05)
    B.lvel[0] = (0.1, -1.0, 0.0)                 # pressing into the ground
    return B, jts


@pytest.mark.parametrize("prec,stepper", [("float64", "quick"), ("float64", "exact"), ("float32", "exact"), ("float32", "quick")])
@pytest.mark.parametrize("nc", [1, 2, 5, 8, 9])
def test_single_body_on_static_ground(prec, stepper, nc):
    """one body with 1..8 contacts (solve_singles' lane) and 9 (an island of its own) against static ground.  (nc = 1 under
    QuickStep: three rows on one body are at their fixed point long before the last sweep -- the 20th moves the velocities by
    4e-5 of the float32 band -- so this one case cannot show a dropped sweep; every other can.)"""
    B, jts = single_case(nc)
    check(prec, B, world(prec), jts, stepper)


def canonicalisation_case():
    rng = np.random.default_rng(5)
    B, jts = chain(3, 6, np.inf, rng, speed=0.05)
    B.lvel[:, 1] = -1.0
    flags = np.full(4, ld.ALIVE, np.uint8)
    flags[3] = 0                                                    # slot 3: dead
    B = ld.Bodies(np.vstack([B.pos, [5, 5, 5]]), np.vstack([B.quat, [1, 0, 0, 0]]), np.vstack([B.lvel, [0, 0, 0]]),
                  np.vstack([B.avel, [0, 0, 0]]), np.append(B.mass, 1.0), np.vstack([B.inertia, [1, 1, 1]]), flags)
    extra = jts[:4].copy()
    extra[0]["body1"], extra[0]["body2"], extra[0]["normal"] = -1, 2, -jts[0]["normal"]     # static body1: swap + flip
    extra[1]["body1"], extra[1]["body2"] = 1, 3                                              # dead slot = static
    extra[2]["body1"], extra[2]["body2"] = -1, 3                                             # static - static
    extra[3]["body1"], extra[3]["body2"] = 2, 2                                              # self-joint
    return B, np.concatenate([jts, extra])


@pytest.mark.parametrize("prec", PRECS)
def test_canonicalisation_of_joints(prec):
    """body1 = -1 (the normal must come out reversed), a joint to a dead slot (static), a joint between two static bodies
    and a self-joint (both ignored)"""
    B, jts = canonicalisation_case()
    for stepper in ("quick", "exact"):
        check(prec, B, world(prec), jts, stepper)


# ---------------------------------------------------------------------------------------------------------------------
# b. QuickStep islands around the kernel thresholds
@pytest.mark.parametrize("prec,m", [("float64", 30), ("float64", 256), ("float64", 257), ("float64", 1536), ("float64", 1537)])
def test_quickstep_island_row_counts(prec, m):
    """float64 island row counts at WAVE_ISLAND_ROWS (256 / 257) and REGS_ROWS<double> (1 536) and one more; mu = 0, one row
    per contact.  (float32: test_quickstep_register_form_f32)"""
    rng = np.random.default_rng(m)
    B, jts = chain(max(2, m // 4), m, 0.0, rng, speed=0.02)
    B.lvel[:, 1] -= 1.0 + 0.1 * np.arange(B.n)             # every body pressing into the one below: normal rows stay positive
    check(prec, B, world(prec, gravity=(0, -9.8, 0)), jts, "quick")


@pytest.mark.parametrize("m", [256, 257, 1025, 3072, 3073])
def test_quickstep_register_form_f32(m):
    """float32 QuickStep islands at WAVE_ISLAND_ROWS, just above 1 024 rows (the 512-thread register form of
    solve_island_wg, compiled for float only) and at REGS_ROWS<float> (3 072) and one more; every row loaded"""
    B, jts = press_chain(m, np.random.default_rng(m))
    (r, _), = check("float32", B, world("float32"), jts, "quick")
    assert r.islands[0].m == m


CLAMP_SEEDS = {255: 255, 258: 258, 1025: 1025, 3073: 3073}      # chosen on the CPU (tests/test_quick_band.py holds what they must give)


def clamp_chain(m, seed=None):
    """a chain whose island has exactly m rows, with mu drawn from {0, 0.4, inf} per contact (one-row contacts at the end make
    up m) and the flags of SURFACES["bounce_mixed"]: bounce on about half of the contacts, restitution 0.7 above 0.05.  The
    bodies move at random (speed 0.3), so normal rows end at 0 and friction rows at +-mu"""
    rng = np.random.default_rng(CLAMP_SEEDS.get(m, m) if seed is None else seed)
    mus, rows = [], 0
    while rows < m:
        mu = rng.choice([0.0, 0.4, np.inf])
        if rows + (3 if mu > 0 else 1) > m:
            mu = 0.0
        mus.append(mu)
        rows += 3 if mu > 0 else 1
    B, jts = chain(max(2, len(mus) // 3), len(mus), np.array(mus), rng)
    jts["mode"] = np.where(rng.random(len(jts)) < 0.5, ld.CONTACT_BOUNCE, 0)
    jts["bounce"], jts["bounce_vel"] = 0.7, 0.05
    return B, jts


@pytest.mark.parametrize("m", [255, 258, 1025, 3073])
def test_quickstep_forms_with_clamping_rows_f32(m):
    """one island per float32 QuickStep kernel form whose rows clamp and carry surface flags: at and just past the
    one-wavefront form (255 / 258 rows), the 512-thread register form (1 025) and the streamed form above REGS_ROWS<float>
    (3 073).  The reference has normal rows at 0 and friction rows at both bounds (asserted)"""
    B, jts = clamp_chain(m)
    (r, _), = check("float32", B, world("float32"), jts, "quick")
    (I,), (lam,) = r.islands, r.lams
    assert I.m == m
    fr = np.isfinite(I.hi)
    assert np.any(lam[I.row_kind == 0] == 0) and np.any(lam[fr] == I.hi[fr]) and np.any(lam[fr] == I.lo[fr])


# ---------------------------------------------------------------------------------------------------------------------
# c. exact solve in one workgroup, d. the grid solve
def _exact_case(prec, m, mu, seed):
    rng = np.random.default_rng(seed)
    mus = contacts_for_rows(m, mu)
    nb = max(1, len(mus) // 3)
    B, jts = chain(nb, len(mus), mus, rng)
    return B, jts


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("mu", [0.0, 0.4, np.inf, "mix"])
@pytest.mark.parametrize("m", [1, 3, 63, 64, 65, "last", "over"])
def test_exact_island_sizes(prec, m, mu):
    """row counts 1, 3, 63, 64, 65, the last that fits lcp_lds_fits and the first that does not; all mu = 0 (nu = 0), all
    finite mu, all infinite, and a per-contact mix (contacts_for_rows: rows a three-row contact cannot make up are
    frictionless one-row contacts, so the island has exactly m rows).  The path is asserted: the grid solve's counter
    moves exactly when the island does not fit the LDS"""
    rb = np.dtype(prec).itemsize
    if m in ("last", "over"):
        first_out = lds_boundary(rb, lambda k: contacts_for_rows(k, mu))
        m = first_out - 1 if m == "last" else first_out
    B, jts = _exact_case(prec, m, mu, seed=m)
    (r, st), = check(prec, B, world(prec), jts, "exact")
    big = max(r.islands, key=lambda I: I.m)
    assert big.m == m
    grid = not lds_fits(rb, big.m, big.nbd) or big.m >= int(os.environ.get("DMX_LCP_GRID_ROWS", 1 << 30))
    assert (st["solves"] > 0) == grid
    if grid:
        assert (st["last_m"], st["last_nu"], st["last_nbd"]) == (big.m, big.nu, big.nbd)
        assert st["fallback"] == 0


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("nu,nbd", [(0, 300), (62, 240), (64, 241), (66, 242), (128, 243), (128, 64), (128, 65),
                                    (256, 129), (2, 1)])
def test_exact_grid_tiles(prec, nu, nbd):
    """the grid solve around its 64-row tiles: nu unbounded rows and nbd bounded ones, exactly.  Contacts make them: mu = inf
    gives 1 bounded + 2 unbounded rows, finite mu 3 bounded, mu = 0 1 bounded -- so nu is even and nu <= 2 nbd (63 / 65
    unbounded rows cannot be formed; 62 / 64 / 66 take their place).  Islands that fit the LDS (the small ones of float32,
    and (2, 1)) take the one-workgroup solve, unless DMX_LCP_GRID_ROWS sends them to the grid (a child case)"""
    rng = np.random.default_rng(nu * 1000 + nbd)
    n_inf = nu // 2
    rest = nbd - n_inf
    mus = np.concatenate([np.full(n_inf, np.inf), np.full(rest // 3, 0.4), np.zeros(rest % 3)])
    B, jts = chain(max(2, len(mus) // 3), len(mus), mus, rng)
    (r, st), = check(prec, B, world(prec), jts, "exact")
    big = max(r.islands, key=lambda I: I.m)
    assert (big.nu, big.nbd) == (nu, nbd)
    grid = not lds_fits(np.dtype(prec).itemsize, big.m, big.nbd) or big.m >= int(os.environ.get("DMX_LCP_GRID_ROWS", 1 << 30))
    assert (st["solves"] > 0) == grid
    if grid:
        assert (st["last_m"], st["last_nu"], st["last_nbd"]) == (big.m, nu, nbd)


@pytest.mark.parametrize("prec", ["float64"])
def test_exact_one_large_island(prec):
    """one island of ~1 100 rows (mixed friction): the grid solve"""
    rng = np.random.default_rng(77)
    mus = rng.choice([0.0, 0.4, np.inf], size=480)
    B, jts = chain(120, len(mus), mus, rng)
    (r, st), = check(prec, B, world(prec), jts, "exact")
    assert st["solves"] == 1 and st["last_m"] == r.islands[0].m and st["fallback"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# e. bounds that bind, f. surface fields
@pytest.mark.parametrize("prec", PRECS)
def test_friction_ends_at_both_bounds(prec):
    """finite mu, two boxes sliding in opposite directions: the reference has friction rows at hi and at lo (ST_HI)"""
    out_B, out_j = [], []
    for k, vx in enumerate((3.0, -3.0)):
        pos = [[3.0 * k, 0.5, 0.0]]
        B = ld.Bodies(pos, [[1, 0, 0, 0]], [[vx, -0.2, 0.5]], [[0, 0, 0]], [1.0], [[0.3, 0.4, 0.5]])
        for dx, dz in ((-0.5, -0.5), (0.5, -0.5), (0.5, 0.5), (-0.5, 0.5)):
            out_j.append(((3.0 * k + dx, 0.0, dz), (0, 1, 0), 0.01, k, -1, 0, 0.5, 0, 0, 0, 0))
        out_B.append(B)
    B = ld.Bodies(*[np.vstack([getattr(b, f) for b in out_B]) for f in ("pos", "quat", "lvel", "avel")],
                  np.array([1.0, 1.0]), np.vstack([b.inertia for b in out_B]))
    jts = np.array(out_j, ld.JOINT_DTYPE)
    (r, _), = check(prec, B, world(prec), jts, "exact")
    assert sum(i["n_hi"] for i in r.infos) >= 4 and sum(i["n_lo"] for i in r.infos) >= 4


def separating_case():
    rng = np.random.default_rng(9)
    B, jts = chain(3, 6, np.inf, rng, speed=0.0)
    B.lvel[:, 1] = 2.0 + np.arange(3) * 3.0
    jts["depth"] = 0.0
    return B, jts


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", ["quick", "exact"])
def test_separating_contacts_end_at_zero(prec, stepper):
    """contacts whose bodies fly apart: the normal rows end at lo = 0"""
    B, jts = separating_case()
    (r, _), = check(prec, B, world(prec, gravity=(0, 0, 0)), jts, stepper)
    if stepper == "exact":
        assert all(np.all(lam[I.row_kind == 0] == 0) for I, lam in zip(r.islands, r.lams))


def _surface_case(seed, **fields):
    rng = np.random.default_rng(seed)
    B, jts = chain(4, 12, rng.choice([0.0, 0.5, np.inf], 12), rng, speed=0.8)
    for k, v in fields.items():
        jts[k] = v(rng, len(jts)) if callable(v) else v
    return B, jts


SURFACES = {
    "bounce_mixed": dict(mode=lambda r, n: np.where(r.random(n) < 0.5, ld.CONTACT_BOUNCE, 0), bounce=0.7, bounce_vel=0.05),
    "bounce_vel_negative": dict(mode=ld.CONTACT_BOUNCE, bounce=0.7, bounce_vel=-1.0),
    "negative_depth": dict(depth=lambda r, n: r.uniform(-0.05, 0.05, n)),
    "soft_erp_0": dict(mode=ld.CONTACT_SOFT_ERP, soft_erp=0.0),
    "soft_erp_08": dict(mode=ld.CONTACT_SOFT_ERP | ld.CONTACT_BOUNCE, soft_erp=0.8),
    "soft_cfm_1e-3": dict(mode=ld.CONTACT_SOFT_CFM, soft_cfm=1e-3),
    "soft_cfm_0": dict(mode=ld.CONTACT_SOFT_CFM, soft_cfm=0.0),
}


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", ["quick", "exact"])
@pytest.mark.parametrize("surface", sorted(SURFACES))
def test_per_contact_surface_fields(prec, stepper, surface):
    """per-contact bounce / bounce_vel / depth / dContactSoftERP / dContactSoftCFM, with mixed mu in one island"""
    B, jts = _surface_case(11, **SURFACES[surface])
    check(prec, B, world(prec), jts, stepper)


# ---------------------------------------------------------------------------------------------------------------------
# g. bodies, h. degenerate contacts
def kinematic_case(prec):
    rng = np.random.default_rng(21)
    B1, j1 = chain(3, 9, 0.4, rng)             # each stack's lowest body rests on "static" (-1): remapped to the slab below
    B2, j2 = chain(3, 9, 0.4, rng)
    n = 7
    pos = np.vstack([[[0, -0.5, 0]], B1.pos + (-2, 0, 0), B2.pos + (2, 0, 0)])
    quat = np.vstack([[[1, 0, 0, 0]], B1.quat, B2.quat])
    lv = np.vstack([[[0.1, 0.2, 0]], B1.lvel, B2.lvel]); av = np.vstack([[[0, 0.3, 0]], B1.avel, B2.avel])
    flags = np.full(n, ld.ALIVE, np.uint8); flags[0] |= ld.KINEMATIC
    B = ld.Bodies(pos, quat, lv, av, np.concatenate([[5.0], B1.mass, B2.mass]), np.vstack([[[1, 1, 1]], B1.inertia, B2.inertia]), flags)
    jj = np.concatenate([j1, j2])
    jj["body1"][:9] += 1; jj["body2"][:9] = np.where(j1["body2"] >= 0, j1["body2"] + 1, 0)
    jj["body1"][9:] += 4; jj["body2"][9:] = np.where(j2["body2"] >= 0, j2["body2"] + 4, 0)
    jj["pos"][:9] += (-2, 0, 0); jj["pos"][9:] += (2, 0, 0)
    for f in ("pos", "quat", "lvel", "avel", "mass", "inertia"):       # the state as the batch will hold it
        setattr(B, f, getattr(B, f).astype(prec).astype(np.float64))
    assert np.sum(jj["body2"] == 0) == 6
    return B, jj


def _kinematic_body_shared_by_two_stacks(prec, stepper):
    B, jj = kinematic_case(prec)
    n = B.n
    (r, _), = check(prec, B, world(prec), jj, stepper)
    (I,) = [I for I in r.islands if 0 in I.slots]
    assert sorted(I.slots) == list(range(n)) and np.any(I.J[:, :6] != 0)      # one island, through the slab's rows
    assert np.array_equal(r.device[0, 7:13], np.concatenate([B.lvel[0], B.avel[0]]))
    # apart: each stack on a static slab moving the same way gives the same velocities
    Wr, jr = as_precision(prec, world(prec), jj[:9])
    apart = ld.step(B, Wr, jr, stepper).bodies.lvel[1:4]
    assert np.max(np.abs(apart - r.bodies.lvel[1:4])) <= 1e-8 * ld.velocity_scale(r.bodies, world(prec))


@pytest.mark.parametrize("prec", PRECS)
def test_kinematic_body_shared_by_two_stacks(prec):
    """a kinematic slab carries two stacks: its velocity does not change, and the exact answer equals that of the two
    stacks solved apart (the kinematic body decouples them)"""
    _kinematic_body_shared_by_two_stacks(prec, "exact")


@pytest.mark.parametrize("prec", PRECS)
def test_kinematic_body_shared_by_two_stacks_quickstep(prec):
    """the same under QuickStep: the slab's rows couple nothing, so the sweeps over one stack alone give the same velocities"""
    _kinematic_body_shared_by_two_stacks(prec, "quick")


def mass_ratio_case(gyro):
    rng = np.random.default_rng(31 + gyro)
    B, jts = chain(6, 18, 0.5, rng, speed=1.0)
    B.mass[:] = [1e-3, 1.0, 1e3, 0.1, 10.0, 1.0]
    B.inertia *= B.mass[:, None]
    B.flags[1] |= ld.NOGRAVITY
    B.flags[3] |= ld.NOGYRO
    return B, jts


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("gyro", [ld.GYRO_OFF, ld.GYRO_EXPLICIT, ld.GYRO_IMPLICIT])
def test_bodies_mass_ratios_nogravity_gyro(prec, gyro):
    """mass ratios 1e-3 .. 1e3, rotated anisotropic inertia, NOGRAVITY and NOGYRO bodies, each gyro mode.  Regression: the
    scenes of GYRO_OFF and GYRO_EXPLICIT made the one-workgroup exact solve cycle -- block flips undoing Murty's single
    flips -- until its round limit, velocities ~1e5 off (csrc/dmx_lcp.hip lds_pivot_rounds)"""
    B, jts = mass_ratio_case(gyro)
    check(prec, B, world(prec, gyro=gyro), jts, "exact")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("gyro", [ld.GYRO_OFF, ld.GYRO_EXPLICIT, ld.GYRO_IMPLICIT])
def test_bodies_mass_ratios_nogravity_gyro_quickstep(prec, gyro):
    """the same scenes under QuickStep (float64 1e-10; float32 the band: with impulses that cancel across mass ratios of 1e6
    the band's M_v, not the velocities that are left, is the size rounding acts on)"""
    B, jts = mass_ratio_case(gyro)
    check(prec, B, world(prec, gyro=gyro), jts, "quick")


@pytest.mark.parametrize("prec", PRECS)
def test_degenerate_contacts(prec):
    """the same contact twice and four coplanar contacts: velocities only (lambda is ill-conditioned here), 1e-6 in
    float64 -- cfm / h = 6e-9 bounds A's conditioning"""
    B = ld.Bodies([[0, 0.5, 0]], [[1, 0, 0, 0]], [[0.2, -0.5, 0]], [[0, 0, 0]], [1.0], [[0.3, 0.3, 0.4]])
    corners = [((dx, 0.0, dz), (0, 1, 0), 0.01, 0, -1, 0, 0.5, 0, 0, 0, 0) for dx, dz in ((-.5, -.5), (.5, -.5), (.5, .5), (-.5, .5))]
    jts = np.array(corners + corners[:1], ld.JOINT_DTYPE)
    check(prec, B, world(prec), jts, "exact", tol=1e-6 if prec == "float64" else None)


# ---------------------------------------------------------------------------------------------------------------------
# i. warm start, j. mixed islands
@pytest.mark.parametrize("prec", PRECS)
def test_warm_start_against_the_memoryless_reference(prec):
    """twenty ticks of a resting stack, the joint list permuted and some contacts' mu switched between inf and 0.5 between
    ticks: every tick equals the reference restarted from the device's state (the grid solve carries active sets)"""
    rng = np.random.default_rng(41)
    B, jts = chain(15, 60, np.inf, rng, speed=0.05)

    def between(t, j):
        j = j[np.random.default_rng(t).permutation(len(j))].copy()
        flip = np.random.default_rng(100 + t).random(len(j)) < 0.3
        j["mu"] = np.where(flip, 0.5, np.inf)
        return j

    check(prec, B, world(prec), jts, "exact", ticks=20, between=between)


def mixed_islands_case():
    rng = np.random.default_rng(51)
    parts = [chain(1, 4, np.inf, rng), chain(1, 3, 0.5, rng), chain(5, 20, 0.4, rng), chain(80, 320, np.inf, rng)]
    Bs, js, off = [], [], 0
    for k, (B, j) in enumerate(parts):
        B.pos[:, 0] += 10.0 * k
        j = j.copy(); j["pos"][:, 0] += 10.0 * k
        j["body1"] += off; j["body2"] = np.where(j["body2"] >= 0, j["body2"] + off, -1)
        Bs.append(B); js.append(j); off += B.n
    B = ld.Bodies(*[np.vstack([getattr(b, f) for b in Bs]) for f in ("pos", "quat", "lvel", "avel")],
                  np.concatenate([b.mass for b in Bs]), np.vstack([b.inertia for b in Bs]))
    return B, np.concatenate(js)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stepper", ["quick", "exact"])
def test_mixed_islands_in_one_call(prec, stepper):
    """singles, LDS islands and a grid island (exact) in one call: every island matches"""
    B, jts = mixed_islands_case()
    (r, st), = check(prec, B, world(prec), jts, stepper)
    if stepper == "exact":
        assert st["solves"] == 1


# ---------------------------------------------------------------------------------------------------------------------
# every float32 QuickStep case of this file: name -> () -> (Bodies, World, joints), one tick each.  tests/test_quick_band.py
# runs the float32 emulation of the reference's sweeps over them (population (b) of quick_band.MEASURED)
F32_QUICK_CASES = {}
for _nc in (1, 2, 5, 8, 9):
    F32_QUICK_CASES[f"single-{_nc}"] = lambda nc=_nc: (*single_case(nc), world("float32"))
F32_QUICK_CASES["canonicalisation"] = lambda: (*canonicalisation_case(), world("float32"))
for _m in (256, 257, 1025, 3072, 3073):
    F32_QUICK_CASES[f"press_chain-{_m}"] = lambda m=_m: (*press_chain(m, np.random.default_rng(m)), world("float32"))
for _m in (255, 258, 1025, 3073):
    F32_QUICK_CASES[f"clamp_chain-{_m}"] = lambda m=_m: (*clamp_chain(m), world("float32"))
F32_QUICK_CASES["separating"] = lambda: (*separating_case(), world("float32", gravity=(0, 0, 0)))
for _s in sorted(SURFACES):
    F32_QUICK_CASES[f"surface-{_s}"] = lambda s=_s: (*_surface_case(11, **SURFACES[s]), world("float32"))
F32_QUICK_CASES["kinematic"] = lambda: (*kinematic_case("float32"), world("float32"))
for _g in (ld.GYRO_OFF, ld.GYRO_EXPLICIT, ld.GYRO_IMPLICIT):
    F32_QUICK_CASES[f"mass_ratios-gyro{_g}"] = lambda g=_g: (*mass_ratio_case(g), world("float32", gyro=g))
F32_QUICK_CASES["mixed_islands"] = lambda: (*mixed_islands_case(), world("float32"))


# ---------------------------------------------------------------------------------------------------------------------
# knobs, each in a child process (read once per process)
_CHILD = {
    "big16": ({"DMX_BIG_ISLAND_ROWS": "16"}, "test_quickstep_island_row_counts", ["float64", 30]),
    "big64": ({"DMX_BIG_ISLAND_ROWS": "64"}, "test_quickstep_island_row_counts", ["float64", 30]),
    "regs_wg256": ({"DMX_REGS_WG": "256"}, "test_quickstep_register_form_f32", [3072]),
    "regs_by_row": ({"DMX_REGS_BY_CONTACT": "0"}, "test_quickstep_register_form_f32", [1025]),
    "big64_f32_surface": ({"DMX_BIG_ISLAND_ROWS": "64"}, "child_lane_per_island_surface_f32", []),
    "regs_by_row_clamps": ({"DMX_REGS_BY_CONTACT": "0"}, "test_quickstep_forms_with_clamping_rows_f32", [1025]),
    "grid_rows_1_tiles": ({"DMX_LCP_GRID_ROWS": "1"}, "test_exact_grid_tiles", ["float64", 2, 1]),
    "grid_rows_1": ({"DMX_LCP_GRID_ROWS": "1"}, "test_exact_island_sizes", ["float64", 65, "mix"]),
    "lcp_warm0": ({"DMX_LCP_WARM": "0"}, "test_warm_start_against_the_memoryless_reference", ["float64"]),
    "lcp_level2_0": ({"DMX_LCP_LEVEL2": "0"}, "test_exact_one_large_island", ["float64"]),
    "lcp_murty": ({"DMX_LCP_MURTY": "1"}, "test_exact_one_large_island", ["float64"]),
}


def child_lane_per_island_surface_f32():
    """(run by test_knob_in_a_child_process under DMX_BIG_ISLAND_ROWS=64) the bounce_mixed surface case, one island of 28 rows on
    four bodies with rows that clamp, in float32 on the lane-per-island form (row_sor in solve_islands): csrc/dmx_joints.cpp gives
    an island a wavefront only from DMX_BIG_ISLAND_ROWS rows on, and four bodies are no solve_singles island; with the
    single-launch tick off the tick takes the general path, where that rule decides (asserted from the counters)"""
    threshold = int(os.environ["DMX_BIG_ISLAND_ROWS"])
    B, jts = _surface_case(11, **SURFACES["bounce_mixed"])
    (r, st), = check("float32", B, world("float32"), jts, "quick", small=B_.SMALL_TICK_OFF)
    (I,), (lam,) = r.islands, r.lams
    assert 8 < I.m < threshold and len(I.slots) > 1, "not an island the lane-per-island form takes"
    assert st["tick"]["small"] == 0 and st["tick"]["general"] == 1, st["tick"]
    fr = np.isfinite(I.hi)
    assert np.any(lam[I.row_kind == 0] == 0) and np.any((lam[fr] == I.hi[fr]) | (lam[fr] == I.lo[fr])), "no row of the case clamps"


@pytest.mark.parametrize("name", sorted(_CHILD))
def test_knob_in_a_child_process(name):
    env, fn, args = _CHILD[name]
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys, json; sys.path[:0] = [%r, %r]; import test_gpu_solver_dense as t; "
            "getattr(t, %r)(*json.loads(%r)); print('CHILD-OK')") % (here, os.path.dirname(here), fn, json.dumps(args))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env={**os.environ, **env})
    assert p.returncode == 0 and "CHILD-OK" in p.stdout, (p.stdout[-2000:] + p.stderr[-3000:])
