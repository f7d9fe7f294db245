"""The dense float64 restatement of a tick with articulation joints (tests/limot_dense.py and, through it, joint_dense.py and
lcp_dense.py) with slider and fixed joints added, written from the definitions in include/dmx_batch.h at DMX_JOINT_SLIDER.

Test infrastructure, not a test file.  Body stage, islands, the solvers and the integration are lcp_dense's; the ball and hinge rows
joint_dense's; the hinge's limot row and the five-line table limot_dense's.  New here, in canonical sides (body1 = -1 with a live
body2 exchanges the sides, anchors and axes included), k = erp / h, cfm = the world's:

  zero pose    q_0 = the joint's limot entry's qrel0 (the identity without limots); q_0c = q_0, or conj(q_0) after an exchange
  lock         (slider, fixed; three rows) e = conj(q_1) q_2 conj(q_0c), negated when e_w < 0; Phi = R_1 (2 e_v);
               d = e_x, e_y, e_z:  J = [ 0, d | 0, -d ],  c = k Phi . d
  linear       (slider; two rows) u = R_1 axis1, r = p, q of plane_space(u):  J = [ r, (p_2 - x_1) x r | -r, -(a_2 x r) ],
               c = k (p_2 - p_1) . r
  position     sides AS GIVEN: s = u . (p_1 - p_2), u = R_1 axis1 (a world side 1: its axis as given);
               s_dot = [ u, (p_2 - x_1) x u | -u, -(a_2 x u) ] . (v_1, w_1, v_2, w_2)
  slider limot present by the hinge's rule: one row with s_dot's Jacobian and limot_dense.row_values(s, ...)
  row order    slider: lock, linear, limot.  fixed: ball rows, lock.
"""
import numpy as np

import joint_dense as jd
import lcp_dense as ld
import limot_dense as lm

BALL, HINGE, SLIDER, FIXED = 1, 2, 3, 4
IDENT = lm.IDENT


def default_limots(n):
    """no stops, no motors, every zero pose the identity: what a set without limots means"""
    l = np.zeros(n, lm.LIMOT_DTYPE)
    l["lo_stop"], l["hi_stop"] = -np.inf, np.inf
    l["qrel0"] = IDENT
    return l


def sides_given(bodies, a):
    """-> (x1, a1, u, x2, a2) of the sides as given"""
    x1, a1, u = jd.side(bodies, int(a["body1"]), a["anchor1"], a["axis1"])
    x2, a2, _ = jd.side(bodies, int(a["body2"]), a["anchor2"], a["axis2"])
    return x1, a1, u, x2, a2


def position(bodies, a):
    x1, a1, u, x2, a2 = sides_given(bodies, a)
    return float(u @ ((x1 + a1) - (x2 + a2)))


def rate_blocks(bodies, a):
    """-> the two 6-blocks of s_dot's Jacobian for the sides as given (a world side's block multiplies nothing)"""
    x1, a1, u, x2, a2 = sides_given(bodies, a)
    return np.concatenate([u, np.cross((x2 + a2) - x1, u)]), np.concatenate([-u, -np.cross(a2, u)])


def rate(bodies, a):
    J1, J2 = rate_blocks(bodies, a)
    b1, b2 = int(a["body1"]), int(a["body2"])
    v = lambda s: np.concatenate([bodies.lvel[s], bodies.avel[s]]) if s >= 0 else np.zeros(6)
    return float(J1 @ v(b1) + J2 @ v(b2))


def positions(bodies, art):
    """-> (s [n], s_dot [n]): 0 for other kinds and inactive joints"""
    s, sd = np.zeros(len(art)), np.zeros(len(art))
    for (_, k), _, _, _ in jd.canonical_arts(bodies, art):
        if int(art[k]["kind"]) == SLIDER:
            s[k], sd[k] = position(bodies, art[k]), rate(bodies, art[k])
    return s, sd


def lock_error(bodies, b1, b2, q0c):
    """-> (2 e_v with e_w >= 0 in the frame of side 1, R_1)"""
    q1 = bodies.quat[b1] if b1 >= 0 else IDENT
    q2 = bodies.quat[b2] if b2 >= 0 else IDENT
    e = ld.quat_mul(ld.quat_mul(lm.qconj(q1), q2), lm.qconj(q0c))
    if e[0] < 0:
        e = -e
    return 2.0 * e[1:], ld.quat_to_R(q1)


def lock_rows(bodies, world, loc, nb, b1, b2, q0, swapped):
    ev2, R1 = lock_error(bodies, b1, b2, lm.qconj(q0) if swapped else np.asarray(q0))
    phi = R1 @ ev2
    k = world.erp / world.h
    rows, c = [], []
    for d in np.eye(3):
        J = np.zeros(6 * nb)
        J[6 * loc[b1] + 3:6 * loc[b1] + 6] = d
        if b2 >= 0:
            J[6 * loc[b2] + 3:6 * loc[b2] + 6] = -d
        rows.append(J)
        c.append(k * (phi @ d))
    return rows, c


def canonical_sides(bodies, b1, b2, a, swapped):
    f = ("anchor2", "axis2", "anchor1", "axis1") if swapped else ("anchor1", "axis1", "anchor2", "axis2")
    x1, a1, u = jd.side(bodies, b1, a[f[0]], a[f[1]])
    x2, a2, _ = jd.side(bodies, b2, a[f[2]], a[f[3]])
    return x1, a1, u, x2, a2


def linear_rows(bodies, world, loc, nb, b1, b2, a, swapped):
    x1, a1, u, x2, a2 = canonical_sides(bodies, b1, b2, a, swapped)
    p1, p2 = x1 + a1, x2 + a2
    k = world.erp / world.h
    rows, c = [], []
    for r in ld.plane_space(u):
        J = np.zeros(6 * nb)
        J[6 * loc[b1]:6 * loc[b1] + 6] = np.concatenate([r, np.cross(p2 - x1, r)])
        if b2 >= 0:
            J[6 * loc[b2]:6 * loc[b2] + 6] = np.concatenate([-r, -np.cross(a2, r)])
        rows.append(J)
        c.append(k * ((p2 - p1) @ r))
    return rows, c


def slimot_row(bodies, world, loc, nb, a, l):
    """-> (J, c, lo, hi, line, margin) of a present slider limot; the row is written for the sides as given, which puts each
    block where the canonical form has it"""
    J1, J2 = rate_blocks(bodies, a)
    J = np.zeros(6 * nb)
    for s, blk in ((int(a["body1"]), J1), (int(a["body2"]), J2)):
        if s >= 0:
            J[6 * loc[s]:6 * loc[s] + 6] = blk
    return (J,) + lm.row_values(position(bodies, a), l, world)


class Island(lm.Island):
    """limot_dense's island with the slider and fixed joints' rows; every articulation row is assembled here, the ball and hinge
    rows by joint_dense.joint_rows and limot_dense.limot_row"""

    def __init__(self, bodies, world, slots, members, jts, art, lim):
        ca = [c for c in members if isinstance(c[0], tuple)]
        cc = [c for c in members if not isinstance(c[0], tuple)]
        ld.Island.__init__(self, bodies, world, slots, cc, jts)
        self.n_art_rows = 0
        self.theta_margin = self.pos_margin = np.inf
        self.limot_rows, self.limot_lines = [], []
        if not ca:
            return
        loc = {s: k for k, s in enumerate(self.slots)}
        nb = len(self.slots)
        rows, c, lo, hi = [], [], [], []

        def add(rs, cs):
            rows.extend(rs)
            c.extend(cs)
            lo.extend([-np.inf] * len(cs))
            hi.extend([np.inf] * len(cs))

        def add_limot(J, cv, l_, h_, line, mg, which):
            self.limot_rows.append(len(rows))
            self.limot_lines.append(line)
            rows.append(J)
            c.append(cv)
            lo.append(l_)
            hi.append(h_)
            setattr(self, which, min(getattr(self, which), mg))

        for (_, k), b1, b2, swapped in ca:
            a, l, kind = art[k], lim[k], int(art[k]["kind"])
            if kind in (BALL, HINGE):
                add(*jd.joint_rows(bodies, world, loc, nb, b1, b2, a, swapped))
                if kind == HINGE and lm.present(l):
                    add_limot(*lm.limot_row(bodies, world, loc, nb, b1, b2, a, l, swapped), "theta_margin")
            elif kind == SLIDER:
                add(*lock_rows(bodies, world, loc, nb, b1, b2, l["qrel0"], swapped))
                add(*linear_rows(bodies, world, loc, nb, b1, b2, a, swapped))
                if lm.present(l):
                    add_limot(*slimot_row(bodies, world, loc, nb, a, l), "pos_margin")
            elif kind == FIXED:
                r, cv = jd.joint_rows(bodies, world, loc, nb, b1, b2, a, swapped)
                add(r[:3], cv[:3])
                add(*lock_rows(bodies, world, loc, nb, b1, b2, l["qrel0"], swapped))
            else:
                raise ValueError(f"joint kind {kind}")
        na = len(rows)
        self.n_art_rows = na
        self.J = np.vstack([np.array(rows).reshape(na, 6 * nb), self.J.reshape(-1, 6 * nb)])
        self.c = np.concatenate([c, self.c])
        self.cfm = np.concatenate([np.full(na, world.cfm), self.cfm])
        self.lo = np.concatenate([lo, self.lo])
        self.hi = np.concatenate([hi, self.hi])
        self.row_joint = np.concatenate([np.full(na, -1, int), self.row_joint])
        self.row_kind = np.concatenate([np.full(na, -1, int), self.row_kind])
        self.m = len(self.c)
        h = self.h
        self.A = self.J @ self.minv(self.J.T) + np.diag(self.cfm / h)
        self.b = self.c / h - self.J @ (self.v / h + self.minv(self.f))
        self.nu = int(np.sum(np.isinf(self.lo) & np.isinf(self.hi)))
        self.nbd = self.m - self.nu


def step(bodies, world, jts, art=None, lim=None, stepper="quick"):
    """one tick with contact joints `jts`, articulation joints `art` of all four kinds and their limots `lim` (one per joint, or
    None) -> lcp_dense.Result; its islands carry theta_margin, pos_margin, limot_rows and limot_lines"""
    if art is None or len(art) == 0:
        return ld.step(bodies, world, jts, stepper)
    if lim is None or len(lim) == 0:
        lim = default_limots(len(art))
    assert len(lim) == len(art)
    jts = np.asarray(jts, ld.JOINT_DTYPE) if len(jts) else np.zeros(0, ld.JOINT_DTYPE)
    members = jd.canonical_arts(bodies, art) + ld.canonical(bodies, jts)
    out = bodies.copy()
    isl, lams, infos, margins = [], [], [], []
    h = world.h
    for slots, ms in ld.islands(bodies, members):
        I = Island(bodies, world, slots, ms, jts, art, lim)
        if stepper == "quick":
            lam, margin = I.quickstep(world.iters, world.sor_w)
            info = {}
        else:
            lam, info = I.exact()
            margin = None
        v = I.velocities(lam)
        for k, s in enumerate(slots):
            if bodies.flags[s] & ld.KINEMATIC:
                lv, av = bodies.lvel[s], bodies.avel[s]
            else:
                lv, av = v[6 * k:6 * k + 3], v[6 * k + 3:6 * k + 6]
            out.lvel[s], out.avel[s] = lv, av
            out.pos[s] = bodies.pos[s] + h * lv
            q = bodies.quat[s] + 0.5 * h * ld.quat_mul(np.concatenate([[0.0], av]), bodies.quat[s])
            out.quat[s] = q / np.linalg.norm(q)
        isl.append(I)
        lams.append(lam)
        infos.append(info)
        margins.append(margin)
    return ld.Result(out, isl, lams, infos, margins)


def pos_margin(result):
    """the least distance of a limited, unlocked slider from its nearer stop, in metres"""
    return min([getattr(I, "pos_margin", np.inf) for I in result.islands] + [np.inf])


def errors(bodies, art, lim=None):
    """-> (pos_err [n], axis_err [n]) as dmxBatchJointErrors defines them for all four kinds"""
    pe, ae = jd.errors(bodies, art)
    if lim is None or len(lim) == 0:
        lim = default_limots(len(art))
    for (_, k), b1, b2, swapped in jd.canonical_arts(bodies, art):
        a, kind = art[k], int(art[k]["kind"])
        if kind not in (SLIDER, FIXED):
            continue
        x1, a1, u, x2, a2 = canonical_sides(bodies, b1, b2, a, swapped)
        d = (x2 + a2) - (x1 + a1)
        if kind == SLIDER:
            d = d - (d @ u) * u
        pe[k] = np.linalg.norm(d)
        ae[k] = np.linalg.norm(lock_error(bodies, b1, b2, lm.qconj(lim[k]["qrel0"]) if swapped else lim[k]["qrel0"])[0])
    return pe, ae


# ---------------------------------------------------------------------------------------------------------------------
# scenes shared by the CPU and GPU tests.  Everything stays within a few metres of the origin.
MODES, MODE_LINES, set_mode, limots = lm.MODES, lm.MODE_LINES, lm.set_mode, lm.limots


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def one_body(mode, swapped=False, seed=3, kind=SLIDER, at=(0.4, 1.0, -0.2)):
    """one body on a slider (its current pose s = 0 and the zero pose) or welded to the world, given as (body, world) or as
    (world, body); mode: an entry of MODES read in metres, m/s and N, or None.  `low_stop_leaving` moves along the axis at 3"""
    rng = np.random.default_rng(seed)
    B = ld.Bodies([at], [_unit(rng.normal(size=4))], [[0.2, -0.1, 0.3]], [[0.5, 1.5, -0.7]], [1.3], [[0.4, 0.7, 0.9]])
    sides = (-1, 0) if swapped else (0, -1)
    art = np.array([jd.from_world(B, kind, sides[0], sides[1], np.asarray(at) + (0.1, 0.3, 0.0), (0.2, 1.0, 0.1))], jd.ART_DTYPE)
    lim = limots(B, art)
    if mode is not None:
        set_mode(lim[0], mode)
    if mode == "low_stop_leaving":
        B.lvel[0] = 3.0 * lm.axis_world(B, art[0]) * (-1.0 if swapped else 1.0)
    return B, art, lim


def merge(parts, dx=1.0):
    """worlds side by side along x, dx apart: bodies renumbered, world-side anchors moved with them"""
    off, Bs, arts, lims = 0, [], [], []
    for k, (B, art, lim) in enumerate(parts):
        shift = np.array([dx * k, 0.0, 0.0])
        B = B.copy()
        B.pos = B.pos + shift
        art = art.copy()
        for side, anchor in (("body1", "anchor1"), ("body2", "anchor2")):
            w = art[side] < 0
            art[anchor][w] += shift
            art[side][~w] += off
        off += B.n
        Bs.append(B)
        arts.append(art)
        lims.append(lim)
    B = ld.Bodies(np.vstack([b.pos for b in Bs]), np.vstack([b.quat for b in Bs]), np.vstack([b.lvel for b in Bs]),
                  np.vstack([b.avel for b in Bs]), np.concatenate([b.mass for b in Bs]), np.vstack([b.inertia for b in Bs]),
                  np.concatenate([b.flags for b in Bs]))
    return B, np.concatenate(arts), np.concatenate(lims)


def one_body_per_mode(swapped, seed=3):
    """one body on a slider to the world per entry of MODES, each its own island, 0.5 apart"""
    return merge([one_body(mode, swapped, seed + k, at=(-2.5, 1.0, -0.2)) for k, mode in enumerate(MODES)], dx=0.5)


def two_bodies(kind, mode=None, kinematic=True, seed=5):
    rng = np.random.default_rng(seed)
    quat = rng.normal(size=(2, 4))
    quat /= np.linalg.norm(quat, axis=1)[:, None]
    B = ld.Bodies([[0.0, 2.0, 0.0], [1.0, 2.2, 0.1]], quat, rng.normal(scale=0.4, size=(2, 3)), rng.normal(scale=0.4, size=(2, 3)),
                  [1.0, 1.7], rng.uniform(0.3, 1.0, (2, 3)))
    if kinematic:
        B.flags[0] |= ld.KINEMATIC
        B.lvel[0], B.avel[0] = (0.5, 0.2, -0.3), (0.0, 1.0, 0.5)
    art = np.array([jd.from_world(B, kind, 0, 1, (0.5, 2.1, 0.0), (0.3, 0.2, 1.0))], jd.ART_DTYPE)
    lim = limots(B, art)
    if mode is not None:
        set_mode(lim[0], mode)
    return B, art, lim


def cart_pole(vel=1.5, fmax=40.0, lean=0.2, at=(0.0, 1.0, 0.0)):
    """a cart of mass 2 on a rail along x (a slider to the world with a motor) and a pole of mass 0.5 and length 1 on a hinge
    about z at the cart's centre, leaning by `lean`"""
    at = np.asarray(at, np.float64)
    q = np.array([np.cos(0.5 * lean), 0.0, 0.0, -np.sin(0.5 * lean)])
    top = at + 0.5 * np.array([np.sin(lean), np.cos(lean), 0.0])
    B = ld.Bodies([at, top], [IDENT, q], [[0.3, 0, 0], [0.3, 0, 0]], np.zeros((2, 3)), [2.0, 0.5], [[0.3, 0.4, 0.3], [0.05, 0.01, 0.05]])
    art = np.array([jd.from_world(B, SLIDER, 0, -1, at, (1.0, 0.0, 0.0)), jd.from_world(B, HINGE, 1, 0, at, (0.0, 0.0, 1.0))], jd.ART_DTYPE)
    lim = limots(B, art)
    set_mode(lim[0], (-2.0, 2.0, vel, fmax))
    return B, art, lim


def all_kinds_chain(seed=11):
    """five bodies in one island: world -slider- 0 -hinge- 1 -ball- 2 -fixed- 3 -slider- 4, random poses and velocities, the
    first slider motorised, the second at its low stop, the hinge with a weak motor"""
    rng = np.random.default_rng(seed)
    n = 5
    quat = rng.normal(size=(n, 4))
    quat /= np.linalg.norm(quat, axis=1)[:, None]
    pos = np.column_stack([0.8 * np.arange(n) - 1.6, np.full(n, 1.5), 0.2 * rng.normal(size=n)])
    B = ld.Bodies(pos, quat, rng.normal(scale=0.3, size=(n, 3)), rng.normal(scale=0.3, size=(n, 3)), rng.uniform(0.5, 2.0, n),
                  rng.uniform(0.3, 1.0, (n, 3)))
    mid = lambda a, b: 0.5 * (B.pos[a] + B.pos[b])
    art = np.array([jd.from_world(B, SLIDER, 0, -1, B.pos[0], rng.normal(size=3)),
                    jd.from_world(B, HINGE, 1, 0, mid(0, 1), rng.normal(size=3)),
                    jd.from_world(B, BALL, 2, 1, mid(1, 2)),
                    jd.from_world(B, FIXED, 3, 2, mid(2, 3)),
                    jd.from_world(B, SLIDER, 3, 4, mid(3, 4), rng.normal(size=3))], jd.ART_DTYPE)
    lim = limots(B, art)
    set_mode(lim[0], (-np.inf, np.inf, 1.0, 30.0))
    set_mode(lim[1], (-np.inf, np.inf, -2.0, 0.05))
    set_mode(lim[4], (0.05, 0.5, 0.0, 0.0))
    return B, art, lim


def mixed_chain(rows, seed=0, contacts=False):
    """joint_dense's slowly converging chain over all four kinds -- hinge with a limot, ball, slider with a limot, fixed, plain
    hinge, plain slider in turn -- whose one island has exactly `rows` rows; the limots cycle through MODES (every line of the
    table, in radians on the hinges and metres on the sliders), their zero poses the poses the joints were made at, then every
    body is disturbed: |theta| <= 4e-3 rad, |s| a few 1e-3 m, 0.006 or more from every stop at the sizes the tests use (the GPU
    files assert 1e-3 per tick).
    contacts: every eighth body also has a ground contact under it -- mu cycling through 0.5, inf and 0, every other one with
    bounce -- and moves down or up in turn, so that normal rows end loaded and at 0 and friction rows at their bounds; the
    contacts' rows count towards `rows`"""
    cycle = [(HINGE, 6), (BALL, 3), (SLIDER, 6), (FIXED, 6), (HINGE, 5), (SLIDER, 5)]
    mus, reserve = [], 0
    if contacts:
        nb = rows // 6                                     # (fewer bodies than the plan will have: it averages 5.2 rows a joint)
        mus = [(0.5, np.inf, 0.0)[c % 3] for c in range(nb // 8)]
        reserve = sum(3 if mu > 0 else 1 for mu in mus)
    plan = jd.plan_rows(rows, cycle, reserve)
    B, art = jd.chain([k for k, _ in plan], seed)
    lim = limots(B, art)
    names = list(MODES)
    for n, k in enumerate(k for k, (_, r) in enumerate(plan) if r == 6 and plan[k][0] != FIXED):
        set_mode(lim[k], names[n % len(names)])
    jd.disturb(B, seed)
    jts = []
    for c, mu in enumerate(mus):
        s = 8 * c + 3
        B.lvel[s] = (0.3, -1.0 if c % 4 != 3 else 1.0, 0.2)
        nrm = _unit((0.1 * (c % 3 - 1), 1.0, 0.15 * (c % 2)))
        jts.append((B.pos[s] + (0.0, -0.5, 0.0), nrm, 0.01, s, -1, ld.CONTACT_BOUNCE if c % 2 else 0, mu, 0.7, 0.05, 0, 0))
    return B, art, lim, np.array(jts, ld.JOINT_DTYPE) if jts else np.zeros(0, ld.JOINT_DTYPE)


def star(n, seed=0, contacts=False):
    """joint_dense's star round a heavy hub, the spokes on sliders along random axes (k % 3 != 2) and welds (k % 3 == 2), given
    as (spoke, hub) and every fourth as (hub, spoke); the sliders' limots cycle through free motor, at the low stop, at the high
    stop with a weak motor, inside, and saturated motor.  contacts: four frictionless ground contacts under the hub"""
    B, _ = jd.star(n, seed=seed)
    rng = np.random.default_rng(seed + 200)
    art = []
    for k in range(n):
        sides = (0, k + 1) if k % 4 == 3 else (k + 1, 0)
        art.append(jd.from_world(B, FIXED if k % 3 == 2 else SLIDER, sides[0], sides[1], B.pos[0] + 0.5 * (B.pos[k + 1] - B.pos[0]), rng.normal(size=3)))
    art = np.array(art, jd.ART_DTYPE)
    B.avel[:] = rng.normal(scale=0.5, size=B.avel.shape)
    lim = limots(B, art)
    ns = 0
    for k in range(n):
        if art[k]["kind"] != SLIDER:
            continue
        m, ns = ns % 5, ns + 1
        if m == 0:
            set_mode(lim[k], (-np.inf, np.inf, rng.normal(), 20.0))
        if m == 1:
            set_mode(lim[k], (0.05, 0.5, 0.0, 0.0))
        if m == 2:
            set_mode(lim[k], (-0.5, -0.05, -0.5, 0.3))
        if m == 3:
            set_mode(lim[k], (-0.5, 0.5, 0.0, 0.0))
        if m == 4:
            set_mode(lim[k], (-np.inf, np.inf, 3.0 * rng.normal(), 0.02))
    jts = np.zeros(0, ld.JOINT_DTYPE)
    if contacts:
        B.lvel[0] = (0.0, -1.0, 0.0)
        pts = [(2.0, -0.5, 0.0), (0.0, -0.5, 2.0), (-2.0, -0.5, 0.0), (0.0, -0.5, -2.0)]
        nrm = np.array([(0.5, 1.0, 0.0), (0.0, 1.0, 0.5), (0.0, 1.0, 0.5), (0.5, 1.0, 0.0)])
        nrm /= np.linalg.norm(nrm, axis=1)[:, None]
        jts = np.array([(B.pos[0] + p, n_, 0.01, 0, -1, 0, 0.0, 0, 0, 0, 0) for p, n_ in zip(pts, nrm)], ld.JOINT_DTYPE)
    return B, art, lim, jts


def star_rows(art, lim):
    """-> (rows, rows that can clamp) of a star's one island"""
    sl = art["kind"] == SLIDER
    nl = sum(1 for a, l in zip(art, lim) if a["kind"] == SLIDER and lm.present(l))
    return int(5 * sl.sum() + 6 * (~sl).sum() + nl), nl


def slider_star(n, seed=0, hub_spin=2.0):
    """the star with a motorised slider on every spoke (the grid solve's carried active set, the timing scenes).  The hub turns at
    hub_spin about y: c = k Phi and c = k (p_2 - p_1) . r carry k = erp / h = 12 times a few float32 roundings of unit-sized numbers
    whatever the velocities are, some 4e-6, and the float32 tolerance is relative to the largest velocity -- a scene whose
    velocities are all small would be compared against less than that"""
    B, _ = jd.star(n, seed=seed)
    rng = np.random.default_rng(seed + 300)
    art = np.array([jd.from_world(B, SLIDER, k + 1, 0, B.pos[0] + 0.5 * (B.pos[k + 1] - B.pos[0]), rng.normal(size=3)) for k in range(n)],
                   jd.ART_DTYPE)
    B.avel[:] = rng.normal(scale=0.5, size=B.avel.shape)
    B.avel[0] = (0.0, hub_spin, 0.0)
    lim = limots(B, art)
    for k in range(n):
        set_mode(lim[k], (-np.inf, np.inf, rng.normal(), 20.0))
    return B, art, lim


def small_world(seed=13):
    """48 bodies within a few metres: 12 cart-poles on rails along x, 8 welded pairs hanging from the world on a slider, 4 bodies
    on ground contacts and 4 free bodies"""
    rng = np.random.default_rng(seed)
    parts = []
    for p in range(12):
        parts.append(cart_pole(vel=rng.normal(), fmax=(40.0, 0.05, 5.0)[p % 3], lean=0.3 * rng.normal(),
                               at=(-2.0 + 0.35 * p, 1.0 + 0.1 * (p % 4), -1.5 + 0.25 * p)))
    names = list(MODES)
    for d in range(8):
        B, art, lim = two_bodies(FIXED, kinematic=False, seed=seed + d)
        B.pos = B.pos * 0.5 + (-2.0 + 0.5 * d, 1.0, 1.5)
        art = np.array([jd.from_world(B, FIXED, 0, 1, 0.5 * (B.pos[0] + B.pos[1])),
                        jd.from_world(B, SLIDER, -1 if d % 2 else 0, 0 if d % 2 else -1, B.pos[0], rng.normal(size=3))], jd.ART_DTYPE)
        lim = limots(B, art)
        set_mode(lim[1], names[(d + 3) % len(names)])
        parts.append((B, art, lim))
    quat = rng.normal(size=(8, 4))
    quat /= np.linalg.norm(quat, axis=1)[:, None]
    free = ld.Bodies(np.column_stack([-2.0 + 0.5 * np.arange(8), np.full(8, 2.5), np.full(8, -2.0)]), quat, rng.normal(scale=0.3, size=(8, 3)),
                     rng.normal(scale=0.3, size=(8, 3)), rng.uniform(0.5, 2.0, 8), rng.uniform(0.3, 1.0, (8, 3)))
    parts.append((free, np.zeros(0, jd.ART_DTYPE), np.zeros(0, lm.LIMOT_DTYPE)))
    B, art, lim = merge(parts, dx=0.0)
    jts = []
    for s in range(B.n - 4, B.n):
        B.lvel[s] = (0.1, -1.0, 0.0)
        for c in range(1 + s % 3):
            nrm = np.array([0.4 * c, 1.0, 0.3 * (c - 1) * c])
            jts.append((B.pos[s] + (0.3 * c, -0.5, 0.2 * c), nrm / np.linalg.norm(nrm), 0.01, s, -1, 0, 0.0 if c else np.inf, 0, 0, 0, 0))
    return B, art, lim, np.array(jts, ld.JOINT_DTYPE)


def weld_chain(n=5):
    """n unit bodies welded in a row along +x, link 0 welded to the world at the origin: a cantilever under gravity"""
    B, ball = jd.hanging_chain(n, horizontal=True)
    art = ball.copy()
    art["kind"] = FIXED
    return B, art, limots(B, art)


def random_joints(n=1000, nb=64, seed=17):
    """n joints of all four kinds between nb bodies with random poses and velocities within a few metres: some inactive, some given
    as (world, body), random zero poses"""
    rng = np.random.default_rng(seed)
    quat = rng.normal(size=(nb, 4))
    quat /= np.linalg.norm(quat, axis=1)[:, None]
    B = ld.Bodies(rng.normal(scale=1.5, size=(nb, 3)), quat, rng.normal(size=(nb, 3)), rng.normal(scale=2.0, size=(nb, 3)), np.ones(nb), np.ones((nb, 3)))
    B.flags[5] = 0                                   # a dead slot: its joints are inactive
    art = jd.arts(n)
    lim = default_limots(n)
    for k in range(n):
        b1, b2 = (int(x) for x in rng.integers(0, nb, 2))
        form = k % 7
        if form == 1:
            b1 = -1                                  # (world, body)
        if form == 2:
            b2 = -1
        if form == 3 and k % 21 == 3:
            b1 = b2 = -1                             # inactive
        if form == 4 and k % 28 == 4:
            b2 = b1                                  # inactive
        art[k] = jd.from_world(B, (SLIDER, FIXED, SLIDER, HINGE, SLIDER, BALL)[k % 6], b1, b2, rng.normal(size=3), rng.normal(size=3))
        q0 = rng.normal(size=4)
        lim[k]["qrel0"] = q0 / np.linalg.norm(q0)
    return B, art, lim
