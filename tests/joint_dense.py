"""The dense float64 restatement of a tick (tests/lcp_dense.py) with ball and hinge joints added, written from the definitions
in include/dmx_batch.h at dmxBatchSetJoints.

Test infrastructure, not a test file.  Body stage, island union-find, projected SOR, the certified box LCP and the integration
are lcp_dense's own; this module adds the articulation joints' canonical form, their part in the island grouping and their rows:

  x_i, R_i = body i's position and rotation, a_i = R_i anchor_i; a world side has x = anchor, a = 0 and no Jacobian block;
  every row has lo = -inf, hi = +inf, cfm = the world's CFM; k = erp / h.
    ball   three rows, d = e_x, e_y, e_z:   J = [ d, a_1 x d | -d, -(a_2 x d) ],   c = k ((x_2 + a_2) - (x_1 + a_1)) . d
    hinge  the ball rows, then with u = R_1 axis1, w = R_2 axis2, (p, q) = plane_space(u), for r = p, q:
           J = [ 0, r | 0, -r ],   c = k (u x w) . r
  A joint is inactive when both sides are -1, when both sides are the same slot, or when a side >= 0 is not alive; body1 = -1
  with a live body2 exchanges the sides (anchors and axes included).  Within an island the active articulation joints come
  first, in the order of the set, then the contacts in creation order.

With no articulation joints `step` returns exactly what lcp_dense.step returns (the same code runs).
"""
import numpy as np

import lcp_dense as ld

BALL, HINGE = 1, 2
# the fields of dmxJoint (include/dmx_batch.h), in order; batch.JOINT_DTYPE is the C layout of the same
ART_FIELDS = [("kind", np.int32), ("body1", np.int32), ("body2", np.int32), ("reserved", np.int32), ("anchor1", np.float64, (3,)),
              ("anchor2", np.float64, (3,)), ("axis1", np.float64, (3,)), ("axis2", np.float64, (3,))]
ART_DTYPE = np.dtype(ART_FIELDS)


def arts(n, **fields):
    """a zeroed array of n articulation joints, fields set from keyword arguments"""
    a = np.zeros(n, ART_DTYPE)
    for k, v in fields.items():
        a[k] = v
    return a


def from_world(bodies, kind, b1, b2, anchor, axis=(0.0, 0.0, 0.0)):
    """the record of a joint given by a world-frame anchor and axis at the bodies' current poses"""
    a = np.zeros((), ART_DTYPE)
    a["kind"], a["body1"], a["body2"] = kind, b1, b2
    anchor, axis = np.asarray(anchor, np.float64), np.asarray(axis, np.float64)
    if np.linalg.norm(axis) > 0:
        axis = axis / np.linalg.norm(axis)
    for s, fa, fx in ((b1, "anchor1", "axis1"), (b2, "anchor2", "axis2")):
        if s < 0:
            a[fa], a[fx] = anchor, axis
        else:
            R = ld.quat_to_R(bodies.quat[s])
            a[fa], a[fx] = R.T @ (anchor - bodies.pos[s]), R.T @ axis
    return a


def canonical_arts(bodies, art):
    """-> list of (("art", index), b1, b2 or -1, swapped): the active joints, body1 a live slot"""
    live = lambda s: 0 <= s < bodies.n and bool(bodies.flags[s] & ld.ALIVE)
    out = []
    for k, a in enumerate(art):
        b1, b2 = int(a["body1"]), int(a["body2"])
        if (b1 < 0 and b2 < 0) or b1 == b2:
            continue
        if (b1 >= 0 and not live(b1)) or (b2 >= 0 and not live(b2)):
            continue
        swapped = b1 < 0
        if swapped:
            b1, b2 = b2, -1
        out.append((("art", k), b1, b2, swapped))
    return out


def side(bodies, s, anchor, axis):
    """-> (x, a, axis in the world frame) of one side of a joint"""
    if s < 0:
        return np.array(anchor, np.float64), np.zeros(3), np.array(axis, np.float64)
    R = ld.quat_to_R(bodies.quat[s])
    return bodies.pos[s], R @ anchor, R @ axis


def joint_rows(bodies, world, loc, nb, b1, b2, a, swapped):
    """-> (J rows, c) of one active joint in canonical form"""
    f = ("anchor2", "axis2", "anchor1", "axis1") if swapped else ("anchor1", "axis1", "anchor2", "axis2")
    x1, a1, u = side(bodies, b1, a[f[0]], a[f[1]])
    x2, a2, w = side(bodies, b2, a[f[2]], a[f[3]])
    k = world.erp / world.h
    rows, c = [], []
    err = (x2 + a2) - (x1 + a1)
    for d in np.eye(3):
        J = np.zeros(6 * nb)
        J[6 * loc[b1]:6 * loc[b1] + 6] = np.concatenate([d, np.cross(a1, d)])
        if b2 >= 0:
            J[6 * loc[b2]:6 * loc[b2] + 6] = np.concatenate([-d, -np.cross(a2, d)])
        rows.append(J)
        c.append(k * (err @ d))
    if int(a["kind"]) == HINGE:
        e = np.cross(u, w)
        for r in ld.plane_space(u):
            J = np.zeros(6 * nb)
            J[6 * loc[b1] + 3:6 * loc[b1] + 6] = r
            if b2 >= 0:
                J[6 * loc[b2] + 3:6 * loc[b2] + 6] = -r
            rows.append(J)
            c.append(k * (e @ r))
    return rows, c


class Island(ld.Island):
    """lcp_dense's island with the articulation joints' rows ahead of the contacts'"""

    def __init__(self, bodies, world, slots, members, jts, art):
        ca = [c for c in members if isinstance(c[0], tuple)]
        cc = [c for c in members if not isinstance(c[0], tuple)]
        super().__init__(bodies, world, slots, cc, jts)
        self.n_art_rows = 0
        if not ca:
            return
        loc = {s: k for k, s in enumerate(self.slots)}
        nb = len(self.slots)
        rows, c = [], []
        for (_, k), b1, b2, swapped in ca:
            r, cv = joint_rows(bodies, world, loc, nb, b1, b2, art[k], swapped)
            rows += r
            c += cv
        na = len(rows)
        self.n_art_rows = na
        self.J = np.vstack([np.array(rows).reshape(na, 6 * nb), self.J.reshape(-1, 6 * nb)])
        self.c = np.concatenate([c, self.c])
        self.cfm = np.concatenate([np.full(na, world.cfm), self.cfm])
        self.lo = np.concatenate([np.full(na, -np.inf), self.lo])
        self.hi = np.concatenate([np.full(na, np.inf), self.hi])
        self.row_joint = np.concatenate([np.full(na, -1, int), self.row_joint])
        self.row_kind = np.concatenate([np.full(na, -1, int), self.row_kind])
        self.m = len(self.c)
        h = self.h
        self.A = self.J @ self.minv(self.J.T) + np.diag(self.cfm / h)
        self.b = self.c / h - self.J @ (self.v / h + self.minv(self.f))
        self.nu = int(np.sum(np.isinf(self.lo) & np.isinf(self.hi)))
        self.nbd = self.m - self.nu


def step(bodies, world, jts, art=None, stepper="quick", order=None):
    """one tick with contact joints `jts` (lcp_dense.JOINT_DTYPE) and articulation joints `art` (ART_DTYPE) -> lcp_dense.Result"""
    if art is None or len(art) == 0:
        return ld.step(bodies, world, jts, stepper, order)
    jts = np.asarray(jts, ld.JOINT_DTYPE) if len(jts) else np.zeros(0, ld.JOINT_DTYPE)
    members = canonical_arts(bodies, art) + ld.canonical(bodies, jts)
    out = bodies.copy()
    isl, lams, infos, margins = [], [], [], []
    h = world.h
    for slots, ms in ld.islands(bodies, members):
        I = Island(bodies, world, slots, ms, jts, art)
        if stepper == "quick":
            lam, margin = I.quickstep(world.iters, world.sor_w, order)
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


def errors(bodies, art):
    """-> (pos_err [n], axis_err [n]): per joint |p2 - p1| and, for hinges, |u x w| (0 for balls and inactive joints)"""
    pe, ae = np.zeros(len(art)), np.zeros(len(art))
    for (_, k), b1, b2, swapped in canonical_arts(bodies, art):
        a = art[k]
        f = ("anchor2", "axis2", "anchor1", "axis1") if swapped else ("anchor1", "axis1", "anchor2", "axis2")
        x1, a1, u = side(bodies, b1, a[f[0]], a[f[1]])
        x2, a2, w = side(bodies, b2, a[f[2]], a[f[3]])
        pe[k] = np.linalg.norm((x2 + a2) - (x1 + a1))
        if int(a["kind"]) == HINGE:
            ae[k] = np.linalg.norm(np.cross(u, w))
    return pe, ae


# ---------------------------------------------------------------------------------------------------------------------
# scenes shared by the CPU and GPU tests
def hanging_chain(n, spacing=1.0, horizontal=False, mass=1.0, bend=0.0):
    """n unit bodies on ball joints, link 0 to the world at the origin: hanging down along -y, or stretched out along +x
    (released horizontally); the anchors sit where neighbouring links meet.  bend: the chain's direction turns by this angle
    in all from its first link to its last, in the xy plane (a straight chain pinned at both ends has a redundant row along
    its axis; a bent one has not)"""
    a0 = np.pi / 2 if horizontal else 0.0
    ang = a0 + bend * (np.arange(n) + 0.5) / n
    d = np.column_stack([np.sin(ang), -np.cos(ang), np.zeros(n)]) * spacing
    ends = np.vstack([np.zeros(3), np.cumsum(d, axis=0)])            # joint k sits at ends[k]
    pos = 0.5 * (ends[:-1] + ends[1:])
    B = ld.Bodies(pos, np.tile([1.0, 0, 0, 0], (n, 1)), np.zeros((n, 3)), np.zeros((n, 3)), np.full(n, mass), np.ones((n, 3)))
    art = np.array([from_world(B, BALL, k, k - 1, ends[k]) for k in range(n)], ART_DTYPE)
    return B, art


def plan_rows(rows, cycle, reserve=0):
    """-> a list of (kind, rows) joints whose row counts and `reserve` sum to exactly `rows`: the entries of `cycle` in turn (each
    a (kind, rows) pair; the kinds are dmxJoint's) while 8 or more rows remain, then a tail of balls (3 rows) and plain hinges (5),
    which make every count from 8 on"""
    plan, left, k = [], rows - reserve, 0
    while left - cycle[k % len(cycle)][1] >= 8:
        plan.append(cycle[k % len(cycle)])
        left -= plan[-1][1]
        k += 1
    hinges = next(j for j in range(left // 5 + 1) if (left - 5 * j) % 3 == 0)
    plan += [(HINGE, 5)] * hinges + [(BALL, 3)] * ((left - 5 * hinges) // 3)
    assert sum(r for _, r in plan) + reserve == rows
    return plan


def chain(kinds, seed, spacing=1.0, bend=2.0):
    """one body per entry of `kinds`, joint k of that kind between body k and body k - 1 (joint 0 to the world) where the two
    links meet; the chain starts at the origin and turns by `bend` in all in the xy plane (hanging_chain's layout).  Random
    rotations -- no R is exact in float32 --, velocities, masses and inertias, random axes.  The joints are made at these
    poses, so their errors are zero: take the zero poses of the limots, then `disturb`.  -> (Bodies, joints)"""
    rng = np.random.default_rng(seed)
    n = len(kinds)
    ang = bend * (np.arange(n) + 0.5) / n
    d = np.column_stack([np.sin(ang), -np.cos(ang), np.zeros(n)]) * spacing
    ends = np.vstack([np.zeros(3), np.cumsum(d, axis=0)])
    quat = rng.normal(size=(n, 4))
    quat /= np.linalg.norm(quat, axis=1)[:, None]
    B = ld.Bodies(0.5 * (ends[:-1] + ends[1:]), quat, rng.normal(scale=0.3, size=(n, 3)), rng.normal(scale=0.3, size=(n, 3)),
                  rng.uniform(0.5, 2.0, n), rng.uniform(0.3, 1.0, (n, 3)))
    art = np.array([from_world(B, kind, k, k - 1, ends[k], rng.normal(size=3)) for k, kind in enumerate(kinds)], ART_DTYPE)
    return B, art


def disturb(B, seed, dist=2e-3, turn=2e-3):
    """move every body by `dist` in a random direction and turn it by `turn` rad about a random axis, in place: every joint made
    before has a position error of about `dist` and an axis / lock error of about `turn` to correct"""
    rng = np.random.default_rng(seed + 1000)
    u = rng.normal(size=(B.n, 3))
    B.pos += dist * u / np.linalg.norm(u, axis=1)[:, None]
    u = rng.normal(size=(B.n, 3))
    u *= np.sin(0.5 * turn) / np.linalg.norm(u, axis=1)[:, None]
    for s in range(B.n):
        q = ld.quat_mul(np.concatenate([[np.cos(0.5 * turn)], u[s]]), B.quat[s])
        B.quat[s] = q / np.linalg.norm(q)
    return B


def ball_hinge_chain(rows, seed=0):
    """a chain of alternating ball and hinge joints whose one island has exactly `rows` rows, with errors to correct: slow to
    converge under QuickStep -- a sweep dropped, or another sor_w, moves its velocities by far more than float32 rounding does.
    (Errors of 5e-3 m: 1 % of ERP moves c by 1 % of (ERP / h) x the error, and the band allows K eps32 (ERP / h) (|a_1| + |a_2|)
    with arms of 0.5 -- at 2e-3 m that is 170 / K bands, too near the 10 asked for)"""
    B, art = chain([k for k, _ in plan_rows(rows, [(BALL, 3), (HINGE, 5)])], seed)
    return disturb(B, seed, dist=5e-3), art


def star(n, hub_mass=100.0, radius=2.0, seed=0):
    """n unit bodies ball-jointed to a hub (slot 0) of mass and inertia hub_mass, spread over a sphere of `radius` round it,
    the anchors midway; small random velocities"""
    rng = np.random.default_rng(seed)
    dirs = rng.normal(size=(n, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    hub = np.array([0.0, 3.0, 0.0])
    pos = np.vstack([hub, hub + radius * dirs])
    B = ld.Bodies(pos, np.tile([1.0, 0, 0, 0], (n + 1, 1)), rng.normal(scale=0.1, size=(n + 1, 3)),
                  rng.normal(scale=0.1, size=(n + 1, 3)), np.concatenate([[hub_mass], np.ones(n)]),
                  np.vstack([np.full(3, hub_mass), np.ones((n, 3))]))
    art = np.array([from_world(B, BALL, k + 1, 0, hub + 0.5 * radius * dirs[k]) for k in range(n)], ART_DTYPE)
    return B, art
