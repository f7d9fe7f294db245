"""Ray casts restated in numpy float64 from the definitions: what tests/test_gpu_raycast.py holds the device's dmxBatchRayCast
against, and what tests/test_ray_reference.py holds the T-precision primitives of csrc/dmx_ray.hpp against on the host.

No grid and no early outs: every ray is tested against every geom that can be seen (bodies whose bounding sphere the segment
misses by more than the band are left out of the pair lists -- a filter in float64 with the band's width to spare).

  ray      o + t d, 0 <= t <= length, d the given direction normalised (here in float64, from the T-valued input)
  hit      the smallest t at which the ray crosses the geom's surface; the normal is the outward unit normal there, negated when
           the origin is inside the solid.  An origin exactly on the surface counts as outside.
  sphere   the quadratic: near root from outside, far root from inside
  box      slab test in the box frame: entering face from outside, leaving face from inside, lowest axis on ties
  plane    n.x = d, from either side
  convex   the segment clipped against the face planes in the body frame: latest entering face from outside, earliest leaving
           face from inside, first face in array order on ties
  winner   smallest t; ties: plane, then static boxes in order, then bodies by slot

The band rule.  The device evaluates the same definitions in its precision T from the same T-valued inputs, so a decision that
a few roundings can move may fall either way.  tol = K_RAY eps_T M, M = max |coordinate| + hit distance + largest extent.  A ray
is IN THE BAND -- nothing is asserted about it but that the device's answer is well formed -- when
  * the runner-up's t lies within 2 tol of the winner's;
  * a geom that could precede the winner grazes: its surface-to-ray margin is within tol.  The margin of a geom is the smallest
    of: the distance of the ray's line from the sphere's silhouette (| |foot| - r |) or from the nearest edge of the box / hull
    (a miss: the line's distance; a hit: the hit point's -- where one face's normal turns into the next's), and the distance of the origin from the surface (where
    outside turns into inside);
  * a geom that could precede the winner is hit at an incidence cosine |n.d| below C_GRAZE.  This is the same graze in the
    only units that mean anything for a hit: an error delta normal to the surface moves the hit by delta / |n.d| along the ray,
    so a bound on |depth - ref| in units of eps M can only be stated from some incidence on.  C_GRAZE is fixed, not fitted;
  * a hit (of the unbounded ray) lies within tol of t = 0 or t = length.
Outside the band: ids equal, |depth - ref| <= tol, |pos - ref| <= tol, |normal - ref| <= K_N eps_T M / (smallest extent).

K_RAY and K_N: four times the largest deviation of the T = float32 primitives (tests/harness/ray_prims_harness.cpp: dmx_ray.hpp
compiled for the host with the product's flags) from this module, in units of eps M resp. eps M / extent, over 131 072 random
ray-geom pairs per class that are outside the band, rounded up to a power of two; test_ray_reference.py repeats the
measurement and asserts the margin.  Measured (seeds 8..11, float32; depth and pos in eps M, normal in eps M / extent):
  sphere  depth 3.46  pos 2.76  normal 5.54       box    depth 4.38  pos 3.09  normal 0.29
  plane   depth 4.87  pos 3.86  normal 0          convex depth 3.84  pos 3.06  normal 0.18
so K_RAY = 32 (4 x 4.87 = 19.5) and K_N = 32 (4 x 5.54 = 22.2).  The worst cases sit at the shallowest incidence admitted,
1 / 16: roughly 0.3 eps M of error normal to the surface, sixteen-fold along the ray.  (The same run in float64 against this
module -- float64 against float64, so both sides err -- gives up to 6.84 and 3.55: inside the constants as well.)
C_GRAZE = 1 / 16 is the trade between the two caps a scene has to keep: the share of hits below an incidence cosine c grows
like c^2 (0.4 % of hits at 1 / 16 -- the near-origin cap is 0.2 % of rays, about half of which hit), the deviation, hence K_RAY, like
1 / c, and 8 km out in float32 K_RAY = 32 already makes tol 3 cm.
"""
import numpy as np

GEOM_NONE, GEOM_SPHERE, GEOM_BOX, GEOM_CONVEX = 0, 1, 2, 3
RAY_MISS, RAY_PLANE = -1, -2
RAY_SPHERES, RAY_BOXES, RAY_CONVEX, RAY_STATIC, RAY_PLANE_BIT, RAY_ALL = 1, 2, 4, 8, 16, 31
K_RAY = 32.0           # measured 4.87 eps M (see above)
K_N = 32.0             # measured 5.54 eps M / extent
C_GRAZE = 1.0 / 16.0   # incidence cosine below which a hit counts as grazing
INF = np.inf


def quat_to_R(q):
    """ODE's dRfromQ, (n, 4) (w, x, y, z) -> (n, 3, 3); the quaternion is used as given"""
    q = np.asarray(q, np.float64)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    qq1, qq2, qq3 = 2 * x * x, 2 * y * y, 2 * z * z
    R = np.empty((q.shape[0], 3, 3))
    R[:, 0, 0] = 1 - qq2 - qq3; R[:, 0, 1] = 2 * (x * y - w * z); R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z); R[:, 1, 1] = 1 - qq1 - qq3; R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y); R[:, 2, 1] = 2 * (y * z + w * x); R[:, 2, 2] = 1 - qq1 - qq2
    return R


def normalize_plane(plane, dtype):
    """dmxBatchSetPlane's (a, b, c, d) as the library normalises it, in T (dmx_normalize_plane)"""
    T = np.dtype(dtype).type
    a, b, c, d = (T(v) for v in plane)
    l = a * a + b * b + c * c
    l = T(1) / np.sqrt(l)
    return np.array([a * l, b * l, c * l, d * l], np.float64)


def hull_edges(points, planes):
    """the hull's edges as vertex pairs (ne, 2, 3): two vertices that share two distinct face planes"""
    p = np.asarray(points, np.float64)
    pl = np.unique(np.round(np.asarray(planes, np.float64), 9), axis=0)
    on = np.abs(p @ pl[:, :3].T - pl[None, :, 3]) < 1e-7 * max(1.0, np.abs(p).max())          # (nv, nplanes)
    shared = (on[:, None, :] & on[None, :, :]).sum(2)
    a, b = np.nonzero(np.triu(shared >= 2, 1))
    return np.stack([p[a], p[b]], 1)


def rays_of(rays):
    """(n, 7) T-valued -> origin, unit direction (float64), length, valid"""
    r = np.asarray(rays, np.float64).reshape(-1, 7)
    o, d, L = r[:, 0:3], r[:, 3:6], r[:, 6]
    with np.errstate(all="ignore"):
        l = np.sqrt((d * d).sum(1))
        valid = np.isfinite(l) & (l > 0) & np.isfinite(L) & (L > 0) & np.isfinite(o).all(1)
        u = d / np.where(valid, l, 1.0)[:, None]
    return o, u, L, valid


def _reach(b, rb):
    """the t from which on a geom (bounding radius rb about its centre, b = (o - c).d) is within reach of the ray; inf when the
    whole geom lies behind the origin"""
    return np.where(-b + rb < 0, INF, np.maximum(-b - rb, 0.0))


class PairResult:
    """per ray-geom pair: t of the UNBOUNDED ray's hit (inf: none), the normal, the decision margin, the incidence cosine at the
    hit (1 for a miss), and the t from which on the geom is within reach of the ray"""

    def __init__(self, t, nrm, margin, cos, t_near):
        self.t, self.nrm, self.margin, self.cos, self.t_near = t, nrm, margin, cos, t_near


def _dot(a, b):
    return (a * b).sum(-1)


def pair_sphere(o, u, c, r):
    m = o - c
    b = _dot(m, u)
    q = m - b[:, None] * u
    perp = np.sqrt(_dot(q, q))
    mm = np.sqrt(_dot(m, m))
    disc = r * r - perp * perp
    ok = disc >= 0
    s = np.sqrt(np.where(ok, disc, 0.0))
    inside = mm < r
    t = np.where(inside, s - b, -b - s)
    hit = ok & (t >= 0)
    t = np.where(hit, t, INF)
    nrm = (m + np.where(hit, t, 0.0)[:, None] * u) / r[:, None] * np.where(inside, -1.0, 1.0)[:, None]
    margin = np.minimum(np.abs(perp - r), np.abs(mm - r))
    cos = np.where(hit, s / r, 1.0)
    return PairResult(t, np.where(hit[:, None], nrm, 0.0), margin, cos, _reach(b, r))


def _line_segment_distance(P, u, A, B):
    """distance of the line P + tau u (u a unit vector) from the segment A..B; arrays (..., 3)"""
    w, e = A - P, B - A
    wp = w - _dot(w, u)[..., None] * u
    ep = e - _dot(e, u)[..., None] * u
    ee = _dot(ep, ep)
    with np.errstate(all="ignore"):
        s = np.where(ee > 0, -_dot(wp, ep) / np.where(ee > 0, ee, 1.0), 0.0)
    s = np.clip(s, 0.0, 1.0)
    v = wp + s[..., None] * ep
    return np.sqrt(_dot(v, v))


def _point_segment_distance(P, A, B):
    e = B - A
    ee = _dot(e, e)
    s = np.clip(_dot(P - A, e) / np.where(ee > 0, ee, 1.0), 0.0, 1.0)
    v = A + s[..., None] * e - P
    return np.sqrt(_dot(v, v))


def _edge_margin(mo, md, t, hit, A, B):
    """a hit: the hit point's distance from the nearest edge (where one face's normal turns into the next's, and a hit into a
    miss); a miss: the line's distance from the nearest edge.  A, B (n, ne, 3)"""
    ph = mo + np.where(hit, t, 0.0)[:, None] * md
    return np.where(hit, _point_segment_distance(ph[:, None, :], A, B).min(1),
                    _line_segment_distance(mo[:, None, :], md[:, None, :], A, B).min(1))


_BOX_EDGES = None


def _box_edges():
    global _BOX_EDGES
    if _BOX_EDGES is None:
        e = []
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            for sb in (-1.0, 1.0):
                for s_c in (-1.0, 1.0):
                    A, B = np.zeros(3), np.zeros(3)
                    A[a], B[a] = -1.0, 1.0
                    A[b] = B[b] = sb
                    A[c] = B[c] = s_c
                    e.append((A, B))
        _BOX_EDGES = np.array(e)           # (12, 2, 3) in units of the half sides
    return _BOX_EDGES


def pair_box(o, u, c, R, sides):
    """R (n, 3, 3) body -> world"""
    m = o - c
    mo = np.einsum("nba,nb->na", R, m)
    md = np.einsum("nba,nb->na", R, u)
    h = 0.5 * sides
    n = o.shape[0]
    inside = (np.abs(mo) < h).all(1)
    with np.errstate(all="ignore"):
        t1 = (-h - mo) / md
        t2 = (h - mo) / md
    lo, hi = np.minimum(t1, t2), np.maximum(t1, t2)
    par = md == 0
    lo = np.where(par, -INF, lo); hi = np.where(par, INF, hi)
    out_par = (par & (np.abs(mo) > h)).any(1)
    a_in, a_out = np.argmax(lo, 1), np.argmin(hi, 1)          # (first index on ties)
    t_in, t_out = lo[np.arange(n), a_in], hi[np.arange(n), a_out]
    ok = (t_in <= t_out) & ~out_par
    t = np.where(inside, t_out, t_in)
    a = np.where(inside, a_out, a_in)
    hit = ok & (t >= 0) & np.isfinite(t)
    t = np.where(hit, t, INF)
    mda = md[np.arange(n), a]
    nrm = -np.sign(mda)[:, None] * R[np.arange(n), :, a]
    # margins: the line against the twelve edges, the origin against the surface
    E = _box_edges()[None] * h[:, None, None, :]                              # (n, 12, 2, 3)
    d_edge = _edge_margin(mo, md, t, hit, E[:, :, 0, :], E[:, :, 1, :])
    d_surf = np.where(inside, (h - np.abs(mo)).min(1), np.sqrt((np.maximum(np.abs(mo) - h, 0.0) ** 2).sum(1)))
    rb = np.sqrt(_dot(h, h))
    return PairResult(t, np.where(hit[:, None], nrm, 0.0), np.minimum(d_edge, d_surf), np.where(hit, np.abs(mda), 1.0),
                      _reach(_dot(m, u), rb))


def pair_plane(o, u, pn, pd):
    """pn (3,) unit normal, pd offset (the values the device holds)"""
    so = o @ pn - pd
    dn = u @ pn
    with np.errstate(all="ignore"):
        t = np.where(dn != 0, -so / np.where(dn != 0, dn, 1.0), INF)
    hit = (t >= 0) & np.isfinite(t)
    t = np.where(hit, t, INF)
    nrm = -np.sign(dn)[:, None] * pn[None, :]
    return PairResult(t, np.where(hit[:, None], nrm, 0.0), np.abs(so), np.where(hit, np.abs(dn), 1.0), np.zeros(len(o)))


def pair_convex(o, u, c, R, planes, edges, rb):
    """planes (nf, 4) and edges (ne, 2, 3) in the body frame (the values the device holds)"""
    n = o.shape[0]
    m = o - c
    mo = np.einsum("nba,nb->na", R, m)
    md = np.einsum("nba,nb->na", R, u)
    N, D = planes[:, :3], planes[:, 3]
    dist = mo @ N.T - D[None, :]                   # (n, nf)
    dn = md @ N.T
    inside = (dist < 0).all(1)
    par = dn == 0
    out_par = (par & (dist > 0)).any(1)
    with np.errstate(all="ignore"):
        tf = -dist / np.where(par, 1.0, dn)
    ent = np.where((dn < 0), tf, -INF)
    lea = np.where((dn > 0), tf, INF)
    f_in, f_out = np.argmax(ent, 1), np.argmin(lea, 1)
    t_in, t_out = ent[np.arange(n), f_in], lea[np.arange(n), f_out]
    ok = (t_in <= t_out) & ~out_par
    t = np.where(inside, t_out, t_in)
    f = np.where(inside, f_out, f_in)
    hit = ok & (t >= 0) & np.isfinite(t)
    t = np.where(hit, t, INF)
    nb = N[f] * np.where(inside, -1.0, 1.0)[:, None]
    nrm = np.einsum("nab,nb->na", R, nb)
    d_edge = _edge_margin(mo, md, t, hit, edges[None, :, 0, :], edges[None, :, 1, :])
    d_surf = np.abs(dist.max(1))                   # outside: a lower bound of the distance; inside: the distance
    return PairResult(t, np.where(hit[:, None], nrm, 0.0), np.minimum(d_edge, d_surf), np.where(hit, np.abs(dn[np.arange(n), f]), 1.0),
                      _reach(_dot(m, u), rb))


class Scene:
    """what the device holds: downloaded POS / QUAT / SIDES, classes, flags; the hull's planes and the static boxes rounded to the
    batch's precision as the library rounds them; the plane normalised as the library normalises it"""

    def __init__(self, dtype, pos, quat, sides, gtype, alive=None, hull_points=None, hull_planes=None, statics=(), plane=None):
        self.dtype = np.dtype(dtype)
        rd = lambda a: np.asarray(a, np.float64).astype(self.dtype).astype(np.float64)
        self.pos, self.quat, self.sides = (np.asarray(a, np.float64) for a in (pos, quat, sides))
        self.gtype = np.asarray(gtype)
        self.alive = np.ones(len(self.gtype), bool) if alive is None else np.asarray(alive, bool)
        self.planes = None if hull_planes is None else rd(hull_planes)
        self.edges = None if hull_planes is None else hull_edges(rd(hull_points), self.planes)
        self.statics = [(rd(s), rd(p), rd(R).reshape(3, 4)[:, :3]) for s, p, R in statics]
        self.plane = None if plane is None else normalize_plane(plane, self.dtype)

    def bound_radius(self):
        s = self.sides
        r = np.where(self.gtype == GEOM_BOX, 0.5 * np.sqrt((s * s).sum(1)), s[:, 0])
        return np.where(self.gtype == GEOM_NONE, 0.0, r)

    def extents(self):
        """(largest, smallest) extent of the geoms a ray can see"""
        g, s = self.gtype, self.sides
        ext = [np.array([1.0])] if not len(g) else []
        if (g == GEOM_BOX).any():
            ext.append(s[g == GEOM_BOX].ravel())
        if (g == GEOM_SPHERE).any():
            ext.append(2 * s[g == GEOM_SPHERE, 0])
        if (g == GEOM_CONVEX).any() and self.planes is not None:
            ext += [2 * s[g == GEOM_CONVEX, 0], 2 * np.abs(self.planes[:, 3])]
        for sd, _, _ in self.statics:
            ext.append(sd)
        e = np.concatenate(ext) if ext else np.array([1.0])
        return float(e.max()), float(e.min())

    def max_coordinate(self):
        m = float(np.abs(self.pos[self.gtype != GEOM_NONE]).max()) if (self.gtype != GEOM_NONE).any() else 0.0
        for _, p, _ in self.statics:
            m = max(m, float(np.abs(p).max()))
        return m


class CastResult:
    """ids, hit, valid; t / pos / normal of the reference's answer (a miss: the end point, zero normal, t = length); runner_t: the
    second smallest hit t (inf: none); tol, ntol: the ray's tolerances; band: is the ray in the band; pairs: the candidates'
    (ray, rank, t, margin, cos) records"""


def _rank_to_id(rank):
    return np.where(rank == 0, RAY_PLANE, np.where(rank <= 64, -3 - (rank - 1), rank - 65)).astype(np.int64)


def cast(scene, rays, mask=RAY_ALL, k_ray=K_RAY, k_n=K_N):
    o, u, L, valid = rays_of(rays)
    nr = len(o)
    eps = float(np.finfo(scene.dtype).eps)
    big, small = scene.extents()
    coord = scene.max_coordinate()
    # candidate records: ray index, rank, t, normal, margin, cos, t_near
    rec = []

    def add(idx, rank, pr):
        rec.append((idx, np.broadcast_to(rank, idx.shape).astype(np.int64), pr.t, pr.nrm, pr.margin, pr.cos, pr.t_near))

    allr = np.arange(nr)
    vr = allr[valid]
    if scene.plane is not None and (mask & RAY_PLANE_BIT) and len(vr):
        add(vr, 0, pair_plane(o[vr], u[vr], scene.plane[:3], scene.plane[3]))
    if mask & RAY_STATIC:
        for k, (sd, p, R) in enumerate(scene.statics):
            if len(vr):
                add(vr, 1 + k, pair_box(o[vr], u[vr], p[None, :], np.broadcast_to(R, (len(vr), 3, 3)), np.broadcast_to(sd, (len(vr), 3))))
    g = scene.gtype
    see = (g != GEOM_NONE) & scene.alive & (((mask >> (np.maximum(g.astype(np.int64), 1) - 1)) & 1) == 1)
    if scene.planes is None:
        see &= g != GEOM_CONVEX
    bodies = np.flatnonzero(see)
    rb = scene.bound_radius()
    slack = 4.0 * k_ray * eps * (coord + big + float(np.abs(o[valid]).max() if valid.any() else 0.0)) + 1e-9
    R_all = quat_to_R(scene.quat)
    for r0 in range(0, len(vr), 512):
        ri = vr[r0:r0 + 512]
        m = o[ri, None, :] - scene.pos[None, bodies, :]
        tc = np.clip(-(m * u[ri, None, :]).sum(2), 0.0, L[ri, None])
        q = m + tc[..., None] * u[ri, None, :]
        near = (q * q).sum(2) <= (rb[bodies][None, :] * (1 + 1e-9) + slack) ** 2
        a, b = np.nonzero(near)
        ia, jb = ri[a], bodies[b]
        for cls in (GEOM_SPHERE, GEOM_BOX, GEOM_CONVEX):
            k = g[jb] == cls
            if not k.any():
                continue
            i, j = ia[k], jb[k]
            if cls == GEOM_SPHERE:
                pr = pair_sphere(o[i], u[i], scene.pos[j], scene.sides[j, 0])
            elif cls == GEOM_BOX:
                pr = pair_box(o[i], u[i], scene.pos[j], R_all[j], scene.sides[j])
            else:
                pr = pair_convex(o[i], u[i], scene.pos[j], R_all[j], scene.planes, scene.edges, scene.sides[j, 0])
            add(i, 65 + j, pr)
    res = CastResult()
    res.valid = valid
    if rec:
        idx = np.concatenate([r[0] for r in rec]); rank = np.concatenate([r[1] for r in rec]); t = np.concatenate([r[2] for r in rec])
        nrm = np.concatenate([r[3] for r in rec]); margin = np.concatenate([r[4] for r in rec]); cos = np.concatenate([r[5] for r in rec])
        t_near = np.concatenate([r[6] for r in rec])
    else:
        idx = rank = np.zeros(0, np.int64); t = margin = cos = t_near = np.zeros(0); nrm = np.zeros((0, 3))
    t_seg = np.where(t <= L[idx], t, INF)                   # the hit of the segment
    order = np.lexsort((rank, t_seg, idx))
    idx_s, t_s, rank_s = idx[order], t_seg[order], rank[order]
    first = np.r_[True, idx_s[1:] != idx_s[:-1]] if len(idx_s) else np.zeros(0, bool)
    pos_first = np.flatnonzero(first)
    win_t = np.full(nr, INF); win_rank = np.full(nr, -1, np.int64); win_n = np.zeros((nr, 3)); run_t = np.full(nr, INF)
    win_t[idx_s[pos_first]] = t_s[pos_first]
    win_rank[idx_s[pos_first]] = rank_s[pos_first]
    win_n[idx_s[pos_first]] = nrm[order][pos_first]
    second = pos_first + 1
    ok2 = (second < len(idx_s))
    second = second[ok2]
    same = idx_s[second] == idx_s[pos_first[ok2]]
    run_t[idx_s[second[same]]] = t_s[second[same]]
    hit = np.isfinite(win_t)
    res.hit = hit & valid
    res.ids = np.where(res.hit, _rank_to_id(np.maximum(win_rank, 0)), RAY_MISS)
    res.t = np.where(valid, np.where(hit, win_t, L), 0.0)
    res.pos = np.where(valid[:, None], o + res.t[:, None] * u, 0.0)
    res.normal = np.where(res.hit[:, None], win_n, 0.0)
    res.runner_t = run_t
    M = np.maximum(coord, np.abs(np.where(valid[:, None], o, 0.0)).max(1)) + res.t + big
    with np.errstate(all="ignore"):
        res.tol = k_ray * eps * M
        res.ntol = k_n * eps * M / small
    # the band
    band = np.zeros(nr, bool)
    with np.errstate(invalid="ignore"):
        band |= hit & (run_t - win_t <= 2 * res.tol)
    reach = np.minimum(L, win_t)                                # nothing beyond the winner matters
    tol_c = res.tol[idx]
    could = (t_near <= reach[idx] + tol_c)
    flag = could & (margin <= tol_c)
    flag |= (t <= np.minimum(L[idx], win_t[idx] + 2 * tol_c) + tol_c) & (cos < C_GRAZE)
    flag |= np.isfinite(t) & (t <= win_t[idx] + 2 * tol_c) & ((t <= tol_c) | (np.abs(t - L[idx]) <= tol_c))
    np.logical_or.at(band, idx, flag)
    res.band = band & valid
    res.pairs = (idx, rank, t, margin, cos)
    return res


def compare(ref, ids, hits):
    """the device's (ids, hits) against a CastResult: -> (mismatch descriptions, worst depth / pos / normal deviation in units of
    the tolerances).  Rays in the band are only asked to be well formed."""
    ids = np.asarray(ids); hits = np.asarray(hits, np.float64)
    bad = []
    inv = ~ref.valid
    if inv.any() and not ((ids[inv] == RAY_MISS).all() and (hits[inv] == 0).all()):
        bad.append("an invalid ray did not give a miss and zeros")
    chk = ref.valid & ~ref.band
    wrong = chk & (ids != ref.ids)
    for i in np.flatnonzero(wrong)[:5]:
        bad.append(f"ray {i}: id {ids[i]} vs reference {ref.ids[i]} (t {hits[i, 6]!r} vs {ref.t[i]!r}, runner-up {ref.runner_t[i]!r}, tol {ref.tol[i]:.3g})")
    k = chk & ~wrong
    with np.errstate(all="ignore"):
        dd = np.abs(hits[k, 6] - ref.t[k]) / ref.tol[k]
        dp = np.abs(hits[k, 0:3] - ref.pos[k]).max(1) / ref.tol[k]
        dn = np.abs(hits[k, 3:6] - ref.normal[k]).max(1) / ref.ntol[k]
    for name, d in (("depth", dd), ("pos", dp), ("normal", dn)):
        if d.size and not (np.nan_to_num(d, nan=INF) <= 1.0).all():
            i = np.flatnonzero(k)[int(np.nanargmax(np.nan_to_num(d, nan=INF)))]
            bad.append(f"ray {i}: {name} off by {np.nanmax(d):.3g} tolerances (id {ids[i]}, hit {hits[i]}, reference t {ref.t[i]!r})")
    # well formed, band or not: a unit or zero normal against the ray, depth inside the segment
    v = ref.valid
    nn = np.sqrt((hits[v, 3:6] ** 2).sum(1))
    is_hit = ids[v] != RAY_MISS
    if not (np.abs(nn[is_hit] - 1.0) <= 1e-3).all() or not (nn[~is_hit] == 0).all():
        bad.append("a normal is neither a unit vector (hit) nor zero (miss)")
    worst = tuple(float(np.nanmax(d)) if d.size else 0.0 for d in (dd, dp, dn))
    return bad, worst
