"""The body-body broadphase restated in numpy float64: what tests/test_gpu_broadphase.py holds the device's pair search
(dmxBatchFindPairs: the hashed (x,z) grid and the three forms of the exact pair search) and its safe zones (bp_safe_zone)
against, and what tests/test_broadphase_reference.py holds the oracle's two broadphase modes against.

No grid and no hashing here: every quantity is its definition, evaluated for all n^2 pairs by broadcasting, in row blocks
where n is large.

  aabbs        world AABB of every body: box = centre +- 1/2 sum_j |R_aj| s_j, sphere = centre +- r, convex = the bounds
               of the transformed hull points (ODE's dxBox / dxSphere / dxConvex::computeAABB; R from the quaternion by
               ODE's dRfromQ formula, evaluated as given -- a quaternion is not renormalised here)
  pairs        signed_gap[i, j] = max over axes of max(lo_i - hi_j, lo_j - hi_i); a pair exists iff gap <= 0 (touching
               counts: collideAABBs rejects on `>` only)
  safe_zones   1/2 min(cap_i, min over j != i of enabled class (hypot(dx, dz) - r_i - r_j)), the minimum over ALL j

The band rule.  The device computes AABBs in its precision T, the reference in float64 from the same T-valued inputs, so
a comparison whose |signed_gap| is a few roundings wide can fall either way.  band(T, coords, r_max) = K_BAND eps_T
(max |coordinate| + 2 r_max) is the width inside which a pair (or a static overlap) is "don't care"; outside it the sets
must match exactly.  zone_tol(T, coords, cell) = K_ZONE eps_T (max |coordinate| + cell) is the same for a safe radius.
K_BAND and K_ZONE come from the number format (a face is rounded once at the size of the coordinate) and from emulating the
kernels' arithmetic in float32 (emulated_aabbs, emulated_safe_zones below) against this module:
tests/test_broadphase_reference.py::test_emulated_* measure the worst deviation over their scenes and assert the margins;
the figures are in that module's docstring.
"""
import numpy as np

GEOM_NONE, GEOM_SPHERE, GEOM_BOX, GEOM_CONVEX = 0, 1, 2, 3
SKIN = 1.25            # cell = 2 SKIN r_max (kSkin, dmx_general.cpp)
K_BAND = 2.0           # twice the bound eps M on a gap's rounding; measured: gaps move by up to 0.54 eps M, flips up to 0.33 eps M
K_ZONE = 1.0           # one rounding of the largest coordinate; measured worst 0.062 eps (M + cell): a 16x margin
ALL_CLASS_PAIRS = np.ones((4, 4), bool)


def class_matrix(off=()):
    """4 x 4 symmetric table: do bodies of class a and class b collide (dmxBatchSetClassPairs); `off` = pairs switched off"""
    m = np.ones((4, 4), bool)
    for a, b in off:
        m[a, b] = m[b, a] = False
    return m


def quat_to_R(q):
    """ODE's dRfromQ, (n, 4) (w, x, y, z) -> (n, 3, 3), in the precision of q"""
    q = np.asarray(q)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    qq1, qq2, qq3 = 2 * x * x, 2 * y * y, 2 * z * z
    R = np.empty((q.shape[0], 3, 3), q.dtype)
    R[:, 0, 0] = 1 - qq2 - qq3
    R[:, 0, 1] = 2 * (x * y - w * z)
    R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z)
    R[:, 1, 1] = 1 - qq1 - qq3
    R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y)
    R[:, 2, 1] = 2 * (y * z + w * x)
    R[:, 2, 2] = 1 - qq1 - qq2
    return R


def bound_radius(sides, gtype):
    """bounding-sphere radius: 1/2 |sides| for a box, sides[0] for a sphere or a hull, 0 for a slot without a geom"""
    s = np.asarray(sides, np.float64)
    g = np.asarray(gtype)
    r = np.where(g == GEOM_BOX, 0.5 * np.sqrt((s * s).sum(1)), s[:, 0])
    return np.where(g == GEOM_NONE, 0.0, r)


def aabbs(pos, quat, sides, gtype, hull=None):
    """-> lo, hi (n, 3) float64.  A GEOM_NONE slot gets the empty box (lo = +inf, hi = -inf): it overlaps nothing."""
    p = np.asarray(pos, np.float64)
    s = np.asarray(sides, np.float64)
    g = np.asarray(gtype)
    n = p.shape[0]
    R = quat_to_R(np.asarray(quat, np.float64))
    half = 0.5 * (np.abs(R) * s[:, None, :]).sum(2)                       # box: 1/2 sum_j |R_aj| s_j
    half = np.where((g == GEOM_SPHERE)[:, None], s[:, :1], half)          # sphere: r on every axis
    lo, hi = p - half, p + half
    cv = np.flatnonzero(g == GEOM_CONVEX)
    if cv.size:
        h = np.asarray(hull, np.float64)
        for k0 in range(0, cv.size, 256):                                 # (256 hulls x 1 265 points at a time)
            k = cv[k0:k0 + 256]
            v = np.einsum("nab,pb->npa", R[k], h) + p[k, None, :]
            lo[k], hi[k] = v.min(1), v.max(1)
    none = g == GEOM_NONE
    lo[none], hi[none] = np.inf, -np.inf
    assert lo.shape == (n, 3)
    return lo, hi


def static_aabbs(static_boxes, dtype):
    """AABBs of body-less box geoms [(sides3, pos3, R12)] whose numbers were rounded to `dtype` (dmxBatchSetStaticBoxes)"""
    if not static_boxes:
        return np.zeros((0, 3)), np.zeros((0, 3))
    rd = lambda a: np.asarray(a, np.float64).astype(dtype).astype(np.float64)
    s = rd([b[0] for b in static_boxes])
    p = rd([b[1] for b in static_boxes])
    R = rd([b[2] for b in static_boxes]).reshape(-1, 3, 4)[:, :, :3]
    half = 0.5 * (np.abs(R) * s[:, None, :]).sum(2)
    return p - half, p + half


def signed_gap(lo_a, hi_a, lo_b, hi_b):
    """gap[i, j] between boxes a_i and b_j: max over axes of max(lo_a - hi_b, lo_b - hi_a); <= 0 iff they overlap or touch"""
    gap = np.full((lo_a.shape[0], lo_b.shape[0]), -np.inf)
    with np.errstate(invalid="ignore"):
        for a in range(3):                               # (axis by axis: no (n, m, 3) temporaries)
            d = lo_a[:, None, a] - hi_b[None, :, a]
            np.maximum(d, lo_b[None, :, a] - hi_a[:, None, a], out=d)
            np.maximum(gap, d, out=gap)
    return gap


class PairResult:
    """pairs      (m, 2) int64, i < j < n_active, ascending (i, then j): enabled classes, both with a geom, gap <= 0
    cross      set of (own, ghost): own < n_active <= ghost, same rule
    involved   ascending int64: bodies in a pair or a cross pair, or whose AABB overlaps (gap <= 0) a static box's
    near       [(i, j, gap)] over ALL i < j of enabled classes with |gap| <= band (pairs and cross pairs alike)
    static_gap (n, n_static) signed gap of every body to every static box"""

    def __init__(self, pairs, cross, involved, near, static_gap):
        self.pairs, self.cross, self.involved, self.near, self.static_gap = pairs, cross, involved, near, static_gap

    def pair_set(self):
        return set(map(tuple, self.pairs.tolist()))

    def near_set(self):
        return {(i, j) for i, j, _ in self.near}


def pairs(lo, hi, gtype, n_active=None, class_pairs=None, static_lo=None, static_hi=None, band=0.0, block=1024):
    g = np.asarray(gtype)
    n = lo.shape[0]
    n_active = n if n_active is None else int(n_active)
    cp = ALL_CLASS_PAIRS if class_pairs is None else class_pairs
    out_i, out_j, near = [], [], []
    for i0 in range(0, n_active, block):                 # rows: active bodies only (ghost-ghost overlaps appear nowhere)
        i1 = min(i0 + block, n_active)
        gap = signed_gap(lo[i0:i1], hi[i0:i1], lo, hi)
        ok = cp[g[i0:i1, None], g[None, :]] & (g[i0:i1, None] != GEOM_NONE) & (g[None, :] != GEOM_NONE)
        ok &= np.arange(i0, i1)[:, None] < np.arange(n)[None, :]
        ii, jj = np.nonzero(ok & (gap <= 0))
        out_i.append(ii + i0); out_j.append(jj)
        if band > 0:
            ii, jj = np.nonzero(ok & (np.abs(gap) <= band))
            near += [(int(a + i0), int(b), float(gap[a, b])) for a, b in zip(ii, jj)]
    ii = np.concatenate(out_i) if out_i else np.zeros(0, np.int64)
    jj = np.concatenate(out_j) if out_j else np.zeros(0, np.int64)
    own = jj < n_active
    plist = np.stack([ii[own], jj[own]], 1).astype(np.int64)             # (np.nonzero is row-major: already ascending)
    cross = set(zip(ii[~own].tolist(), jj[~own].tolist()))
    inv = np.zeros(n, bool)
    inv[plist.ravel()] = True
    inv[ii[~own]] = True
    sgap = np.zeros((n, 0))
    if static_lo is not None and len(static_lo):
        sgap = signed_gap(lo, hi, np.asarray(static_lo, np.float64), np.asarray(static_hi, np.float64))
        sgap[g == GEOM_NONE] = np.inf
        inv[:n_active] |= (sgap[:n_active] <= 0).any(1)
    return PairResult(plist, cross, np.flatnonzero(inv[:n_active]), near, sgap)


def cell_size(sides, gtype):
    """the grid's cell: 2 SKIN r_max over every slot with a geom (ghost slots included); r_max = 1 in a batch without geoms"""
    r = bound_radius(sides, gtype)
    rmax = r.max() if r.size and r.max() > 0 else 1.0
    return 2.0 * SKIN * rmax


def zone_parts(pos, sides, gtype, class_pairs=None, block=1024):
    """-> (cap (n,), gapmin (n,), cell): cap_i = cell - r_i - (largest radius among the classes present that i's class collides
    with), +inf when there is none; gapmin_i = min over j != i whose class collides with i's of hypot(dx, dz) - r_i - r_j, over
    ALL j.  Every slot with a geom takes part, ghost slots too."""
    p = np.asarray(pos, np.float64)
    g = np.asarray(gtype)
    cp = ALL_CLASS_PAIRS if class_pairs is None else class_pairs
    n = p.shape[0]
    r = bound_radius(sides, gtype)
    cell = cell_size(sides, gtype)
    r_cls = np.array([r[g == c].max() if (g == c).any() else 0.0 for c in range(4)])
    r_cls[GEOM_NONE] = 0.0
    rm = np.array([max([r_cls[c] for c in range(1, 4) if cp[gi, c]] + [0.0]) for gi in range(4)])
    cap = np.where(rm[g] > 0, cell - r - rm[g], np.inf)
    gapmin = np.full(n, np.inf)
    for i0 in range(0, n, block):
        i1 = min(i0 + block, n)
        d = np.hypot(p[i0:i1, None, 0] - p[None, :, 0], p[i0:i1, None, 2] - p[None, :, 2])
        d -= r[i0:i1, None]
        d -= r[None, :]
        ok = cp[g[i0:i1, None], g[None, :]] & (g[None, :] != GEOM_NONE) & (np.arange(i0, i1)[:, None] != np.arange(n)[None, :])
        gapmin[i0:i1] = np.where(ok, d, np.inf).min(1)
    return cap, gapmin, cell


def safe_zones(pos, sides, gtype, class_pairs=None, block=1024, capped=True):
    """-> (safe (n,), cell).  safe_i = 1/2 min(cap_i, gapmin_i) (zone_parts); +inf for a slot without a geom.  capped=False
    leaves the cap out: half the true horizontal gap to the nearest bounding sphere, the bound a sound zone may not exceed."""
    cap, gapmin, cell = zone_parts(pos, sides, gtype, class_pairs, block)
    safe = 0.5 * (np.minimum(cap, gapmin) if capped else gapmin)
    return np.where(np.asarray(gtype) == GEOM_NONE, np.inf, safe), cell


def band(dtype, pos, sides, gtype, static_boxes=None):
    """K_BAND eps_T (max |coordinate| + 2 r_max): the |signed_gap| below which rounding decides an overlap"""
    m = float(np.abs(np.asarray(pos, np.float64)).max()) if len(pos) else 0.0
    for b in static_boxes or ():
        m = max(m, float(np.abs(np.asarray(b[1], np.float64)).max() + 0.5 * np.linalg.norm(b[0])))
    rmax = float(bound_radius(sides, gtype).max()) if len(pos) else 0.0
    return K_BAND * float(np.finfo(dtype).eps) * (m + 2.0 * rmax)


def zone_tol(dtype, pos, cell):
    """K_ZONE eps_T (max |coordinate| + cell): the width inside which a safe radius may differ from safe_zones()"""
    m = float(np.abs(np.asarray(pos, np.float64)).max()) if len(pos) else 0.0
    return K_ZONE * float(np.finfo(dtype).eps) * (m + cell)


# ---- the kernels' arithmetic in float32, operation by operation (no contraction beyond the fma the source writes) ------------
def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)    # (exact product, one rounding)


def emulated_aabbs(pos, quat, sides, gtype, hull=None):
    """body_aabb / wave_hull_aabb (dmx_grid.hpp, dmx_collide_wave.hpp) in float32: -> lo, hi float32"""
    f = np.float32
    p, q, s, g = np.asarray(pos, f), np.asarray(quat, f), np.asarray(sides, f), np.asarray(gtype)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    two, one = f(2), f(1)
    qq1, qq2, qq3 = two * x * x, two * y * y, two * z * z
    R = np.empty((len(p), 3, 3), f)
    R[:, 0, 0] = one - qq2 - qq3
    R[:, 0, 1] = two * _fma32(x, y, -(w * z))
    R[:, 0, 2] = two * _fma32(x, z, w * y)
    R[:, 1, 0] = two * _fma32(x, y, w * z)
    R[:, 1, 1] = one - qq1 - qq3
    R[:, 1, 2] = two * _fma32(y, z, -(w * x))
    R[:, 2, 0] = two * _fma32(x, z, -(w * y))
    R[:, 2, 1] = two * _fma32(y, z, w * x)
    R[:, 2, 2] = one - qq1 - qq2
    half = f(0.5) * (np.abs(R[:, :, 0] * s[:, None, 0]) + np.abs(R[:, :, 1] * s[:, None, 1]) + np.abs(R[:, :, 2] * s[:, None, 2]))
    half = np.where((g != GEOM_BOX)[:, None], s[:, :1], half).astype(f)
    lo, hi = p - half, p + half
    cv = np.flatnonzero(g == GEOM_CONVEX)
    if cv.size:
        h = np.asarray(hull, f)
        for k in cv:                                     # mulv: (R00 v0 + R01 v1) + R02 v2, then + x
            v = (R[k, None, :, 0] * h[:, None, 0] + R[k, None, :, 1] * h[:, None, 1]) + R[k, None, :, 2] * h[:, None, 2]
            v = v + p[k]
            lo[k], hi[k] = v.min(0), v.max(0)
    none = g == GEOM_NONE
    lo[none], hi[none] = np.inf, -np.inf
    return lo, hi


def emulated_safe_zones(pos, sides, gtype, class_pairs=None):
    """bp_safe_zone's arithmetic in float32 over ALL j (the walk's 3x3 block is the kernel's business, not the arithmetic's)"""
    f = np.float32
    p, s, g = np.asarray(pos, f), np.asarray(sides, f), np.asarray(gtype)
    cp = ALL_CLASS_PAIRS if class_pairs is None else class_pairs
    n = len(p)
    r = np.where(g == GEOM_BOX, f(0.5) * np.sqrt(s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1] + s[:, 2] * s[:, 2]), s[:, 0]).astype(f)
    r = np.where(g == GEOM_NONE, f(0), r).astype(f)
    r64 = bound_radius(s, g)                                              # (the host's maxima are taken in double)
    rmax = r64.max() if r64.max() > 0 else 1.0
    cell = f(2.0 * SKIN * rmax)
    r_cls = np.array([r64[g == c].max() if (g == c).any() else 0.0 for c in range(4)]).astype(f)
    rm = np.array([max([r_cls[c] for c in range(1, 4) if cp[gi, c]] + [f(0)]) for gi in range(4)], f)
    cap = np.where(rm[g] > 0, cell - r - rm[g], f(np.inf)).astype(f)
    ddx, ddz = p[None, :, 0] - p[:, None, 0], p[None, :, 2] - p[:, None, 2]
    d = np.sqrt(ddx * ddx + ddz * ddz) - r[:, None] - r[None, :]
    ok = cp[g[:, None], g[None, :]] & (g[None, :] != GEOM_NONE) & ~np.eye(n, dtype=bool)
    safe = f(0.5) * np.minimum(cap, np.where(ok, d, f(np.inf)).min(1))
    return np.where(g == GEOM_NONE, f(np.inf), safe).astype(f), float(cell)
