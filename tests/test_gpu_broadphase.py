"""The device's body-body broadphase against tests/bp_reference.py, the float64 restatement of its definitions: the pair search
(dmxBatchFindPairs: the hashed (x,z) grid and the three forms of the exact pair search) and the safe zones (bp_safe_zone).

Inputs are uploaded, then POS, QUAT and SIDES are downloaded again and THOSE feed the reference: what the device holds.

The band rule (bp_reference.py).  The device computes AABBs in its precision T, the reference in float64 from the same T-valued
inputs.  A pair or a static overlap with |signed gap| <= band = K_BAND eps_T (max |coordinate| + 2 r_max) may fall either way;
everything outside the band matches exactly, and a scene may leave at most 2 % of its reference pairs inside the band (0.1 % near
the origin) -- asserted per scene.  The list's structure (i < j < n_active, strictly ascending, `involved` strictly ascending and
exactly what the device's own pairs and static overlaps imply, cross pairs unique) is asserted with no band at all.
K_BAND = 2: a face is rounded once at the coordinate's size (at most eps M / 2), a gap is a difference of two faces; the float32
emulation of body_aabb / wave_hull_aabb (test_broadphase_reference.py) moved gaps by at most 0.54 eps M and decided 13 of
~100 000 pairs differently, the widest at |gap| = 0.33 eps M.
Safe radii: |device - reference| <= tol = K_ZONE eps_T (max |coordinate| + cell), K_ZONE = 1; the emulation of bp_safe_zone's
arithmetic deviated by at most 0.062 eps (M + cell).  Soundness (a zone never exceeds half the true gap) uses the same tol.

Which implementation ran.  The pair search has three forms -- one workgroup (ex_small_front; set_exact_pipeline(2)), a wavefront
per body (ex_pair_count_wave; set_exact_pipeline(1), n_active <= 8 192) and a lane per body (more than 8 192) -- and no counter
of the C ABI says which one a dmxBatchFindPairs call took (collision_stats counts ticks, and this call is not one).  The forms
are chosen by the pipeline mode and sizes alone (use_small_exact / launch_exact_pairs): the helper below restates the one-workgroup
form's size rule and asserts it for every scene that names that form, and scenes naming the other forms set the staged mode.
Bucket growth (torus -> scrambled -> capacity doubling) has no counter either: the column scenes hold more bodies in one (x,z)
column than the initial capacity of 8, which the staged forms cannot serve without growing.
"""
import ctypes as C

import numpy as np
import pytest

from __graft_entry__ import load_package

import bp_reference as ref
import bp_scenes as sc
from bp_reference import GEOM_BOX, GEOM_CONVEX, GEOM_NONE, GEOM_SPHERE

pkg = load_package()
B = pkg.batch
pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32"]
H = 1.0 / 60.0
CLASS_PAIRS = [(GEOM_SPHERE, GEOM_SPHERE), (GEOM_SPHERE, GEOM_BOX), (GEOM_SPHERE, GEOM_CONVEX), (GEOM_BOX, GEOM_BOX),
               (GEOM_BOX, GEOM_CONVEX), (GEOM_CONVEX, GEOM_CONVEX)]


# ---- helpers ---------------------------------------------------------------------------------------------------------------
def _world(case, dtype, class_off=(), plane=False, static_fused=None):
    w = pkg.BatchWorld(case.n, dtype=dtype, gravity=(0.0, 0.0, 0.0))
    w.upload(B.POS, case.pos)
    w.upload(B.QUAT, case.quat)
    w.upload(B.LVEL, np.zeros((case.n, 3)))
    w.upload(B.AVEL, np.zeros((case.n, 3)))
    if case.hull is not None:
        w.set_convex_hull(case.hull)
    w.upload(B.SIDES, case.sides)
    w.upload_geom_type(case.gtype)
    if case.statics:
        w.set_static_boxes(case.statics)
    if static_fused is not None:
        w.set_static_path(static_fused)
    if plane:
        w.set_plane(0.0, 1.0, 0.0, -100.0, enable=True)
    if case.n_active is not None:
        w.set_active_count(case.n_active)
    for a, b in class_off:
        w.set_class_pairs(a, b, False)
    return w


def _one_workgroup_fits(n, n_static, n_pairs):
    """use_small_exact's size rule (dmx_general.cpp, dmx_exact.hip) for the capacity dmxBatchFindPairs ends up with: slots <= 8 192,
    a grid of fewer than 32 768 buckets, and inv (1 + n_static) + pairs <= 8 192 entries with the pair capacity grown to hold the
    scene's pairs (1 024 doubled, or pairs * 1.25 + 64)"""
    cap = 1024
    while cap < n_pairs:
        cap = max(2 * cap, n_pairs + n_pairs // 4 + 64)
    inv = min(2 * cap, n)
    return n <= 8192 and 2 * n <= 32768 and inv * (1 + n_static) + cap <= 8192 and inv <= 8192


def _set_form(w, form, n_active, n, n_static=0, n_pairs=0):
    if form == "one":
        assert _one_workgroup_fits(n, n_static, n_pairs), "scene too large for the one-workgroup form"
        w.set_exact_pipeline(B.EXACT_ONE_WORKGROUP)
    else:
        assert (n_active <= 8192) == (form == "wave")
        w.set_exact_pipeline(B.EXACT_STAGED)


def _held(w, case, dtype):
    """what the device holds: downloaded poses and extents, the hull and the static boxes rounded as the library rounds them"""
    pos, quat, sides = w.download(B.POS), w.download(B.QUAT), w.download(B.SIDES)
    hull = None if case.hull is None else case.hull.astype(dtype)
    return pos, quat, sides, hull


_REF_CACHE = {}


def _reference(case, dtype, held, class_off=()):
    pos, quat, sides, hull = held
    key = (case.name, dtype, tuple(class_off), case.n_active, len(case.statics), pos.tobytes()[:4096], sides.tobytes()[:1024])
    if key not in _REF_CACHE:
        lo, hi = ref.aabbs(pos, quat, sides, case.gtype, hull)
        slo, shi = ref.static_aabbs(case.statics, dtype)
        band = 0.0 if case.exact else ref.band(dtype, pos, sides, case.gtype, case.statics)
        blk = max(64, 2_000_000 // max(case.n, 1))
        _REF_CACHE[key] = (ref.pairs(lo, hi, case.gtype, case.n_active, ref.class_matrix(class_off), slo, shi, band=band, block=blk), band)
    return _REF_CACHE[key]


def _check_find_pairs(w, case, dtype, r, band, label):
    """one dmxBatchFindPairs call against the reference result r: structure with no band, membership by the band rule"""
    n_active = case.n if case.n_active is None else case.n_active
    pairs, involved, cross = w.find_pairs()
    what = f"{case.name} {dtype} {label}"
    # -- structure, no band
    if len(pairs):
        assert np.all(pairs[:, 0] >= 0) and np.all(pairs[:, 0] < pairs[:, 1]) and np.all(pairs[:, 1] < n_active), what
        key = pairs[:, 0].astype(np.int64) * (case.n + 1) + pairs[:, 1]
        assert np.all(np.diff(key) > 0), f"{what}: pairs not strictly ascending"
    assert np.all(np.diff(involved) > 0), f"{what}: involved not strictly ascending"
    assert len(involved) == 0 or (involved[0] >= 0 and involved[-1] < n_active), what
    cross_set = set(map(tuple, cross.tolist()))
    assert len(cross_set) == len(cross), f"{what}: duplicate cross pairs"
    assert all(a < n_active <= b < case.n for a, b in cross_set), what
    # -- membership: everything outside the band matches exactly
    got = set(map(tuple, pairs.tolist()))
    near = r.near_set()
    want = r.pair_set()
    missing, extra = (want - got) - near, (got - want) - near
    assert not missing and not extra, f"{what}: missing {sorted(missing)[:8]} extra {sorted(extra)[:8]} (band {band:.3g})"
    nref = len(want) + len(r.cross)
    share = len(near) / max(nref, 1)
    limit = 0.0 if case.exact else (0.001 if case.near_origin else 0.02)
    print(f"{what}: {len(got)} pairs, {len(cross_set)} cross, {len(involved)} involved; band {band:.3g} holds {len(near)} of {nref} ({100 * share:.3f} %)")
    assert share <= limit, f"{what}: {len(near)} of {nref} reference pairs inside the band"
    # -- cross pairs: the whole set when it fits the list, else 256 of them
    cross_ok = r.cross | {p for p in near if p[1] >= n_active}
    assert cross_set <= cross_ok, f"{what}: cross pairs not in the reference {sorted(cross_set - cross_ok)[:8]}"
    sure_cross = r.cross - near
    if len(cross_ok) <= 256:
        assert sure_cross <= cross_set, f"{what}: lost cross pairs {sorted(sure_cross - cross_set)[:8]}"
    else:
        assert len(cross_set) == 256 or len(sure_cross) <= len(cross_set) <= 256, what
    # -- involved: exactly the members of the device's own pairs, the own bodies of its cross pairs (of all of them: bodies that
    #    the reference puts in a cross pair outside the band) and the static overlappers, static overlaps inside the band free
    inv = np.zeros(case.n, bool)
    inv[pairs.ravel()] = True
    must = inv.copy()
    for a, _ in (sure_cross if len(cross_ok) > 256 else cross_set):
        must[a] = True
    may = must.copy()
    for a, _ in cross_ok:
        may[a] = True
    if r.static_gap.shape[1]:
        sg = r.static_gap[:n_active].min(1)
        must[:n_active] |= sg < -band
        may[:n_active] |= sg <= band
    got_inv = np.zeros(case.n, bool)
    got_inv[involved] = True
    assert not (must & ~got_inv).any(), f"{what}: not involved {np.flatnonzero(must & ~got_inv)[:8]}"
    assert not (got_inv & ~may).any(), f"{what}: involved without cause {np.flatnonzero(got_inv & ~may)[:8]}"
    return got


def _run_pairs(case, dtype, forms, class_off=(), calls=1, **kw):
    out = None
    for form in forms:
        w = _world(case, dtype, class_off, **kw)
        held = _held(w, case, dtype)
        r, band = _reference(case, dtype, held, class_off)
        _set_form(w, form, case.n if case.n_active is None else case.n_active, case.n, len(case.statics), len(r.pairs))
        for k in range(calls):
            out = _check_find_pairs(w, case, dtype, r, band, f"{form}#{k}")
        w.close()
    return out, r


def _forms_for(n, n_active=None):
    return ("one", "wave") if (n if n_active is None else n_active) <= 8192 else ("lane",)


# ---- the pair search -------------------------------------------------------------------------------------------------------
_RANDOM = sc.random_pair_cases()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", range(len(_RANDOM)), ids=[c.name for c, _ in _RANDOM])
def test_random_scenes_near_and_far(dtype, k):
    """tumbling boxes at 3-10 partners per body; spheres, boxes and hulls (a cube, the stored teapot) with GEOM_NONE slots
    sprinkled in; the same scenes 1 km and 8 km out and in negative coordinates; through every form their size allows"""
    case, forms = _RANDOM[k]
    got, r = _run_pairs(case, dtype, forms)
    assert len(got) > case.n


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hull", ["cube", "teapot"])
def test_class_pairs_switched_off_one_by_one(dtype, hull):
    """pairs of a switched-off class pair vanish and nothing else changes"""
    case = sc.mixed(700, 31, sc.cube_hull() if hull == "cube" else sc.teapot_hull(), none_share=0.04, name=hull)
    base, _ = _run_pairs(case, dtype, ("wave",))
    g = case.gtype
    for a, b in CLASS_PAIRS:
        got, r = _run_pairs(case, dtype, ("one", "wave"), class_off=[(a, b)])
        of_class = {p for p in base if {int(g[p[0]]), int(g[p[1]])} == {a, b}}
        assert of_class, "the scene has pairs of every class pair"
        assert not (got & of_class)
        assert (base - of_class) - r.near_set() == got - r.near_set()


@pytest.mark.parametrize("dtype", DTYPES)
def test_exactly_representable_edges(dtype):
    """faces touching are a pair, faces 2^-10 apart are not, nested boxes are; no band: every number and every sum is exact"""
    case = sc.lattice_boxes()
    for c in (case, sc.with_filler(case, 700), sc.with_filler(case, 8400)):
        got, r = _run_pairs(c, dtype, _forms_for(c.n))
        assert got == r.pair_set() == {(0, 1), (0, 3), (1, 3), (5, 6), (5, 7), (9, 10), (10, 11), (12, 13)}


@pytest.mark.parametrize("dtype", DTYPES)
def test_spheres_on_cell_boundaries(dtype):
    """r = 0.4: cell = exactly 1; centres on integer cell boundaries, at x = -0.0, straddling ix = -1 | 0.  Every gap is 0.0125 or
    more from zero: the band (1e-6) is empty, the answer exact."""
    case = sc.cell_boundary_spheres()
    for c in (case, sc.with_filler(case, 600), case.moved((-3.0, 0.0, -3.0)), case.moved((0.5, 0.0, 0.5))):
        got, r = _run_pairs(c, dtype, ("one", "wave"))
        assert not r.near and got == r.pair_set() and len(got) >= 12


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [8, 9, 17, 40])
def test_stacks_in_one_column_grow_the_buckets(dtype, k):
    """k bodies in one (x,z) column against a bucket capacity of 8: the staged forms go torus -> scrambled -> capacity doubling
    (twice for 17, three times for 40); the result equals the reference after the growth and on a second call"""
    case = sc.column(k)
    for c in (case, sc.with_filler(case, 8300)):
        got, r = _run_pairs(c, dtype, _forms_for(c.n), calls=2)
        assert len(got) >= k - 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nc,axis", [(2, 0), (3, 0), (2, 2), (3, 2)])
def test_clusters_one_torus_period_apart(dtype, nc, axis):
    """n <= 512: 32 x 32 columns of cell 1.0; clusters 32.0 apart along x or z share their buckets cell for cell: no pair across
    clusters, none lost, none twice"""
    case = sc.torus_clusters(nc, axis)
    assert case.n <= 512
    got, r = _run_pairs(case, dtype, ("one", "wave"))
    m = case.n // nc
    assert all(i // m == j // m for i, j in got)
    per = [{(i % m, j % m) for i, j in got if i // m == c} for c in range(nc)]
    assert len(per[0]) > m and all(p == per[0] for p in per)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [8, 9, 32, 33])
@pytest.mark.parametrize("big_last", [False, True])
def test_partner_list_limits(dtype, k, big_last):
    """one large box over k small ones: with the lowest index it owns k pairs -- 8 fit the one-workgroup form's staged list, 32 the
    staged forms', one more makes the write pass walk again -- with the highest index it owns none of them"""
    case = sc.one_over_many(k, big_last)
    for c in (case, sc.with_filler(case, 600), sc.with_filler(case, 8300)):
        got, r = _run_pairs(c, dtype, _forms_for(c.n))
        big = k if big_last else 0
        assert got == r.pair_set() and sum(1 for p in got if big in p) == k


@pytest.mark.parametrize("dtype", DTYPES)
def test_ghost_slots(dtype):
    """overlaps between active bodies and ghosts are cross pairs, never pairs, and make the active body involved; ghost-ghost
    overlaps appear nowhere; more than 256 cross pairs: 256 are listed, all of them true"""
    base = sc.tumbling_boxes(1200, 41)
    few = sc.with_ghosts(base, 1160)                 # 40 ghosts: a hundred or so cross pairs
    got, r = _run_pairs(few, dtype, ("one", "wave"))
    assert 0 < len(r.cross) <= 256
    many = sc.with_ghosts(base, 800)
    got, r = _run_pairs(many, dtype, ("one", "wave"))
    assert len(r.cross) > 256
    big = sc.with_ghosts(sc.tumbling_boxes(9000, 42), 8600)
    _run_pairs(big, dtype, ("lane",))


def _static_sets():
    tilted = [((6.0, 0.4, 3.0), (1.0, 1.2, -2.0), sc.rot_y_z(0.5, 0.3)), ((0.5, 5.0, 0.5), (-4.0, 1.0, 4.0), sc.rot_y_z(1.1, -0.4))]
    flat = [((8.0, 1.0, 8.0), (0.0, -0.5, 0.0), sc.IDENT_R12), ((2.0, 2.0, 2.0), (5.0, 2.0, 5.0), sc.IDENT_R12)]
    return {"flat": flat, "tilted": tilted, "map": pkg.scenes.reference_map()}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("statics", ["flat", "tilted", "map"])
def test_static_boxes_make_bodies_involved(dtype, statics):
    """every body whose AABB overlaps a static box's AABB is involved, in a pair or not -- with the ground plane on or off and
    either static path (dmxBatchFindPairs' contract does not depend on them)"""
    case = sc.with_statics(sc.tumbling_boxes(500, 56, extent=24.0, height=4.0), _static_sets()[statics], statics)
    for plane in (False, True):
        for fused in (True, False):
            got, r = _run_pairs(case, dtype, ("one", "wave"), plane=plane, static_fused=fused)
            alone = set(np.flatnonzero(r.static_gap.min(1) < 0).tolist()) - {i for p in got for i in p}
            assert len(alone) >= 3, "the scene has bodies at static boxes that are in no pair"
    mixed = sc.with_statics(sc.mixed(400, 52, sc.cube_hull(), extent=14.0), _static_sets()[statics], statics)
    _run_pairs(mixed, dtype, ("one", "wave"))
    far = sc.with_statics(sc.tumbling_boxes(500, 56, extent=24.0, height=4.0), _static_sets()[statics], statics).moved((-1000.0, 0.0, 1000.0))
    _run_pairs(far, dtype, ("wave",))


@pytest.mark.parametrize("dtype", DTYPES)
def test_resizing_follows_into_the_cell(dtype):
    """new SIDES that enlarge r_max after a first search: the cell follows, the result equals the reference"""
    case = sc.tumbling_boxes(800, 61, extent=30.0)
    for form in ("one", "wave"):
        w = _world(case, dtype)
        r, band = _reference(case, dtype, _held(w, case, dtype))
        _set_form(w, form, case.n, case.n, 0, len(r.pairs))
        _check_find_pairs(w, case, dtype, r, band, form)
        grown = sc.Case(case.name + "x2", case.pos, case.quat, case.sides * 2.0, case.gtype)
        w.upload(B.SIDES, grown.sides)
        r2, band2 = _reference(grown, dtype, _held(w, grown, dtype))
        assert len(r2.pairs) > 3 * len(r.pairs) > 0 and (form != "one" or _one_workgroup_fits(case.n, 0, len(r2.pairs)))
        _check_find_pairs(w, grown, dtype, r2, band2, form + " grown")
        w.close()


# ---- safe zones ------------------------------------------------------------------------------------------------------------
_hip = None


def _read_slab(w, n, dtype):
    """components of the current slab by the documented tile layout (DMX_SLAB_TILE 64 x DMX_SLAB_COMPONENTS 30), device to host"""
    global _hip
    if _hip is None:
        _hip = C.CDLL(None)                      # the HIP runtime is already in the process
    tiles = (n + 63) // 64
    buf = np.empty(tiles * 30 * 64, dtype)
    addr = w.device_ptr(B.POS, 0)
    assert addr
    assert _hip.hipMemcpy(C.c_void_p(buf.ctypes.data), C.c_void_p(addr), C.c_size_t(buf.nbytes), 2) == 0      # device to host
    t = buf.reshape(tiles, 30, 64)
    return {c: t[:, c, :].reshape(-1)[:n].copy() for c in (0, 2, 26, 27, 28, 29)}


def _ulps(a, b, dtype):
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b).astype(dtype)).astype(np.float64)


def _check_zones(case, dtype, class_off=(), expect_exact_only=None, **kw):
    w = _world(case, dtype, class_off, **kw)
    pos, quat, sides, _ = _held(w, case, dtype)
    g = case.gtype
    cp = ref.class_matrix(class_off)
    blk = max(64, 2_000_000 // max(case.n, 1))
    cap, gapmin, cell = ref.zone_parts(pos, sides, g, cp, block=blk)
    want = np.where(g == GEOM_NONE, np.inf, 0.5 * np.minimum(cap, gapmin))         # = ref.safe_zones
    bound = 0.5 * gapmin                                                           # half the true gap, no cap
    tol = ref.zone_tol(dtype, pos, cell)
    exact_only, ballistic = w.chunk_begin()
    slab = _read_slab(w, case.n, dtype)
    what = f"{case.name} {dtype} off={list(class_off)}"
    geom = g != GEOM_NONE
    # (c) the build position is the position, bit for bit; the radius is the bounding radius to 2 ulp
    assert np.array_equal(slab[26].view(np.uint8), pos[:, 0].copy().view(np.uint8)), what
    assert np.array_equal(slab[27].view(np.uint8), pos[:, 2].copy().view(np.uint8)), what
    assert _ulps(slab[29][geom], ref.bound_radius(sides, g)[geom], dtype).max() <= 2.0, what
    safe = slab[28].astype(np.float64)
    fin = np.isfinite(want)
    # (b) agreement with the reference, class rule and cap included; unbounded where the reference is
    assert np.array_equal(np.isfinite(safe), fin), f"{what}: finite zones differ at {np.flatnonzero(np.isfinite(safe) != fin)[:8]}"
    assert np.all(safe[~fin] == np.inf), what
    dev = np.abs(safe[fin] - want[fin]) if fin.any() else np.zeros(1)
    print(f"{what}: {int(fin.sum())} zones, {int((want[fin] > 0).sum())} positive, worst deviation {dev.max() / tol * ref.K_ZONE:.4f} eps (M + cell); "
          f"tol {tol:.3g}; exact_only {exact_only}")
    assert dev.max() <= tol, f"{what}: zone off by {dev.max():.3g} > {tol:.3g} at {np.flatnonzero(fin)[dev.argmax()]}"
    # (a) soundness: never more than half the true gap
    assert np.all(safe[fin] <= bound[fin] + tol), what
    # (d) exact_only = some zone is not positive (margins well outside tol decide; inside them nothing is asserted)
    lowest = want[fin].min() if fin.any() else np.inf
    if expect_exact_only is not None:
        assert exact_only == expect_exact_only, what
    elif lowest < -tol:
        assert exact_only, what
    elif lowest > tol and not case.statics:
        assert not exact_only, what
    if not exact_only and not case.statics:
        assert ballistic
        w.chunk_ticks(H, 1)                       # the state moves to the other slab: the zones are constants of both
        other = _read_slab(w, case.n, dtype)
        for c in (26, 27, 28, 29):
            assert np.array_equal(other[c][geom].view(np.uint8), slab[c][geom].view(np.uint8)), f"{what}: component {c} differs between the slabs"
        violated, _ = w.chunk_end()
        assert not violated
        w.chunk_commit(1)
    else:
        w.chunk_end()
        w.chunk_commit(0)
    w.close()
    return want, tol


def _spread(case, factor):
    """the same bodies with their horizontal positions scaled: bounding spheres apart, zones positive"""
    pos = case.pos.copy()
    pos[:, [0, 2]] *= factor
    return sc.Case(f"{case.name}x{factor}", pos, case.quat, case.sides, case.gtype, case.hull, case.statics, case.n_active, case.near_origin)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("offset", [(0.0, 0.0, 0.0)] + sc.FAR, ids=["origin", "+1km", "-1km", "+8km", "-8km", "negative"])
def test_zones_of_sparse_and_crowded_scenes(dtype, offset):
    for hull in (sc.cube_hull(), sc.teapot_hull()):
        sparse = sc.sparse_mixed(1500, 71, hull).moved(offset)
        want, tol = _check_zones(sparse, dtype)
        assert (want[np.isfinite(want)] > tol).sum() > 800
    _check_zones(sc.tumbling_boxes(2000, 1).moved(offset), dtype)          # crowded: most zones negative
    if offset in ((0.0, 0.0, 0.0), sc.FAR[3]):
        _check_zones(sc.tumbling_boxes(9000, 2).moved(offset), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_zones_with_class_pairs_off(dtype):
    """zones keep apart only what can collide: the enabled-class rule in the neighbours and in the cap"""
    case = sc.sparse_mixed(1200, 72, sc.cube_hull())
    for pair in CLASS_PAIRS:
        _check_zones(case, dtype, class_off=[pair])
    _check_zones(case, dtype, class_off=[(GEOM_BOX, GEOM_BOX), (GEOM_BOX, GEOM_SPHERE), (GEOM_BOX, GEOM_CONVEX)])      # boxes: unbounded
    hulls = sc.sparse_mixed(600, 73, sc.teapot_hull())
    hulls.gtype[hulls.gtype != GEOM_NONE] = GEOM_CONVEX
    hulls.sides[:, 0] = sc.hull_radius(hulls.hull)
    want, _ = _check_zones(hulls, dtype)
    assert np.isfinite(want).sum() > 500 and (want[np.isfinite(want)] < 0).any() and (want[np.isfinite(want)] > 0).any()
    want, _ = _check_zones(hulls, dtype, class_off=[(GEOM_CONVEX, GEOM_CONVEX)], expect_exact_only=False)
    assert not np.isfinite(want).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_zones_of_stacks_clusters_and_ghosts(dtype):
    for k in (9, 17, 40):                                       # bucket growth inside build_safe_zones
        _check_zones(sc.column(k), dtype)
        _check_zones(sc.with_filler(sc.column(k), 300), dtype)
    for nc, axis in ((2, 0), (3, 2)):                           # torus aliasing: the clusters' buckets coincide
        _check_zones(sc.torus_clusters(nc, axis), dtype)
        _check_zones(_spread(sc.torus_clusters(nc, axis), 4.0), dtype)          # (4 x 32: still whole periods apart)
    sparse = sc.sparse_mixed(1200, 74, sc.cube_hull())
    want, tol = _check_zones(sc.with_ghosts(sparse, 1000), dtype)              # ghost slots take part and get zones too
    assert np.isfinite(want[1000:]).sum() > 150


def _two_spheres(gap, y=0.0):
    """two spheres r = 0.5 whose bounding spheres are `gap` apart horizontally, and bystanders well away"""
    pos = np.array([[0.0, 0.0, 0.0], [0.6 * (1.0 + gap), y, 0.8 * (1.0 + gap)], [6.0, 0.0, 0.0], [0.0, 0.0, 6.0]])
    sides = np.zeros((4, 3)); sides[:, 0] = 0.5
    q = np.zeros((4, 4)); q[:, 0] = 1.0
    return sc.Case(f"two{gap:+g}", pos, q, sides, np.full(4, GEOM_SPHERE, np.uint8))


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_only_follows_the_sign_of_the_smallest_zone(dtype):
    """margins of 0.01 on both sides, 10^4 times the float32 tolerance"""
    _check_zones(_two_spheres(+0.01), dtype, expect_exact_only=False)
    _check_zones(_two_spheres(-0.01), dtype, expect_exact_only=True)
    _check_zones(_two_spheres(-0.01, y=30.0), dtype, expect_exact_only=True)            # horizontal gap: height does not matter
    _check_zones(_two_spheres(-0.01), dtype, class_off=[(GEOM_SPHERE, GEOM_SPHERE)], expect_exact_only=False)
    box = lambda top: [((2.0, 1.0, 2.0), (0.0, top - 0.5, 0.0), sc.IDENT_R12)]      # a static box under sphere 0, its top face at `top`
    reach = sc.with_statics(_two_spheres(+0.5), box(-0.49), "reach")
    clear = sc.with_statics(_two_spheres(+0.5), box(-0.51), "clear")
    _check_zones(reach, dtype, static_fused=False, expect_exact_only=True)       # exact static path: a sphere that reaches a static AABB
    _check_zones(clear, dtype, static_fused=False, expect_exact_only=False)
    _check_zones(reach, dtype, static_fused=True, expect_exact_only=False)       # fused static path: the fused kernels step it


@pytest.mark.parametrize("dtype", DTYPES)
def test_chunks_report_a_body_leaving_its_zone(dtype):
    """spheres on a 2 m grid moving horizontally at 0.1-0.5 m/s, no gravity: zone = cap / 2 = 0.0625 m for every one.  A checked
    tick tests the position it starts from.  6-tick chunks: the fastest body is 5 x 0.0083 = 0.042 m out at the last test: clean.
    A 12-tick chunk: 11 x 0.0083 = 0.092 m: violated, and rolled back to its start state.  Margins 0.02 m, tol 1e-6."""
    rng = np.random.default_rng(81)
    n, side = 256, 16
    k = np.arange(n)
    pos = np.stack([2.0 * (k % side), rng.uniform(0.0, 3.0, n), 2.0 * (k // side)], 1)
    sides = np.zeros((n, 3)); sides[:, 0] = 0.25
    q = np.zeros((n, 4)); q[:, 0] = 1.0
    speed, ang = rng.uniform(0.1, 0.5, n), rng.uniform(0.0, 2 * np.pi, n)
    speed[:4] = 0.5
    vel = np.stack([speed * np.cos(ang), np.zeros(n), speed * np.sin(ang)], 1)
    case = sc.Case("movers", pos, q, sides, np.full(n, GEOM_SPHERE, np.uint8))
    w = _world(case, dtype)
    w.upload(B.LVEL, vel)
    vel_t = w.download(B.LVEL).astype(np.float64)
    hT = float(np.dtype(dtype).type(H))

    def run_chunk(nticks, start):
        zone, cell = ref.safe_zones(start, sides, case.gtype)
        tol = ref.zone_tol(dtype, start, cell)
        assert np.allclose(zone, 0.0625, atol=1e-6)
        exact_only, ballistic = w.chunk_begin()
        assert not exact_only and ballistic
        w.chunk_ticks(H, nticks)                         # ballistic: tested at the first and the last tick's start positions
        violated, _ = w.chunk_end()
        disp = (nticks - 1) * hT * np.hypot(vel_t[:, 0], vel_t[:, 2])
        inside, outside = np.all(disp < zone - tol - 0.01), np.any(disp > zone + tol + 0.01)
        assert inside != outside, "the chunk is decided with margin"
        assert violated == outside
        traj = [start + t * hT * vel_t for t in range(nticks + 1)]
        if not violated:
            r = ref.bound_radius(sides, case.gtype)
            for p in traj:                               # no two bounding spheres touch at any tick of a clean chunk
                d = np.hypot(p[:, None, 0] - p[None, :, 0], p[:, None, 2] - p[None, :, 2]) - r[:, None] - r[None, :]
                np.fill_diagonal(d, np.inf)
                assert d.min() > 0
        return violated, traj[-1]

    p0 = w.download(B.POS).astype(np.float64)
    v, p1 = run_chunk(6, p0)
    assert not v
    w.chunk_commit(6, refresh_zones=True)
    got = w.download(B.POS).astype(np.float64)
    assert np.abs(got - p1).max() <= 64 * np.finfo(dtype).eps * np.abs(p1).max()
    before = w.download(B.STATE)
    v, _ = run_chunk(12, got)
    assert v
    w.chunk_rollback()
    assert np.array_equal(w.download(B.STATE), before)
    v, p2 = run_chunk(6, got)
    assert not v
    w.chunk_commit(6, refresh_zones=True)
    assert np.abs(w.download(B.POS).astype(np.float64) - p2).max() <= 64 * np.finfo(dtype).eps * np.abs(p2).max()
    st = w.collision_stats()
    assert st["fast_ticks"] == 12 and st["rebuilds"] >= 3
    w.close()
