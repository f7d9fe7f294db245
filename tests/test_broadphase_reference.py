"""CPU checks of tests/bp_reference.py, the float64 restatement the device broadphase is pinned to: known answers worked by
hand, symmetries, the oracle's two broadphase modes against it, and the float32 emulation of the kernels' arithmetic that the
band constants come from.

Measured here (float32 emulation, no contraction, against the float64 reference on the same float32 inputs; 6 seeds of 2 000
tumbling boxes and mixed scenes with a cube and the teapot hull, each at the origin, 1 km and 8 km out):
  signed gaps     move by at most 0.54 eps M, M = max |coordinate| + 2 r_max; 13 of ~10^5 pairs are decided differently, the
                  widest at |gap| = 0.33 eps M.  K_BAND = 2 (bp_reference.py): twice the bound eps M that one rounding per
                  face at the coordinate's size allows a gap to move.
  safe radii      deviate by at most 0.062 eps (max |coordinate| + cell).  K_ZONE = 1: a 16x margin.
test_emulated_* re-measure both, print the figures and assert the margins.
"""
import numpy as np
import pytest

import bp_reference as ref
import bp_scenes as sc
from bp_reference import GEOM_BOX, GEOM_CONVEX, GEOM_NONE, GEOM_SPHERE


def _case_ref(case, dtype, class_pairs=None):
    """the reference's answer for a case whose numbers were rounded to dtype (unit quaternions renormalised in dtype, as an
    upload does)"""
    rd = lambda a: np.asarray(a, np.float64).astype(dtype)
    pos, sides = rd(case.pos), rd(case.sides)
    q = rd(case.quat)
    q = (q / np.sqrt((q * q).sum(1, keepdims=True))).astype(dtype)
    hull = None if case.hull is None else rd(case.hull)
    lo, hi = ref.aabbs(pos, q, sides, case.gtype, hull)
    slo, shi = ref.static_aabbs(case.statics, dtype)
    b = 0.0 if case.exact else ref.band(dtype, pos, sides, case.gtype, case.statics)
    blk = max(64, 2_000_000 // max(case.n, 1))
    return ref.pairs(lo, hi, case.gtype, case.n_active, class_pairs, slo, shi, band=b, block=blk), b


# ---- known answers --------------------------------------------------------------------------------------------------------
def _boxes(pos, sides, quat=None):
    n = len(pos)
    q = np.tile([1.0, 0, 0, 0], (n, 1)) if quat is None else np.asarray(quat, float)
    return ref.aabbs(np.asarray(pos, float), q, np.asarray(sides, float), np.full(n, GEOM_BOX, np.uint8))


def test_two_unit_boxes_touching_are_a_pair_and_apart_are_not():
    lo, hi = _boxes([[0, 0, 0], [1, 0, 0]], [[1, 1, 1]] * 2)
    assert np.array_equal(lo, [[-0.5, -0.5, -0.5], [0.5, -0.5, -0.5]]) and np.array_equal(hi, [[0.5, 0.5, 0.5], [1.5, 0.5, 0.5]])
    r = ref.pairs(lo, hi, [GEOM_BOX] * 2)
    assert ref.signed_gap(lo, hi, lo, hi)[0, 1] == 0.0 and r.pairs.tolist() == [[0, 1]] and r.involved.tolist() == [0, 1]
    lo, hi = _boxes([[0, 0, 0], [1 + 2.0 ** -10, 0, 0]], [[1, 1, 1]] * 2)
    r = ref.pairs(lo, hi, [GEOM_BOX] * 2)
    assert ref.signed_gap(lo, hi, lo, hi)[0, 1] == 2.0 ** -10 and len(r.pairs) == 0 and len(r.involved) == 0


def test_a_box_turned_45_degrees_about_y_is_sqrt2_wide():
    c, s = np.cos(np.pi / 8), np.sin(np.pi / 8)
    lo, hi = _boxes([[0, 0, 0], [1.2, 0, 0]], [[1, 1, 1]] * 2, quat=[[c, 0, s, 0], [1, 0, 0, 0]])
    assert np.allclose(hi[0], [np.sqrt(0.5), 0.5, np.sqrt(0.5)], atol=1e-15) and np.allclose(lo[0], -hi[0], atol=1e-15)
    # unturned the boxes are 0.2 apart; turned, box 0 reaches 0.7071 and overlaps box 1's face at 0.7
    assert ref.signed_gap(lo, hi, lo, hi)[0, 1] == pytest.approx(0.7 - np.sqrt(0.5), abs=1e-15)
    assert ref.pairs(lo, hi, [GEOM_BOX] * 2).pairs.tolist() == [[0, 1]]


def test_sphere_and_hull_boxes():
    cube = sc.cube_hull(1.0)
    c, s = np.cos(np.pi / 8), np.sin(np.pi / 8)
    pos = np.array([[0.0, 0, 0], [3.0, 0, 0], [3.0, 2.0, 0]])
    quat = np.array([[1.0, 0, 0, 0], [c, 0, 0, s], [1.0, 0, 0, 0]])          # the hull turned 45 degrees about z
    sides = np.array([[0.25, 9, 9], [np.sqrt(0.75), 0, 0], [np.sqrt(0.75), 0, 0]])
    g = np.array([GEOM_SPHERE, GEOM_CONVEX, GEOM_CONVEX], np.uint8)
    lo, hi = ref.aabbs(pos, quat, sides, g, cube)
    assert np.array_equal(lo[0], [-0.25] * 3) and np.array_equal(hi[0], [0.25] * 3)            # a sphere ignores sides[1:]
    assert np.allclose(hi[1] - pos[1], [np.sqrt(0.5), np.sqrt(0.5), 0.5], atol=1e-15)         # the points' bounds ...
    assert np.all(hi[1] - pos[1] < np.sqrt(0.75) - 0.1)                                       # ... not the bounding sphere's box
    assert np.allclose(hi[2] - pos[2], [0.5] * 3, atol=1e-15)
    # the two hulls: y faces at 0.7071 and 1.5 -- apart, though their bounding spheres (r = 0.866) overlap
    r = ref.pairs(lo, hi, g)
    assert len(r.pairs) == 0
    assert ref.signed_gap(lo, hi, lo, hi)[1, 2] == pytest.approx(1.5 - np.sqrt(0.5), abs=1e-15)


def test_class_pairs_ghosts_none_slots_and_static_boxes():
    pos = np.array([[0.0, 0, 0], [0.5, 0, 0], [0.0, 0.5, 0], [0.5, 0.5, 0], [10.0, 0, 0], [0.2, 0.2, 0.2], [20.0, 0, 0], [20.2, 0, 0]])
    n = len(pos)
    sides = np.full((n, 3), 1.0); sides[1, 0] = 0.5
    g = np.array([GEOM_BOX, GEOM_SPHERE, GEOM_BOX, GEOM_BOX, GEOM_BOX, GEOM_NONE, GEOM_BOX, GEOM_BOX], np.uint8)
    lo, hi = ref.aabbs(pos, np.tile([1.0, 0, 0, 0], (n, 1)), sides, g)
    assert ref.pairs(lo, hi, g).pair_set() == {(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (6, 7)}
    off = ref.pairs(lo, hi, g, class_pairs=ref.class_matrix([(GEOM_BOX, GEOM_SPHERE)]))
    assert off.pair_set() == {(0, 2), (0, 3), (2, 3), (6, 7)} and off.involved.tolist() == [0, 2, 3, 6, 7]
    gh = ref.pairs(lo, hi, g, n_active=4)                  # slots 4.. are ghosts: 6-7 overlap one another and appear nowhere
    assert gh.pair_set() == {(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)} and gh.cross == set()
    gh = ref.pairs(lo, hi, g, n_active=2)
    assert gh.pair_set() == {(0, 1)} and gh.cross == {(0, 2), (0, 3), (1, 2), (1, 3)} and gh.involved.tolist() == [0, 1]
    slo, shi = ref.static_aabbs([((2.0, 1.0, 2.0), (10.0, -1.0, 0.0), sc.IDENT_R12)], "float64")        # its top face at y = -0.5
    st = ref.pairs(lo, hi, g, static_lo=slo, static_hi=shi)
    assert st.static_gap[4, 0] == 0.0 and 4 in st.involved.tolist() and st.static_gap[5, 0] == np.inf
    assert st.involved.tolist() == [0, 1, 2, 3, 4, 6, 7]


def test_a_safe_zone_worked_on_paper():
    # three spheres r = 0.5 on the x axis at 0, 3, 10 and a 1 x 1 x 1 box (r = 0.866) at z = 2 above the first (y is ignored)
    pos = np.array([[0.0, 0, 0], [3.0, 5.0, 0], [10.0, 0, 0], [0.0, 9.0, 2.0]])
    sides = np.array([[0.5, 0, 0], [0.5, 0, 0], [0.5, 0, 0], [1.0, 1.0, 1.0]])
    g = np.array([GEOM_SPHERE] * 3 + [GEOM_BOX], np.uint8)
    rb = np.sqrt(0.75)
    safe, cell = ref.safe_zones(pos, sides, g)
    assert cell == pytest.approx(2.5 * rb)
    cap_s, cap_b = cell - 0.5 - rb, cell - rb - rb                # 0.799, 0.433
    assert safe[0] == pytest.approx(0.5 * min(cap_s, 2.0 - 0.5 - rb))          # the box is nearest: 0.634 < cap
    assert safe[1] == pytest.approx(0.5 * cap_s)                               # nearest sphere 2.0 away: the cap binds
    assert safe[2] == pytest.approx(0.5 * cap_s)
    assert safe[3] == pytest.approx(0.5 * cap_b)
    # sphere-box switched off: the spheres see spheres only (cap = cell - 2 r), the box nobody (cap from its own class)
    safe, _ = ref.safe_zones(pos, sides, g, ref.class_matrix([(GEOM_SPHERE, GEOM_BOX)]))
    assert safe[0] == pytest.approx(0.5 * min(cell - 1.0, 2.0)) and safe[3] == pytest.approx(0.5 * cap_b)
    # box-box off as well: nothing collides with the box, its zone is unbounded
    safe, _ = ref.safe_zones(pos, sides, g, ref.class_matrix([(GEOM_SPHERE, GEOM_BOX), (GEOM_BOX, GEOM_BOX)]))
    assert safe[3] == np.inf
    # touching bounding spheres: zero; overlapping: negative
    pos[1] = (1.0, 0, 0)
    assert ref.safe_zones(pos, sides, g)[0][1] == 0.0
    pos[1] = (0.5, 0, 0)
    assert ref.safe_zones(pos, sides, g)[0][1] == -0.25


# ---- symmetries -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [lambda: sc.tumbling_boxes(300, 11), lambda: sc.mixed(300, 12, sc.cube_hull(), none_share=0.1)])
def test_gap_is_symmetric_and_pairs_follow_a_permutation(make):
    case = make()
    lo, hi = ref.aabbs(case.pos, case.quat, case.sides, case.gtype, case.hull)
    gap = ref.signed_gap(lo, hi, lo, hi)
    assert np.array_equal(gap, gap.T)
    base = ref.pairs(lo, hi, case.gtype)
    assert len(base.pairs) > 300
    assert np.all(base.pairs[:, 0] < base.pairs[:, 1])
    assert sorted(map(tuple, base.pairs.tolist())) == list(map(tuple, base.pairs.tolist()))
    perm = np.random.default_rng(1).permutation(case.n)                    # new slot k holds old body perm[k]
    lo2, hi2 = ref.aabbs(case.pos[perm], case.quat[perm], case.sides[perm], case.gtype[perm], case.hull)
    got = ref.pairs(lo2, hi2, case.gtype[perm])
    back = {tuple(sorted((int(perm[i]), int(perm[j])))) for i, j in got.pairs}
    assert back == base.pair_set()
    assert sorted(perm[got.involved].tolist()) == base.involved.tolist()
    z1, _ = ref.safe_zones(case.pos, case.sides, case.gtype)
    z2, _ = ref.safe_zones(case.pos[perm], case.sides[perm], case.gtype[perm])
    assert np.array_equal(z1[perm], z2)


# ---- the oracle's pair search -----------------------------------------------------------------------------------------------
def _oracle_scene(kind, seed):
    if kind == "boxes":
        return sc.tumbling_boxes(600, seed)
    if kind == "spheres":
        c = sc.tumbling_boxes(600, seed, extent=11.0)
        c.gtype[:] = GEOM_SPHERE
        c.sides[:, 0] *= 0.5
        return c
    c = sc.mixed(300, seed, sc.teapot_hull(), extent=9.0)
    c.gtype[:] = GEOM_CONVEX
    c.sides[:, 0] = sc.hull_radius(c.hull)
    return c


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("kind,seed", [("boxes", 21), ("spheres", 22), ("hulls", 23)])
def test_oracle_pair_count_equals_the_reference(dtype, mode, kind, seed):
    """n_body_pairs() after a tick = the reference's count on the poses the oracle collided (the tick collides, then steps:
    the poses before it).  A difference would have to lie inside the band; these seeds leave the band empty, so: equal."""
    from oracle.orc_ctypes import Oracle
    case = _oracle_scene(kind, seed)
    orc = Oracle(dtype)
    ow = orc.world(gravity=(0.0, 0.0, 0.0))
    orc.lib.orc_world_set_broadphase(ow.w, mode)
    n = case.n
    z3, one = np.zeros((n, 3)), np.ones(n)
    if kind == "boxes":
        ow.add_boxes(case.pos, case.quat, z3, z3, one, np.ones((n, 3)), case.sides)
    elif kind == "spheres":
        ow.add_spheres(case.pos, case.quat, z3, z3, one, np.ones((n, 3)), case.sides[:, 0])
    else:
        ow.set_hull(case.hull)
        ow.add_convex(case.pos, case.quat, z3, z3, one, np.ones((n, 3)))
    pos, quat, _, _ = ow.state()
    ow.tick(1.0 / 60.0)
    sides = case.sides.astype(dtype)
    hull = None if case.hull is None else case.hull.astype(dtype)
    lo, hi = ref.aabbs(pos, quat, sides, case.gtype, hull)
    b = ref.band(dtype, pos, sides, case.gtype)
    r = ref.pairs(lo, hi, case.gtype, band=b)
    assert len(r.near) == 0, f"seed leaves {len(r.near)} pairs inside the band {b:.3g}: choose another"
    assert len(r.pairs) > 2 * n // 3
    assert ow.n_body_pairs() == len(r.pairs)
    ow.close()


# ---- the band constants: the kernels' arithmetic emulated in float32 ---------------------------------------------------------
def _emulation_scenes():
    out = []
    for seed in range(6):
        b = sc.tumbling_boxes(2000, 100 + seed)
        out += [b, b.moved((1000.0, 0, 1000.0)), b.moved((8000.0, 0, -8000.0))]
    for hull, name in ((sc.cube_hull(), "cube"), (sc.teapot_hull(), "teapot")):
        m = sc.mixed(400, 7, hull, name=name)
        out += [m, m.moved((-1000.0, 0, 1000.0)), m.moved((-8000.0, 0, 8000.0))]
    return out


def test_emulated_aabbs_decide_like_the_reference_outside_half_the_band():
    """float32 body_aabb / wave_hull_aabb against the float64 reference on the same float32 inputs, in units of eps M with
    M = max |coordinate| + 2 r_max: the worst deviation of a signed gap near zero, and the largest |gap| of a pair the two decide
    differently.  Each face is rounded once at the size of the coordinate (half an ulp, at most eps M / 2), so a gap -- a
    difference of two faces -- moves by at most about eps M: K_BAND = 2 is twice that bound, and the assertion keeps the measured
    deviation inside half the band."""
    f, eps = np.float32, float(np.finfo(np.float32).eps)
    worst_dev, worst_flip, flips = 0.0, 0.0, 0
    for case in _emulation_scenes():
        pos, sides, hull = case.pos.astype(f), case.sides.astype(f), None if case.hull is None else case.hull.astype(f)
        q = case.quat.astype(f)
        q = (q / np.sqrt((q * q).sum(1, keepdims=True))).astype(f)
        lo, hi = ref.aabbs(pos, q, sides, case.gtype, hull)
        elo, ehi = ref.emulated_aabbs(pos, q, sides, case.gtype, hull)
        M = float(np.abs(pos).max()) + 2.0 * float(ref.bound_radius(sides, case.gtype).max())
        gap = ref.signed_gap(lo, hi, lo, hi)
        egap = ref.signed_gap(elo, ehi, elo, ehi).astype(np.float64)         # (the device compares faces; their difference is the same test)
        close = np.triu(np.abs(gap) < 0.05, 1)
        worst_dev = max(worst_dev, float(np.abs(egap - gap)[close].max() / (eps * M)))
        flip = close & ((gap <= 0) != (ehi[:, None, :] >= elo[None, :, :]).all(2) & (ehi[None, :, :] >= elo[:, None, :]).all(2))
        flips += int(flip.sum())
        if flip.any():
            worst_flip = max(worst_flip, float(np.abs(gap[flip]).max() / (eps * M)))
    print(f"worst gap deviation {worst_dev:.3f} eps M; {flips} pairs decided differently, the widest at |gap| = {worst_flip:.3f} eps M")
    assert worst_flip <= worst_dev <= ref.K_BAND / 2.0


def test_emulated_safe_zones_stay_inside_a_quarter_of_the_tolerance():
    """float32 bp_safe_zone arithmetic against safe_zones(): worst deviation in units of eps (max |coordinate| + cell)"""
    f, eps = np.float32, float(np.finfo(np.float32).eps)
    worst = 0.0
    for case in _emulation_scenes():
        k = slice(0, 700)
        pos, sides, g = case.pos[k].astype(f), case.sides[k].astype(f), case.gtype[k]
        for cp in (None, ref.class_matrix([(GEOM_BOX, GEOM_BOX)]), ref.class_matrix([(GEOM_CONVEX, GEOM_CONVEX), (GEOM_SPHERE, GEOM_BOX)])):
            want, cell = ref.safe_zones(pos, sides, g, cp)
            got, _ = ref.emulated_safe_zones(pos, sides, g, cp)
            fin = np.isfinite(want)
            assert np.array_equal(fin, np.isfinite(got))
            if fin.any():
                worst = max(worst, float(np.abs(got[fin] - want[fin]).max() / (eps * (np.abs(pos).max() + cell))))
    print("worst zone deviation / (eps (M + cell)):", worst)
    assert worst <= ref.K_ZONE / 4.0


# ---- the device test's seeded scenes satisfy their band condition with the reference alone -----------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_seeded_scenes_leave_few_pairs_in_the_band(dtype):
    for case, _ in sc.random_pair_cases():
        r, b = _case_ref(case, dtype)
        npairs = len(r.pairs) + len(r.cross)
        share = len(r.near) / max(npairs, 1)
        print(f"{case.name:40s} {dtype} pairs {npairs:6d} per body {npairs / case.n:5.2f} band {b:.3g} in band {len(r.near)} ({100 * share:.3f} %)")
        assert 1.5 * case.n <= npairs <= 5 * case.n                      # 3 to 10 pairs per body
        # (three quarters of the device test's limit: its inputs are the downloaded ones, a quaternion's rounding away from these)
        assert share <= 0.75 * (0.001 if case.near_origin else 0.02), case.name
