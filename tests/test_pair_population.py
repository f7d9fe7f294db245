"""The populations of tests/pair_population.py through the oracle alone (no GPU), in float64 and float32: the COVERAGE CONDITIONS --
conditions on the inputs of a one-tick device-against-oracle comparison, not measurements of anything under test.  A generator that misses
one is changed; the bound is not.  DESIGN.md section 5 carries the table these tests print.  Last: one tick of every population in
float32 against the same tick in float64 (pair_population.precision_tick), the numbers tests/test_gpu_precision_pairs.py holds the
device to."""
import numpy as np
import pytest

import pair_population as pp

DTYPES = ["float64", "float32"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_box_box_covers_faces_edges_culling_and_near_misses(dtype):
    pop = pp.box_box()
    a = pp.analyse(pop, dtype)
    n = a["pairs"]
    assert n == 3072
    # the first contact's normal: along a face normal of body 1 (the lower slot), of body 2, or neither (an edge-edge contact)
    first = {}
    for j in a["joints"]:
        first.setdefault(int(pop.cell[j[0]]), j)
    R = _rotations(pop, dtype)
    f1 = f2 = edge = 0
    for c, j in first.items():
        nrm = np.asarray(j[3], float)
        d1 = np.max(np.abs(R[2 * c].T @ nrm)); d2 = np.max(np.abs(R[2 * c + 1].T @ nrm))
        tol = 1e-5 if dtype == "float32" else 1e-12
        if d1 > 1 - tol and d1 >= d2:
            f1 += 1
        elif d2 > 1 - tol:
            f2 += 1
        else:
            edge += 1
    # more than 4 clipped points: cull_points runs when max_contacts is 4 and the unculled count (max_contacts 8) exceeds it
    many = int((a["per_cell"] > 4).sum())
    print(f"COVERAGE box_box {dtype}: pairs {n} colliding {a['colliding']} ({100.0 * a['colliding'] / n:.1f} %) "
          f"face1/face2/edge {f1}/{f2}/{edge} over-4-points {many} near-miss {a['near_miss']} contacts {a['contacts']}")
    assert a["colliding"] >= n // 2
    assert f1 >= 500 and f2 >= 500 and edge >= 250
    assert many >= 200
    assert a["near_miss"] >= 500


def _rotations(pop, dtype):
    orc, ow, sc = pp.oracle_world(pop, dtype)
    return pp.world_poses(orc, ow, sc.n)[:, 3:].reshape(-1, 3, 4)[:, :, :3].astype(float)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["sphere_box", "sphere_sphere"])
def test_sphere_populations(name, dtype):
    pop = pp.get(name)
    a = pp.analyse(pop, dtype)
    print(f"COVERAGE {name} {dtype}: pairs {a['pairs']} colliding {a['colliding']} near-miss {a['near_miss']} contacts {a['contacts']}")
    assert a["pairs"] == 1024 + 128
    # the tail: 64 centres inside the other geom and 64 degenerate poses, every one a contact
    assert np.all(a["per_cell"][1024:] == 1)
    assert a["colliding"] >= 1024 // 2


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", pp.HULL_SHAPES)
@pytest.mark.parametrize("name", ["hull_hull", "sphere_hull", "box_hull"])
def test_hull_populations(name, shape, dtype):
    pop = pp.get(name, shape)
    a = pp.analyse(pop, dtype)
    print(f"COVERAGE {name}[{shape}] {dtype}: pairs {a['pairs']} colliding {a['colliding']} near-miss {a['near_miss']} at-cap {a['at_cap']} "
          f"contacts {a['contacts']}")
    assert a["pairs"] == 1024
    assert a["colliding"] >= 200
    assert a["near_miss"] >= 100                 # AABBs overlap, no contact: the pairs the filters must let through unharmed
    # the 8-contact cap, for hulls of >= 63 points (the sphere-hull collider makes one contact at most: no cap to reach)
    if name != "sphere_hull" and len(pop.hull.points) >= 63:
        assert a["at_cap"] >= 100


@pytest.mark.parametrize("dtype", DTYPES)
def test_on_plane(dtype):
    pop = pp.on_plane()
    a = pp.analyse(pop, dtype)
    print(f"COVERAGE on_plane {dtype}: bodies {a['bodies']} colliding {a['colliding']} contacts {a['contacts']}")
    assert a["bodies"] == 1024
    assert a["colliding"] >= 0.6 * a["bodies"]
    for cls in (pp.BOX, pp.SPHERE, pp.CONVEX):
        assert (a["per_cell"][pop.gtype == cls] > 0).sum() >= 100


@pytest.mark.parametrize("dtype", DTYPES)
def test_on_statics(dtype):
    pop = pp.on_statics()
    assert len(pop.static_boxes) == 64
    a = pp.analyse(pop, dtype)
    print(f"COVERAGE on_statics {dtype}: bodies {a['bodies']} colliding {a['colliding']} two-statics {a['two_statics']} over-8 {a['over_8']} "
          f"contacts {a['contacts']} aabb-marginal {a['aabb_marginal']}")
    assert a["bodies"] == 512
    assert a["colliding"] >= 0.6 * a["bodies"]
    assert a["two_statics"] >= 50
    assert a["over_8"] >= 20                     # more than the fused buffer's 8: these bodies fall back to the exact tick
    for cls in (pp.BOX, pp.SPHERE, pp.CONVEX):
        assert (a["per_cell"][pop.gtype == cls] > 0).sum() >= 50


@pytest.mark.parametrize("key", pp.ALL, ids=pp.pop_id)
def test_far_translation_keeps_the_shares(key):
    """float32 at (4 096, 0, -2 560) m: positions round to 0.25-0.5 mm; each population still collides as it does at the origin and
    still meets the conditions its kind has at the origin (contacts, near misses, the cap, two static boxes, more than 8 contacts)"""
    pop = pp.get(*key)
    near = pp.analyse(pop, "float32")
    a = pp.analyse(pop, "float32", shift=pp.FAR)
    print(f"COVERAGE far {pp.pop_id(key)}: colliding {near['colliding']} -> {a['colliding']}, contacts {near['contacts']} -> {a['contacts']}, "
          f"aabb-marginal {a['aabb_marginal']}")
    assert a["colliding"] >= 0.9 * near["colliding"]
    name = key[0]
    if name == "box_box":
        assert a["colliding"] >= a["pairs"] // 2 and a["near_miss"] >= 500 and int((a["per_cell"] > 4).sum()) >= 200
    elif name in ("sphere_box", "sphere_sphere"):
        assert np.all(a["per_cell"][1024:] == 1) and a["colliding"] >= 1024 // 2
    elif name in ("hull_hull", "sphere_hull", "box_hull"):
        assert a["colliding"] >= 200 and a["near_miss"] >= 100
        if name != "sphere_hull" and len(pop.hull.points) >= 63:
            assert a["at_cap"] >= 100
    elif name == "on_plane":
        assert a["colliding"] >= 0.6 * a["bodies"]
    else:
        assert a["colliding"] >= 0.6 * a["bodies"] and a["two_statics"] >= 50 and a["over_8"] >= 20


@pytest.mark.parametrize("far", [False, True], ids=["near", "far"])
@pytest.mark.parametrize("key", pp.ALL, ids=pp.pop_id)
def test_one_tick_in_float32_against_float64(key, far):
    """One tick through the float32 oracle against the float64 oracle on the same float32 values, cfm 1e-5 in both, near the origin and
    at FAR.  Cells whose contacts differ in count, slot or by more than the band (pp.precision_tick) are left out -- at most 8 % of a
    population's cells, or its generator is changed; on the rest the states agree within 4 x the maxima measured here (pp.TICK_MEASURED,
    per population class and place; this test prints what it measures), velocities in eps32 M_world / h, poses in eps32 M_world."""
    r = pp.precision_tick(key, far)
    share = r["not_comparable"] / r["cells"]
    print(f"PRECISION {pp.pop_id(key)} {'far' if far else 'near'}: M_world {r['m_world']:.0f} m; not comparable {r['not_comparable']} of {r['cells']} cells "
          f"({100 * share:.2f} %, {r['by_count']} by count); lvel / avel / pos / quat " + " / ".join(f"{v:.3g}" for v in r["dev"])
          + "; same-slot contacts pos / depth / normal " + " / ".join(f"{v:.3g}" for v in r["contact_dev"]))
    assert share <= pp.MAX_NOT_COMPARABLE, f"{pp.pop_id(key)}: {100 * share:.1f} % of the cells not comparable: change the generator"
    assert r["comparable"].sum() >= 0.5 * r["cells"]
    for a in r["state32"] + r["state64"]:
        assert np.all(np.isfinite(a))
    for name, got, tol in zip(("lvel", "avel", "pos", "quat"), r["dev"], pp.tick_tolerance(key[0], far)):
        assert got <= tol, f"{pp.pop_id(key)} {name}: float32 is {got:.3g} units from float64, tolerance {tol:.3g}"
