"""The oracle in worlds that are not y-up, judged without the oracle's own code: rigid-body dynamics commute with a rotation
of the world, so the oracle run on rotate_scene(S), rotated back, must equal the oracle run on S up to rounding.  A y-up
assumption anywhere in it (gravity, plane, AABBs, contact frames) shows as a defect of 1e-2 or more within a few ticks.

Scenes: the float64 fuzz scenes of tests/test_gpu_fuzz.py::_scene below seed 24 (twelve: eight of boxes and spheres, four with
convex hulls in the cluster -- the CPU suite's build provides hull.build -- eight with static boxes), the seed's own solver and
surface parameters except mu, 40 ticks, in z_up, x_up, down and tilted against y_up.

Friction under QuickStep is left out on purpose.  dPlaneSpace builds a contact's tangent basis from the world's axes, and 8-30
SOR sweeps do not converge to the (basis-independent) solution, so with 0 < mu the oracle's defect is of order 1 m/s from the
first tick: ODE's behaviour, not a bug.  What is used: mu = 0 under both steppers, and mu = inf under the exact stepper, where
the solution is unique.

Measured here (max over pos / lvel / avel, the twelve seeds, the four rotations, after 40 ticks), and the bounds asserted --
100 x the measured maximum of each class, because the defect grows with every contact event (the test prints each case's figure):

    class               measured    bound
    QuickStep, mu = 0   7.9e-10     7.9e-8
    exact,     mu = 0   5.5e-9      5.5e-7
    exact,     mu = inf 3.6e-7      3.6e-5      (seeds 18, 20 and 4, in that order: the conditioning drives it)

One finding, kept as named cases (SPHERE_HULL_GATED).  Under `tilted` the hull seeds 6, 12 and 18 differ from y_up by metres.
The cause is the sphere-hull collider, not an axis assumption: it takes the largest face-plane distance for the distance of
the sphere's centre from the hull, which over an edge or a vertex of a coarse hull (12-150 random points) is far less than
the true distance, so it reports contacts between geoms that are well apart -- and whether it is asked at all is decided by
the AABB test in front of it.  AABBs are invariant under the signed permutations and not under a general rotation: at tick 13
of seed 6 the tilted world has a sphere-hull contact the y-up world's AABBs filtered out.  With spheres and hulls kept from
meeting (category bits; nothing else changed) the same seeds commute with `tilted` like every other, which is how those three
cases run here.  Contact counts are compared with n_contacts(); n_body_pairs() counts AABB pairs and differs under `tilted`."""
import functools

import numpy as np
import pytest

import rotated_worlds as rw
from test_gpu_fuzz import _scene

TICKS = 40
SEEDS = tuple(range(0, 24, 2))
CLASSES = {"quick-mu0": (False, 0.0), "exact-mu0": (True, 0.0), "exact-muinf": (True, float("inf"))}
MEASURED = {"quick-mu0": 7.9e-10, "exact-mu0": 5.5e-9, "exact-muinf": 3.6e-7}
BOUND = {k: 100.0 * v for k, v in MEASURED.items()}
SPHERE_HULL_GATED = {(6, "tilted"), (12, "tilted"), (18, "tilted")}


@functools.lru_cache(maxsize=None)
def _fuzz_scene(seed):
    return _scene(seed)


@functools.lru_cache(maxsize=None)
def _run(seed, cls, name, sphere_hull=True):
    """-> (state in the y-up frame, contacts, body pairs at the last tick)"""
    scene, dtype, p, _ = _fuzz_scene(seed)
    exact, mu = CLASSES[cls]
    sc, g = rw.rotate_scene(scene, name, dtype)
    ow = rw.oracle_world(sc, dtype, dict(p, mu=mu), g, exact=exact, sphere_hull=sphere_hull)
    ow.run(rw.H, TICKS)
    out = (rw.rotate_back(ow.state(), name), ow.n_contacts(), ow.n_body_pairs())
    ow.close()
    return out


def defect(seed, cls, name):
    sphere_hull = (seed, name) not in SPHERE_HULL_GATED
    got, nc, _ = _run(seed, cls, name, sphere_hull)
    ref, nc0, _ = _run(seed, cls, "y_up", sphere_hull)
    for a in got:
        assert np.all(np.isfinite(a))
    return max(float(np.max(np.abs(got[k] - ref[k]))) for k in (0, 2, 3)), nc, nc0


def test_the_orientations_are_the_rotations_the_table_names():
    for name in rw.ORIENTATIONS:
        R = rw.matrix(name)
        Q = rw.quat_matrix(rw.QUATS[name])
        assert abs(np.linalg.det(R) - 1.0) < 1e-15 and np.max(np.abs(R @ R.T - np.eye(3))) < 1e-15
        if name != "tilted":
            assert np.array_equal(R, Q) and set(np.abs(R).ravel()) == {0.0, 1.0}        # a signed permutation, exactly
    g = 9.8
    assert rw.rotate_gravity("y_up") == (0.0, -g, 0.0) and rw.rotate_gravity("z_up") == (0.0, 0.0, -g)
    assert rw.rotate_gravity("x_up") == (-g, 0.0, 0.0) and rw.rotate_gravity("down") == (0.0, g, 0.0)
    assert rw.rotate_plane("z_up", (0.0, 1.0, 0.0, 0.25)) == (0.0, 0.0, 1.0, 0.25)
    assert rw.rotate_plane("down", (0.0, 1.0, 0.0, 0.25)) == (0.0, -1.0, 0.0, 0.25)
    assert rw.rotate_vectors("z_up", [1.0, 2.0, 3.0]).tolist() == [3.0, 1.0, 2.0]          # x -> y -> z -> x
    assert rw.rotate_vectors("x_up", [1.0, 2.0, 3.0]).tolist() == [2.0, 3.0, 1.0]
    ax = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    T = rw.matrix("tilted")
    assert np.max(np.abs(T @ ax - ax)) < 1e-15 and abs(np.trace(T) - (1 + 2 * np.cos(np.radians(50.0)))) < 1e-15
    assert min(np.min(np.abs(T)), 1 - np.max(np.abs(T))) > 0.05                            # nothing axis-aligned


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", rw.ORIENTATIONS)
def test_rotate_scene_gives_images_in_the_worlds_precision(name, dtype):
    scene = _fuzz_scene(2 if dtype == "float64" else 5)[0]
    assert scene.pos.dtype == np.dtype(dtype) and scene.static_boxes
    sc, g = rw.rotate_scene(scene, name, dtype)
    R = rw.matrix(name)
    eps = float(np.finfo(dtype).eps)
    for f in ("pos", "lvel", "avel"):
        a, b = getattr(scene, f).astype(np.float64), getattr(sc, f)
        assert b.dtype == np.dtype(dtype)
        if name == "tilted":
            assert np.max(np.abs(b - a @ R.T)) <= 4 * eps * np.max(np.abs(a))
        else:
            assert np.array_equal(b.astype(np.float64), a @ R.T)                 # exact images: components moved and negated
    for f in ("mass", "inertia", "sides", "gtype"):
        assert np.array_equal(getattr(sc, f), getattr(scene, f))
    # body-to-world matrices: R times the old ones
    for i in (0, scene.n - 1):
        assert np.max(np.abs(rw.quat_matrix(sc.quat[i]) - R @ rw.quat_matrix(scene.quat[i]))) < (1e-6 if dtype == "float32" else 1e-15)
    for (sz, at, M), (sz0, at0, M0) in zip(sc.static_boxes, scene.static_boxes):
        assert tuple(sz) == tuple(sz0)
        assert np.max(np.abs(np.array(at) - R @ np.array(at0))) < 1e-5
        M, M0 = np.array(M).reshape(3, 4), np.array(M0).reshape(3, 4)
        assert np.max(np.abs(M[:, :3] - R @ M0[:, :3])) < 1e-6 and not M[:, 3].any()
    # what the device and the oracle are handed is representable in the world's precision
    for v in (*g, *sc.plane, *(c for b in sc.static_boxes for c in (*b[1], *b[2]))):
        assert float(np.dtype(dtype).type(v)) == v
    back = rw.rotate_back((sc.pos, sc.quat, sc.lvel, sc.avel), name)
    for k, (a, b) in enumerate(zip(back, (scene.pos, scene.quat, scene.lvel, scene.avel))):
        if name != "tilted" and k != 1:
            assert np.array_equal(a, b)
        else:
            assert np.max(np.abs(a - b)) <= 8 * eps * max(1.0, np.max(np.abs(b)))


def test_every_scene_is_in_contact_and_some_have_static_boxes():
    """otherwise the equivariance below would prove free flight only"""
    with_statics = with_hulls = 0
    for seed in SEEDS:
        scene, dtype, _, _ = _fuzz_scene(seed)
        assert dtype == "float64"
        with_statics += bool(scene.static_boxes)
        with_hulls += scene.hull_points is not None
        for cls in CLASSES:
            _, nc, npairs = _run(seed, cls, "y_up")
            assert nc > 0 and npairs > 0, (seed, cls, nc, npairs)
    assert with_statics >= 4 and with_hulls >= 1


@pytest.mark.parametrize("name", rw.ROTATED)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("cls", list(CLASSES))
def test_the_oracle_commutes_with_a_rotation_of_the_world(cls, seed, name):
    d, nc, nc0 = defect(seed, cls, name)
    print(f"{cls} seed {seed} {name}: defect {d:.3e}, contacts {nc}")
    assert nc == nc0
    assert d <= BOUND[cls], (cls, seed, name, d)
