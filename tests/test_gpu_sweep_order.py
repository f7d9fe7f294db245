"""integrate_free walks the tiles in alternating directions from one contact-free launch to the next (csrc/dmx_sweep.hpp):
workgroup b works on tile group sweep_block(b, grid, rev), on a grid rounded up to a multiple of 8 workgroups.  Which workgroup
steps a body must not change a single bit, and every body must be stepped exactly once per tick: a body stepped twice, or
left out, in any of the ticks differs from the CPU oracle, with which every case is compared by value AND on the bit patterns.
The shapes are the smallest at which the remap can go wrong: 1, 7, 8, 9, 16 and 17 workgroups of 256 bodies, each exact and
37 bodies short of a full workgroup (which also gives counts that are no multiple of the 64-body tile); 6 ticks in calls of
1, 2 and 3, so that both directions and both slabs of the chunk's ping-pong take part."""
import numpy as np
import pytest

from __graft_entry__ import load_package

pkg = load_package()
pytestmark = pytest.mark.gpu

H = 1.0 / 60.0
MASKS = [3, 0]
DTYPES = ["float32", "float64"]
BLOCKS = [1, 7, 8, 9, 16, 17]
COUNTS = [256 * k - short for k in BLOCKS for short in (0, 37)]
CALLS = (1, 2, 3)
NX, NZ = 64, 68                     # 4352 bodies = 17 workgroups


def _orc(dtype):
    from oracle.orc_ctypes import Oracle
    return Oracle(dtype)


def _oracle_world(orc, scene):
    ow = orc.world()
    ow.add_boxes(scene.pos, scene.quat, scene.lvel, scene.avel, scene.mass[:, 0], scene.inertia, scene.sides)
    return ow


def _gpu_world(scene, dtype, mask, setup=None, slots=None):
    w = pkg.BatchWorld(scene.n if slots is None else slots, dtype=dtype)
    w.set_elision(mask)
    if setup:
        setup(w)
    w.load_scene(scene)
    return w


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(got, ref, what=""):
    for name, a, b in zip(("pos", "quat", "lvel", "avel"), got, ref):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert np.array_equal(a, b), f"{what}{name}: values differ, max abs diff {np.max(np.abs(a - b))}"
        diff = _bits(a) != _bits(b)
        assert not diff.any(), f"{what}{name}: {int(diff.sum())} components differ in their bits (first at {np.argwhere(diff)[0]})"


def _step_calls(w):
    for k in CALLS:
        w.step(H, k)
    w.synchronize()


def _scene(dtype, box_mass):
    # the reference's AddBody (m = 1, I = identity) or per-body box masses; spinning, dropped at rest, far apart: no contacts
    return pkg.scenes.box_grid(NX, NZ, seed=17, spin=True, box_mass=box_mass, plane=False).astype(dtype)


# the oracle's state after the 6 ticks, once per scene: free bodies do not act on one another, so the first n bodies of the
# full scene after 6 ticks are the n-body scene after 6 ticks (the GPU runs assert that no pair was ever met)
_REF = {}


def _reference(dtype, box_mass):
    key = (dtype, box_mass)
    if key not in _REF:
        scene = _scene(dtype, box_mass)
        ow = _oracle_world(_orc(dtype), scene)
        ow.run(H, sum(CALLS))
        ref = ow.state()
        for a in ref:
            a.setflags(write=False)
        _REF[key] = (scene, ref)
    return _REF[key]


def _first(ref, n):
    return tuple(a[:n] for a in ref)


# 1. every grid size at which the remap can go wrong, exact and ragged
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_body_counts_around_the_group_of_eight(dtype, n, mask):
    full, ref = _reference(dtype, False)
    w = _gpu_world(full.slice(0, n), dtype, mask)
    _step_calls(w)
    _same_bits(w.state(), _first(ref, n))
    assert w.collision_stats()["pair_ticks"] == 0
    w.close()


# 2. per-body mass and anisotropic inertia: the constants are loaded, avel changes every tick (every component is stored)
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_per_body_constants(dtype, mask):
    full, ref = _reference(dtype, True)
    n = 256 * 9 - 37
    w = _gpu_world(full.slice(0, n), dtype, mask)
    _step_calls(w)
    _same_bits(w.state(), _first(ref, n))
    w.close()


# 3. external force on a few bodies (first and last workgroup among them): the launch that consumes it clears it
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_external_force_on_a_few_bodies(dtype, mask):
    full, _ = _reference(dtype, False)
    n = 256 * 9 - 37
    scene = full.slice(0, n)
    force = np.zeros((n, 3), dtype)
    force[[0, 255, 256, 64 * 17 + 5, 2048, n - 1], 0] = 1.5
    force[[3, 256 * 8 + 200], 1] = -0.75
    orc = _orc(dtype)
    ow = _oracle_world(orc, scene)
    for b in np.where(force.any(axis=1))[0]:
        orc.lib.orc_body_add_force(ow.w, int(b), *[float(x) for x in force[b]])
    ow.run(H, sum(CALLS))
    w = _gpu_world(scene, dtype, mask)
    w.upload(pkg.batch.FORCE, force)
    _step_calls(w)
    _same_bits(w.state(), ow.state())
    assert np.array_equal(w.download(pkg.batch.FORCE), np.zeros_like(force))
    w.close()


# 4. three ticks per launch, no collision proof: every launch in place, calls of 1, 2 and 3 ticks are one launch each
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_three_ticks_per_launch_without_the_collision_proof(dtype, mask):
    full, ref = _reference(dtype, False)
    n = 256 * 17 - 37
    w = _gpu_world(full.slice(0, n), dtype, mask, setup=lambda w: (w.set_ticks_per_launch(3), w.set_body_collisions(False)))
    _step_calls(w)
    _same_bits(w.state(), _first(ref, n))
    w.close()


# 5. fewer active bodies than slots: the grid is sized by the active count (9 workgroups, rounded up to 16), the reversed sweep's
#    surplus workgroups land on slots behind it -- which must keep their bits
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_slots_behind_the_active_count_keep_their_bits(dtype, mask):
    full, ref = _reference(dtype, False)
    slots, active = 256 * 17 - 37, 256 * 8 + 100
    scene = full.slice(0, slots)
    w = _gpu_world(scene, dtype, mask)
    w.set_active_count(active)
    before = w.state()
    _step_calls(w)
    got = w.state()
    _same_bits(tuple(a[:active] for a in got), _first(ref, active), what="active: ")
    _same_bits(tuple(a[active:] for a in got), tuple(a[active:] for a in before), what="behind the active count: ")
    _same_bits(tuple(a[active:] for a in got), (scene.pos[active:], scene.quat[active:], scene.lvel[active:], scene.avel[active:]),
               what="behind the active count, against the scene: ")
    w.close()


# 6. a mid-air collision rolls a chunk back (the scene of test_gpu_elision's test_rollback_and_replay): the replayed launches
#    run in whatever direction the bit has reached
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_rollback_and_replay(dtype, mask):
    scene = pkg.scenes.box_grid(16, 16, seed=13, y_range=(10.0, 12.0), spin=True, box_mass=False, plane=False).astype(dtype)
    rng = np.random.default_rng(5)
    movers = rng.random(scene.n) < 0.4
    scene.lvel[movers, 0] = rng.uniform(-3.0, 3.0, int(movers.sum()))
    scene.lvel[movers, 2] = rng.uniform(-3.0, 3.0, int(movers.sum()))
    ow = _oracle_world(_orc(dtype), scene)
    ow.run(H, 150)
    w = _gpu_world(scene, dtype, mask)
    for k in (7, 50, 1, 92):
        w.step(H, k)
    w.synchronize()
    _same_bits(w.state(), ow.state())
    assert w.collision_stats()["pair_ticks"] > 0, "the scene is meant to collide in mid-air"
    w.close()
