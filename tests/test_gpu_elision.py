"""What integrate_free leaves out (dmxBatchSetElision: stores of components an in-place launch did not change, loads of
mass / inertia that are the same for every slot) must not change a single bit.  Every case runs with the default mask (3)
and with 0 (every load and store), and is compared with the CPU oracle by value (array_equal) AND on the bit patterns,
which is what tells -0.0 from +0.0."""
import numpy as np
import pytest

from __graft_entry__ import load_package

pkg = load_package()
pytestmark = pytest.mark.gpu

H = 1.0 / 60.0
MASKS = [3, 0]


def _orc(dtype):
    from oracle.orc_ctypes import Oracle
    return Oracle(dtype)


def _oracle_world(orc, scene):
    ow = orc.world()
    ow.add_boxes(scene.pos, scene.quat, scene.lvel, scene.avel, scene.mass[:, 0], scene.inertia, scene.sides)
    return ow


def _gpu_world(scene, dtype, mask, setup=None):
    w = pkg.BatchWorld(scene.n, dtype=dtype)
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
        assert a.dtype == b.dtype
        assert np.array_equal(a, b), f"{what}{name}: values differ, max abs diff {np.max(np.abs(a - b))}"
        diff = _bits(a) != _bits(b)
        assert not diff.any(), f"{what}{name}: {int(diff.sum())} components differ in their bits (first at {np.argwhere(diff)[0]})"


def _headline_scene(dtype, spin, nx=64, nz=32):
    # the reference's AddBody: m = 1, I = identity; dropped at rest
    return pkg.scenes.box_grid(nx, nz, seed=7, spin=spin, box_mass=False, plane=False).astype(dtype)


# 1. the headline's shape, in calls of 1, 7 and 150 ticks (chunks stay open across calls; the first launch of each is out of place)
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("per_call", [1, 7, 150])
@pytest.mark.parametrize("spin", [False, True])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_headline_shape(dtype, spin, per_call, mask):
    scene = _headline_scene(dtype, spin)
    ow = _oracle_world(_orc(dtype), scene)
    ow.run(H, 150)
    w = _gpu_world(scene, dtype, mask)
    done = 0
    while done < 150:
        k = min(per_call, 150 - done)
        w.step(H, k)
        done += k
    w.synchronize()
    _same_bits(w.state(), ow.state())
    assert w.collision_stats()["pair_ticks"] == 0
    w.close()


# 2. per-body constants, anisotropic inertia: avel changes every tick, the constants are loaded
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_per_body_constants(dtype, mask):
    scene = pkg.scenes.box_grid(64, 32, seed=3, spin=True, box_mass=True, plane=False).astype(dtype)
    ow = _oracle_world(_orc(dtype), scene)
    ow.run(H, 150)
    w = _gpu_world(scene, dtype, mask)
    w.step(H, 150)
    w.synchronize()
    _same_bits(w.state(), ow.state())
    w.close()


# 3. lateral velocity on whole 64-body tiles and on single lanes of other tiles: those wavefronts store, the rest do not
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_lateral_velocity_on_some_tiles_and_lanes(dtype, mask):
    scene = _headline_scene(dtype, spin=True)
    for tile in (1, 6, 31):
        scene.lvel[64 * tile:64 * tile + 64, 0] = 0.05
    for tile in (9, 20):
        scene.lvel[64 * tile:64 * tile + 64, 2] = -0.03
    for body in (5, 64 * 3 + 63, 64 * 12, 64 * 17 + 31):       # one lane of its wavefront
        scene.lvel[body, 0] = 0.04
        scene.lvel[body, 2] = 0.02
    scene.avel[64 * 25 + 7] = (0.0, 0.0, 0.0)
    ow = _oracle_world(_orc(dtype), scene)
    ow.run(H, 150)
    w = _gpu_world(scene, dtype, mask)
    w.step(H, 100); w.step(H, 50)
    w.synchronize()
    _same_bits(w.state(), ow.state())
    w.close()


# 4. -0.0 in components the tick "does not change": v + 0 turns it into +0.0, and that has to reach the slab
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("per_call", [1, 40])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_negative_zero_is_a_change(dtype, per_call, mask):
    scene = _headline_scene(dtype, spin=False, nx=63, nz=33)        # 2079 bodies; column 31 sits at x = 0
    centre = np.where(scene.pos[:, 0] == 0.0)[0]
    assert len(centre) == 33
    scene.pos[centre[::2], 0] = -0.0
    neg_v = np.r_[np.arange(64 * 4, 64 * 5), [3, 64 * 10 + 17, 2078]]
    scene.lvel[neg_v, 0] = -0.0
    neg_w = np.r_[np.arange(64 * 8, 64 * 9), [64 * 2 + 1, 2000]]
    scene.avel[neg_w] = -0.0
    assert np.signbit(scene.lvel[neg_v, 0]).all() and np.signbit(scene.pos[centre[::2], 0]).all()
    ow = _oracle_world(_orc(dtype), scene)
    ow.run(H, 40)
    ref = ow.state()
    assert not np.signbit(ref[2][neg_v, 0]).any(), "the oracle's tick turns lvel.x = -0.0 into +0.0"
    assert not np.signbit(ref[0][centre[::2], 0]).any(), "... and pos.x = -0.0 with it"
    w = _gpu_world(scene, dtype, mask)
    for _ in range(40 // per_call):
        w.step(H, per_call)
    w.synchronize()
    got = w.state()
    _same_bits(got, ref)
    assert not np.signbit(got[2][neg_v, 0]).any() and not np.signbit(got[0][centre[::2], 0]).any()
    w.close()


# 5. constants uniform -> mixed -> uniform in mid-run; the uniform inertia is not isotropic (live gyroscopic term)
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_mass_uploads_in_mid_run(dtype, mask):
    scene = _headline_scene(dtype, spin=True)
    scene.inertia[:] = (0.5, 1.0, 1.5)
    scene.avel *= 3.0
    force = np.zeros((scene.n, 3), dtype)
    force[::3, 0] = 0.7; force[::5, 1] = -2.0                   # mass enters through (h / m) f
    orc = _orc(dtype)
    ow = _oracle_world(orc, scene)
    w = _gpu_world(scene, dtype, mask)

    def set_mass(first, count, m):
        w.upload(pkg.batch.MASS, np.full((count, 1), m, dtype), first=first)
        I9 = np.diag(np.array([0.5, 1.0, 1.5], dtype)).astype(dtype).ravel()
        _, ip = orc.arr(I9)
        for b in range(first, first + count):
            orc.lib.orc_body_set_mass(ow.w, b, m, ip)

    def push():
        w.upload(pkg.batch.FORCE, force)
        for b in np.where(force.any(axis=1))[0]:
            orc.lib.orc_body_add_force(ow.w, int(b), float(force[b, 0]), float(force[b, 1]), float(force[b, 2]))

    def run(k):
        w.step(H, k); ow.run(H, k)
        w.synchronize()
        _same_bits(w.state(), ow.state(), what=f"after {k} more ticks: ")

    push(); run(20)                          # uniform m = 1
    set_mass(100, 200, 2.0)                  # a sub-range: mixed
    push(); run(20)
    set_mass(100, 200, 2.0)                  # the same again: still mixed
    run(5)
    set_mass(0, scene.n, 3.0)                # the full range: uniform again, at 3
    push(); run(20)
    set_mass(scene.n - 1, 1, 3.0)            # a sub-range of the value in place: stays uniform
    push(); run(20)
    w.close()


# 6. eight ticks per launch, external force on some bodies, no collision proof (every launch in place)
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("box_mass", [False, True])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_many_ticks_per_launch_with_external_force(dtype, box_mass, mask):
    scene = pkg.scenes.box_grid(64, 32, seed=11, spin=True, box_mass=box_mass, plane=False).astype(dtype)
    force = np.zeros((scene.n, 3), dtype)
    force[64 * 2:64 * 3, 0] = 1.5
    force[[7, 64 * 9 + 5, 2047], 2] = -0.25
    torque = np.zeros((scene.n, 3), dtype)
    torque[64 * 5 + 3] = (0.1, 0.0, -0.2)
    orc = _orc(dtype)
    ow = _oracle_world(orc, scene)
    for b in np.where(force.any(axis=1))[0]:
        orc.lib.orc_body_add_force(ow.w, int(b), *[float(x) for x in force[b]])
    for b in np.where(torque.any(axis=1))[0]:
        orc.lib.orc_body_add_torque(ow.w, int(b), *[float(x) for x in torque[b]])
    ow.run(H, 45)
    w = _gpu_world(scene, dtype, mask, setup=lambda w: (w.set_ticks_per_launch(8), w.set_body_collisions(False)))
    w.upload(pkg.batch.FORCE, force); w.upload(pkg.batch.TORQUE, torque)
    w.step(H, 45)
    w.synchronize()
    _same_bits(w.state(), ow.state())
    assert np.array_equal(w.download(pkg.batch.FORCE), np.zeros_like(force))      # cleared by the tick they acted in
    w.close()


# 7. a mid-air collision rolls a chunk back; the first launch after the rollback is out of place again
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("mode", ["pingpong", "copy"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_rollback_and_replay(dtype, mode, mask):
    scene = pkg.scenes.box_grid(16, 16, seed=13, y_range=(10.0, 12.0), spin=True, box_mass=False, plane=False).astype(dtype)
    rng = np.random.default_rng(5)
    movers = rng.random(scene.n) < 0.4                          # the others keep lvel.x / lvel.z = 0: their stores are elided
    scene.lvel[movers, 0] = rng.uniform(-3.0, 3.0, int(movers.sum()))
    scene.lvel[movers, 2] = rng.uniform(-3.0, 3.0, int(movers.sum()))
    ow = _oracle_world(_orc(dtype), scene)
    ow.run(H, 150)
    w = _gpu_world(scene, dtype, mask,
                   setup=lambda w: w.set_snapshot_mode(pkg.batch.SNAPSHOT_COPY if mode == "copy" else pkg.batch.SNAPSHOT_PINGPONG))
    for k in (7, 50, 1, 92):
        w.step(H, k)
    w.synchronize()
    _same_bits(w.state(), ow.state())
    assert w.collision_stats()["pair_ticks"] > 0, "the scene is meant to collide in mid-air"
    w.close()


# 8. body counts that are no multiple of the 64-body tile or the 256-body block
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("n", [1, 63, 65, 257, 1000])
def test_ragged_body_counts(n, mask):
    full = _headline_scene("float32", spin=True, nx=40, nz=25)
    scene = full.slice(0, n).astype("float32")
    scene.lvel[n // 2, 0] = 0.01
    ow = _oracle_world(_orc("float32"), scene)
    ow.run(H, 70)
    w = _gpu_world(scene, "float32", mask)
    w.step(H, 33); w.step(H, 37)
    w.synchronize()
    _same_bits(w.state(), ow.state())
    w.close()


# 9. a caller that writes constants through a device pointer: ANY dmxBatchDevicePtr is an address into the slab, whose documented
#    layout reaches components 13..16 -- from then on the constants are loaded, whatever field the pointer was asked for
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("via", ["inertia", "pos"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_constants_written_through_a_device_pointer(dtype, via, mask):
    import ctypes as C
    hip = C.CDLL(None)                       # the HIP runtime is already in the process
    scene = _headline_scene(dtype, spin=True)
    scene.avel *= 3.0
    orc = _orc(dtype)
    ow = _oracle_world(orc, scene)
    w = _gpu_world(scene, dtype, mask, setup=lambda w: w.set_body_collisions(False))      # the state stays in one slab
    w.step(H, 10); ow.run(H, 10)
    w.synchronize()
    item = np.dtype(dtype).itemsize
    if via == "inertia":
        addr = w.device_ptr(pkg.batch.INERTIA, 0)                       # inertia.x of the first tile's 64 bodies: one run
    else:
        addr = w.device_ptr(pkg.batch.POS, 0) + 14 * 64 * item          # the same run, from pos.x by the documented layout
    new = np.full(64, 3.0, dtype)
    assert hip.hipMemcpy(C.c_void_p(addr), C.c_void_p(new.ctypes.data), C.c_size_t(new.nbytes), 1) == 0      # host to device
    _, ip = orc.arr(np.diag(np.array([3.0, 1.0, 1.0], dtype)).ravel())
    for b in range(64):
        orc.lib.orc_body_set_mass(ow.w, b, 1.0, ip)
    w.step(H, 40); ow.run(H, 40)
    w.synchronize()
    _same_bits(w.state(), ow.state())
    w.close()


# 10. ticks replayed from a captured HIP graph see a later upload of the constants like eager ticks do (a launch recorded into
#     a graph does not take them as arguments: their values would be those of capture time for good)
@pytest.mark.parametrize("mask", MASKS)
def test_graph_replays_see_uploaded_constants(mask):
    import torch
    dtype = "float32"
    scene = _headline_scene(dtype, spin=True)
    scene.inertia[:] = (0.5, 1.0, 1.5)
    scene.avel *= 3.0
    orc = _orc(dtype)
    ow = _oracle_world(orc, scene)
    w = _gpu_world(scene, dtype, mask, setup=lambda w: w.set_body_collisions(False))
    stream = torch.cuda.Stream()
    w.set_stream(stream.cuda_stream)
    w.step(H, 2); ow.run(H, 2)                       # eager: the kernels are loaded before the capture
    w.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        w.step(H, 4)                                 # recorded, not run
    for _ in range(3):
        g.replay()
    ow.run(H, 12)
    torch.cuda.synchronize()
    _same_bits(w.state(), ow.state(), what="before the upload: ")
    w.upload(pkg.batch.INERTIA, np.tile(np.array([1.5, 1.0, 0.5], dtype), (scene.n, 1)))      # uniform before, uniform after
    _, ip = orc.arr(np.diag(np.array([1.5, 1.0, 0.5], dtype)).ravel())
    for b in range(scene.n):
        orc.lib.orc_body_set_mass(ow.w, b, 1.0, ip)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    w.step(H, 3); ow.run(H, 15)
    w.synchronize()
    _same_bits(w.state(), ow.state(), what="after the upload: ")
    del g
    w.close()


def test_mask_is_validated():
    w = pkg.BatchWorld(4, dtype="float32")
    for bad in (-1, 4, 8):
        with pytest.raises(Exception):
            w.set_elision(bad)
    for ok in (0, 1, 2, 3):
        w.set_elision(ok)
    w.close()
