"""integrate_free leaves out the loads of pos.x/z and lvel.x/z in tiles that have proven them fixed (dmxBatchSetLoadElision,
csrc/dmx_fixed.hpp).  That must not change a single bit, whatever happens to the batch in mid-run: every case is compared with
the CPU oracle by value (array_equal) AND on the bit patterns, with the feature on (the default) and again switched off, and
the launch counts say that the feature was at work where it should be and at rest where it must be."""
import ctypes as C

import numpy as np
import pytest

from __graft_entry__ import load_package

pkg = load_package()
pytestmark = pytest.mark.gpu

H = 1.0 / 60.0
DTYPES = ["float32", "float64"]
ON_OFF = [True, False]


def _orc(dtype):
    from oracle.orc_ctypes import Oracle
    return Oracle(dtype)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(got, ref, what="", rows=slice(None)):
    for name, a, b in zip(("pos", "quat", "lvel", "avel"), got, ref):
        a, b = a[rows], b[rows]
        assert a.dtype == b.dtype
        assert np.array_equal(a, b), f"{what}{name}: values differ, max abs diff {np.max(np.abs(a - b))}"
        diff = _bits(a) != _bits(b)
        assert not diff.any(), f"{what}{name}: {int(diff.sum())} components differ in their bits (first at {np.argwhere(diff)[0]})"


def _headline_scene(dtype, spin=True, nx=64, nz=32):
    # the reference's AddBody: m = 1, I = identity; dropped at rest.  2 048 bodies = 32 tiles
    return pkg.scenes.box_grid(nx, nz, seed=7, spin=spin, box_mass=False, plane=False).astype(dtype)


class Pair:
    """a batch on the GPU and the oracle's world of the same scene, advanced together"""

    def __init__(self, scene, dtype, on, setup=None, gravity=(0.0, -9.8, 0.0)):
        self.dtype, self.on = dtype, on
        self.orc = _orc(dtype)
        self.ow = self.orc.world(gravity=gravity)
        self.ow.add_boxes(scene.pos, scene.quat, scene.lvel, scene.avel, scene.mass[:, 0], scene.inertia, scene.sides)
        self.w = pkg.BatchWorld(scene.n, dtype=dtype, gravity=gravity)
        if not on:
            self.w.set_load_elision(False)
        if setup:
            setup(self.w)
        self.w.load_scene(scene)

    def run(self, k, per_call=1, h=H):
        done = 0
        while done < k:
            j = min(per_call, k - done)
            self.w.step(h, j)
            done += j
        self.ow.run(h, k)

    def check(self, what="", rows=slice(None)):
        self.w.synchronize()
        _same_bits(self.w.state(), self.ow.state(), what=what, rows=rows)

    def stats(self):
        return self.w.load_elision_stats()

    def finish(self, min_lean=20):
        """the end of a door case: same bits, and the feature was at work on both sides of the door (or not at all)"""
        self.check()
        s = self.stats()
        if self.on:
            assert s["lean"] >= min_lean and s["establish"] >= 2 and s["ended"] == 0, s
        else:
            assert all(v == 0 for v in s.values()), s
        self.w.close()

    def set_lvel(self, bodies, lvel):
        for b, v in zip(bodies, lvel):
            self.w.upload(pkg.batch.LVEL, v[None, :], first=int(b))
            self.orc.lib.orc_body_set_linear_vel(self.ow.w, int(b), float(v[0]), float(v[1]), float(v[2]))


def _tiles_fixed_on_x(w, n):
    """which tiles' words say x fixed: the stats count the tiles of the active range, so prefix counts over a shrinking active
    range give every tile's bit (no launch happens in between: the words stay as the last launch left them)"""
    ntiles = (n + 63) // 64
    prefix = [0]
    for t in range(1, ntiles + 1):
        w.set_active_count(min(64 * t, n))
        prefix.append(w.load_elision_stats()["tiles_x_fixed"])
    w.set_active_count(n)
    return [prefix[t + 1] - prefix[t] == 1 for t in range(ntiles)]


# ---- the feature is not inert --------------------------------------------------------------------------------------
@pytest.mark.parametrize("on", ON_OFF)
@pytest.mark.parametrize("per_call", [1, 7, 150])
@pytest.mark.parametrize("dtype", DTYPES)
def test_headline_shape_runs_lean(dtype, per_call, on):
    scene = _headline_scene(dtype)
    p = Pair(scene, dtype, on)
    p.run(150, per_call=per_call)
    p.check()
    s = p.stats()
    if on:
        assert s["lean"] > 0 and s["establish"] > 0 and s["ended"] == 0, s
        if per_call == 1:
            assert s["lean"] >= 100, s
        assert s["tiles_x_fixed"] == 32 and s["tiles_z_fixed"] == 32, s
    else:
        assert all(v == 0 for v in s.values()), s
    p.w.close()


@pytest.mark.parametrize("on", ON_OFF)
@pytest.mark.parametrize("dtype", DTYPES)
def test_lateral_velocity_on_some_tiles_and_lanes(dtype, on):
    scene = _headline_scene(dtype)
    moving = {1, 6, 31, 0, 3, 12, 17}
    for tile in (1, 6, 31):
        scene.lvel[64 * tile:64 * tile + 64, 0] = 0.05
    for body in (5, 64 * 3 + 63, 64 * 12, 64 * 17 + 31):       # one lane of its wavefront
        scene.lvel[body, 0] = 0.04
    p = Pair(scene, dtype, on)
    p.run(100, per_call=100)
    p.run(50, per_call=1)
    p.check()
    s = p.stats()
    if on:
        assert s["lean"] >= 100 and s["tiles_x_fixed"] == 32 - len(moving) and s["tiles_z_fixed"] == 32, s
        fixed = _tiles_fixed_on_x(p.w, scene.n)
        assert [t for t in range(32) if not fixed[t]] == sorted(moving)
    else:
        assert all(v == 0 for v in s.values()), s
    p.w.close()


# ---- one case per door, in mid-run: at least 10 lean ticks before it, at least 10 more ticks behind it --------------------
@pytest.mark.parametrize("on", ON_OFF)
@pytest.mark.parametrize("dtype", DTYPES)
def test_door_lvel_uploaded_on_a_sub_range(dtype, on):
    scene = _headline_scene(dtype)
    p = Pair(scene, dtype, on)
    p.run(14)
    lv = p.w.download(pkg.batch.LVEL)
    bodies = np.arange(100, 200)                   # cuts through tiles 1 and 3, covers tile 2
    lv[bodies, 0] = 0.05
    p.set_lvel(bodies, lv[bodies])
    p.run(14)
    p.finish()


@pytest.mark.parametrize("on", ON_OFF)
@pytest.mark.parametrize("dtype", DTYPES)
def test_door_negative_zero_uploaded_into_pos_x(dtype, on):
    scene = _headline_scene(dtype, spin=False)
    p = Pair(scene, dtype, on)
    p.run(14)
    pos = p.w.download(pkg.batch.POS)
    bodies = [5, 64 * 3 + 9, 64 * 10 + 17, 2047]   # one per row of the grid: they do not meet at x = 0
    for b in bodies:
        pos[b, 0] = -0.0
        p.w.upload(pkg.batch.POS, pos[b][None, :], first=b)
        p.orc.lib.orc_body_set_position(p.ow.w, b, float(pos[b, 0]), float(pos[b, 1]), float(pos[b, 2]))
    p.run(14)
    got = p.w.download(pkg.batch.POS)
    assert not np.signbit(got[bodies, 0]).any(), "x + h * 0 turns pos.x = -0.0 into +0.0, and that has to reach the slab"
    p.finish()


@pytest.mark.parametrize("on", ON_OFF)
@pytest.mark.parametrize("dtype", DTYPES)
def test_door_gravity_changed_and_back(dtype, on):
    scene = _headline_scene(dtype)
    p = Pair(scene, dtype, on)
    p.run(14)
    p.w.set_gravity(0.3, -9.81, 0.0); p.orc.lib.orc_world_set_gravity(p.ow.w, 0.3, -9.81, 0.0)
    p.run(6)
    p.w.set_gravity(0.0, -9.8, 0.0); p.orc.lib.orc_world_set_gravity(p.ow.w, 0.0, -9.8, 0.0)
    p.run(14)
    p.finish()


@pytest.mark.parametrize("on", ON_OFF)
@pytest.mark.parametrize("dtype", DTYPES)
def test_door_h_changed_between_calls(dtype, on):
    scene = _headline_scene(dtype, spin=False)
    ring = np.where((np.abs(scene.pos[:, 0]) >= 16.0) & (np.abs(scene.pos[:, 0]) < 32.0))[0]
    assert len(ring) > 100
    scene.lvel[ring, 0] = 3e-5          # h v is below half an ulp of x in [16, 32) at h = 1/60 in f32, above one at h = 1/10
    p = Pair(scene, dtype, on)
    x0 = scene.pos[ring, 0].copy()
    p.run(14)
    if dtype == "float32":
        assert np.array_equal(_bits(p.ow.state()[0][ring, 0]), _bits(x0)), "pos.x is a fixed point of f32 at h = 1/60"
    p.run(10, h=0.1)
    if dtype == "float32":
        assert (p.ow.state()[0][ring, 0] != x0).all(), "... and moves at h = 1/10"
    p.check(what="after the ticks at h = 1/10: ")
    p.run(14)
    p.finish()


@pytest.mark.parametrize("on", ON_OFF)
@pytest.mark.parametrize("dtype", DTYPES)
def test_door_force_on_x(dtype, on):
    scene = _headline_scene(dtype)
    force = np.zeros((scene.n, 3), dtype)
    force[64 * 2:64 * 3, 0] = 1.5
    force[[7, 64 * 9 + 5, 2047], 0] = -0.25
    p = Pair(scene, dtype, on)
    p.run(14)
    p.w.upload(pkg.batch.FORCE, force)
    for b in np.where(force.any(axis=1))[0]:
        p.orc.lib.orc_body_add_force(p.ow.w, int(b), *[float(x) for x in force[b]])
    p.run(14)
    p.finish()


@pytest.mark.parametrize("on", ON_OFF)
@pytest.mark.parametrize("dtype", DTYPES)
def test_door_many_ticks_per_launch_for_one_call(dtype, on):
    scene = _headline_scene(dtype)
    scene.lvel[64 * 4 + 3, 0] = 0.02
    p = Pair(scene, dtype, on)
    p.run(14)
    p.w.set_ticks_per_launch(8)
    p.run(16, per_call=16)
    p.w.set_ticks_per_launch(1)
    p.run(14)
    p.finish()


@pytest.mark.parametrize("on", ON_OFF)
@pytest.mark.parametrize("dtype", DTYPES)
def test_door_ground_plane_on_and_off(dtype, on):
    scene = _headline_scene(dtype)
    p = Pair(scene, dtype, on)
    p.run(14)
    p.w.set_plane(0.0, 1.0, 0.0, -1000.0, True)         # far below: the kernels of ticks with contacts step the bodies, nobody lands
    g = p.ow.add_plane(0.0, 1.0, 0.0, -1000.0)
    p.run(5)
    p.w.set_plane(0.0, 1.0, 0.0, -1000.0, False)
    p.orc.lib.orc_geom_set_category_bits(p.ow.w, g, 0); p.orc.lib.orc_geom_set_collide_bits(p.ow.w, g, 0)
    p.run(14)
    p.finish()


@pytest.mark.parametrize("on", ON_OFF)
@pytest.mark.parametrize("dtype", DTYPES)
def test_door_active_count_lowered_and_raised(dtype, on):
    # lowered by 72, not 70: an active count below n must be a multiple of 4 (dmxBatchSetActiveCount); 1 976 cuts tile 30
    scene = _headline_scene(dtype)
    scene.lvel[1970:1990, 0] = 0.03
    p = Pair(scene, dtype, on)
    tail = _orc(dtype).world()          # the 72 bodies that sit out 12 ticks: the oracle's world without those ticks
    tail.add_boxes(scene.pos, scene.quat, scene.lvel, scene.avel, scene.mass[:, 0], scene.inertia, scene.sides)
    p.run(14); tail.run(H, 14)
    p.w.set_active_count(scene.n - 72)
    p.run(12)
    p.w.set_active_count(scene.n)
    p.run(14); tail.run(H, 14)
    p.check(rows=slice(0, scene.n - 72))
    _same_bits(p.w.state(), tail.state(), what="bodies that sat out: ", rows=slice(scene.n - 72, scene.n))
    s = p.stats()
    assert (s["lean"] >= 30 and s["ended"] == 0) if on else all(v == 0 for v in s.values()), s
    p.w.close()


@pytest.mark.parametrize("on", ON_OFF)
@pytest.mark.parametrize("dtype", DTYPES)
def test_door_checkpoint_restored(dtype, on):
    scene = _headline_scene(dtype)
    scene.lvel[64 * 7:64 * 8, 2] = -0.03
    p = Pair(scene, dtype, on)
    p.run(14)
    ck = p.w.checkpoint()
    p.w.step(H, 20)                     # ticks the restore throws away: the oracle does not take them
    p.w.restore(ck)
    p.run(14)
    p.finish()


@pytest.mark.parametrize("on", ON_OFF)
@pytest.mark.parametrize("mode", ["pingpong", "copy"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_door_rollback_and_replay(dtype, mode, on):
    # the scene of test_gpu_elision.py::test_rollback_and_replay: a mid-air collision rolls a chunk back
    scene = pkg.scenes.box_grid(16, 16, seed=13, y_range=(10.0, 12.0), spin=True, box_mass=False, plane=False).astype(dtype)
    rng = np.random.default_rng(5)
    movers = rng.random(scene.n) < 0.4
    scene.lvel[movers, 0] = rng.uniform(-3.0, 3.0, int(movers.sum()))
    scene.lvel[movers, 2] = rng.uniform(-3.0, 3.0, int(movers.sum()))
    p = Pair(scene, dtype, on,
             setup=lambda w: w.set_snapshot_mode(pkg.batch.SNAPSHOT_COPY if mode == "copy" else pkg.batch.SNAPSHOT_PINGPONG))
    p.ow.run(H, 150)
    for k in (7, 50, 1, 92):
        p.w.step(H, k)
    s = p.stats()           # first: the counts are those of the run, taken before this call settles the batch (a door itself)
    p.check()
    cs = p.w.collision_stats()
    assert cs["pair_ticks"] > 0 and cs["careful_ticks"] > 0, "the scene is meant to collide in mid-air: a chunk rolled back and replayed exactly"
    # breaks > 0: nothing but dmxBatchStep was called, so what broke the chain is the rollback and the exact ticks behind it
    assert (s["lean"] > 0 and s["breaks"] > 0) if on else all(v == 0 for v in s.values()), s
    p.w.close()


@pytest.mark.parametrize("on", ON_OFF)
@pytest.mark.parametrize("dtype", DTYPES)
def test_door_state_read_between_calls(dtype, on):
    scene = _headline_scene(dtype)
    p = Pair(scene, dtype, on)
    p.run(14)
    p.check(what="in mid-run: ")
    p.run(14)
    p.finish()


# ---- ended for good ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on", ON_OFF)
@pytest.mark.parametrize("dtype", DTYPES)
def test_device_pointer_ends_it(dtype, on):
    hip = C.CDLL(None)                       # the HIP runtime is already in the process
    scene = _headline_scene(dtype)
    p = Pair(scene, dtype, on, setup=lambda w: w.set_body_collisions(False))       # the state stays in one slab
    p.run(14)
    p.w.synchronize()
    before = p.stats()
    addr = p.w.device_ptr(pkg.batch.LVEL, 0)                 # lvel.x of the first tile's 64 bodies: one run
    new = np.full(64, 0.05, dtype)
    assert hip.hipMemcpy(C.c_void_p(addr), C.c_void_p(new.ctypes.data), C.c_size_t(new.nbytes), 1) == 0      # host to device
    lv = p.ow.state()[2]
    for b in range(64):
        p.orc.lib.orc_body_set_linear_vel(p.ow.w, b, 0.05, float(lv[b, 1]), float(lv[b, 2]))
    p.run(14)
    p.check()
    after = p.stats()
    assert after["lean"] == before["lean"] and after["establish"] == before["establish"], (before, after)
    assert after["ended"] == 1
    assert before["lean"] >= 10 if on else before["lean"] == 0
    p.w.close()


@pytest.mark.parametrize("on", ON_OFF)
@pytest.mark.parametrize("dtype", DTYPES)
def test_capture_ends_it(dtype, on):
    import torch
    scene = _headline_scene(dtype)
    p = Pair(scene, dtype, on, setup=lambda w: w.set_body_collisions(False))
    stream = torch.cuda.Stream()
    p.w.set_stream(stream.cuda_stream)
    p.run(14)                                        # eager: the kernels are loaded before the capture
    p.w.synchronize()
    before = p.stats()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        p.w.step(H, 4)                               # recorded, not run
    for _ in range(3):
        g.replay()
    p.ow.run(H, 12)
    torch.cuda.synchronize()
    p.check(what="after the replays: ")
    lv = p.w.download(pkg.batch.LVEL)
    lv[:64, 0] = 0.05
    p.set_lvel(np.arange(64), lv[:64])
    g.replay(); p.ow.run(H, 4)
    torch.cuda.synchronize()
    p.run(10)
    p.check(what="after eager ticks behind the replays: ")
    after = p.stats()
    assert after["lean"] == before["lean"] and after["establish"] == before["establish"], (before, after)
    assert after["ended"] == 1          # (asked whether or not the switch is on: a graph recorded while it is off is replayed all the same)
    assert before["lean"] >= 10 if on else before["lean"] == 0
    del g
    p.w.close()


# ---- body counts that are no multiple of the 64-body tile or the 256-body block ----------------------------------------
@pytest.mark.parametrize("on", ON_OFF)
@pytest.mark.parametrize("n", [1, 63, 65, 257, 1000])
def test_ragged_body_counts(n, on):
    full = _headline_scene("float32", nx=40, nz=25)
    scene = full.slice(0, n).astype("float32")
    scene.lvel[n // 2, 0] = 0.01
    p = Pair(scene, "float32", on)
    p.run(33, per_call=33)
    p.run(37, per_call=1)
    p.check()
    s = p.stats()
    if on:
        ntiles = (n + 63) // 64
        assert s["lean"] >= 30 and s["tiles_x_fixed"] == ntiles - 1 and s["tiles_z_fixed"] == ntiles, s
    else:
        assert all(v == 0 for v in s.values()), s
    p.w.close()


# ---- gravity along z: x and y become fixed, z does not -----------------------------------------------------------------
@pytest.mark.parametrize("on", ON_OFF)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gravity_along_z(dtype, on):
    scene = _headline_scene(dtype)
    p = Pair(scene, dtype, on, setup=lambda w: w.set_body_collisions(False), gravity=(0.0, 0.0, -9.81))
    p.run(30)
    p.check()
    s = p.stats()
    if on:
        assert s["lean"] >= 25 and s["tiles_x_fixed"] == 32 and s["tiles_z_fixed"] == 0, s
    else:
        assert all(v == 0 for v in s.values()), s
    p.w.close()


def test_switch_is_validated():
    w = pkg.BatchWorld(4, dtype="float32")
    for bad in (-1, 2):
        with pytest.raises(Exception):
            pkg.batch._check(w.lib.dmxBatchSetLoadElision(w.h, bad), "dmxBatchSetLoadElision")
    for bad in (4, 8):                              # the new removal is no bit of the public mask
        with pytest.raises(Exception):
            w.set_elision(bad)
    w.set_load_elision(False); w.set_load_elision(True)
    w.close()
