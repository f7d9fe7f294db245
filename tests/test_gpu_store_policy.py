"""integrate_free's state stores carry a cache-policy bit (csrc/dmx_internal.hpp: store_state).  A store of another flavour cannot
change a value; what it could change is what the next reader of the slab sees.  So these tests read the state right behind a launch
by every route the library has, and compare with the CPU oracle by value (array_equal) and on the bit patterns: tolerance zero.
Scenes as tests/test_gpu_launch_consts.py builds them: box_grid with spin, no plane, unit mass; 200 bodies (three full tiles and one
of 8 lanes) and 321 (five tiles and one lane), f32 and f64.
  1. one tick per call, 24 calls, the state downloaded after every tick (the reference's loop reading poses after any tick);
     dmxBatchLoadElisionStats must show establishing and lean launches, dmxBatchTorqueFreeStats the short tick.  Run with the
     body-body proof off (set_body_collisions(False)), the one configuration in which a launch behind a download can be lean:
     the state stays in one slab and every launch runs in place.  dmxBatchDownload closes the open chunk but leaves the
     fixed-axis chain standing (csrc/dmx_fixed.hpp), so the first launch establishes and the 23 behind downloads are lean.
  1a. the same loop with the proof on, as a batch comes: every call is a collision-proof chunk of one tick, whose only launch
     fills the other slab and tests the safe zones, so it loads every pos.x / pos.z and is an establishing launch by necessity
     (24 of them, no lean one); values and the short tick as in 1
  1b. three ticks per call, 8 calls (an establishing launch, then lean ones), the state and the transforms read after every call
  2. case 1 with the transform read-out (pack_transforms) after every tick, against orc_pack_transform of the oracle's bodies
  3. a host upload behind lean launches: 12 ticks in one call (the last eleven launches lean), then one body's lvel and another's
     quat uploaded, the oracle given the same change, then one tick per call with a download after each -- a line kept in a cache
     across the launch boundary would show as stale here.  (The launch behind an upload is an establishing one and has to be: the
     upload may have moved a body whose axis the tile's word calls fixed.)
  4. four ticks per launch over 24 ticks: the many-ticks kernel's single write per launch, read after every launch
  5. forces and torques applied before a tick (the instantiation with accumulators): its state stores, the cleared accumulators,
     and a second tick behind it"""
import ctypes as C
import functools

import numpy as np
import pytest

from __graft_entry__ import load_package

pkg = load_package()
pytestmark = pytest.mark.gpu

H = 1.0 / 60.0
TICKS = 24
GRIDS = {200: (20, 10), 321: (107, 3)}
DTYPES = ["float32", "float64"]
NAMES = ("pos", "quat", "lvel", "avel")


def _scene(n, dtype):
    s = pkg.scenes.box_grid(*GRIDS[n], seed=23, spin=True, box_mass=False, plane=False).astype(dtype)
    assert s.n == n
    return s


def _orc(dtype):
    from oracle.orc_ctypes import Oracle
    return Oracle(dtype)


def _oracle_world(orc, s):
    ow = orc.world()
    ow.add_boxes(s.pos, s.quat, s.lvel, s.avel, s.mass[:, 0], s.inertia, s.sides)
    return ow


def _oracle_transforms(orc, ow, n):
    out = np.zeros((n, 16), orc.dtype)
    RP = C.POINTER(orc.real)
    for i in range(n):
        orc.lib.orc_pack_transform(out[i].ctypes.data_as(RP), orc.lib.orc_body_get_position(ow.w, i), orc.lib.orc_body_get_rotation(ow.w, i))
    return out


@functools.lru_cache(maxsize=None)
def _oracle_ticks(n, dtype):
    """-> per tick 1..TICKS: (state, transforms), computed once and shared read-only"""
    orc = _orc(dtype)
    ow = _oracle_world(orc, _scene(n, dtype))
    out = []
    for _ in range(TICKS):
        ow.tick(orc.dtype.type(H))
        assert ow.n_contacts() == 0
        st, tr = ow.state(), _oracle_transforms(orc, ow, n)
        for a in st + (tr,):
            a.setflags(write=False)
        out.append((st, tr))
    ow.close()
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(got, ref, what):
    for name, a, b in zip(NAMES, got, ref):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert not np.isnan(b).any(), f"{what}: the oracle's {name} holds a NaN"
        assert np.array_equal(a, b), f"{what}: {name}: values differ, max abs diff {np.max(np.abs(a - b))}"
        diff = _bits(a) != _bits(b)
        assert not diff.any(), f"{what}: {name}: {int(diff.sum())} components differ in their bits (first at {np.argwhere(diff)[0]})"


def _world(n, dtype, setup=None):
    w = pkg.BatchWorld(n, dtype=dtype)
    if setup is not None:
        setup(w)
    w.load_scene(_scene(n, dtype))
    return w


def _one_tick_per_call(dtype, n, setup):
    ref = _oracle_ticks(n, dtype)
    w = _world(n, dtype, setup=setup)
    try:
        for t in range(TICKS):
            w.step(H, 1)
            _same_bits(w.state(), ref[t][0], f"{dtype} n={n} tick {t + 1}")
        tf, fix = w.torque_free_stats(), w.load_elision_stats()
    finally:
        w.close()
    print(dtype, n, tf, fix)
    return tf, fix


@pytest.mark.parametrize("n", sorted(GRIDS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_state_downloaded_after_every_tick(dtype, n):
    tf, fix = _one_tick_per_call(dtype, n, lambda w: w.set_body_collisions(False))
    assert fix["establish"] > 0 and fix["lean"] > 0, fix
    assert tf["short"] > 0 and tf["general"] == 0, tf
    assert fix["establish"] == 1 and fix["lean"] == TICKS - 1, fix      # every download was followed by a lean launch


@pytest.mark.parametrize("n", sorted(GRIDS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_state_downloaded_after_every_tick_with_the_proof_on(dtype, n):
    tf, fix = _one_tick_per_call(dtype, n, None)
    assert fix["establish"] == TICKS and fix["lean"] == 0, fix          # a chunk's first launch each: it cannot be lean
    assert tf["short"] == TICKS and tf["general"] == 0, tf


@pytest.mark.parametrize("n", sorted(GRIDS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_transforms_read_after_every_tick(dtype, n):
    ref = _oracle_ticks(n, dtype)
    w = _world(n, dtype)
    try:
        for t in range(TICKS):
            w.step(H, 1)
            T = w.transforms()
            assert np.array_equal(T, ref[t][1]), f"{dtype} n={n} tick {t + 1}: transforms differ in {int((T != ref[t][1]).any(axis=1).sum())} bodies"
            assert not (_bits(T) != _bits(ref[t][1])).any(), f"{dtype} n={n} tick {t + 1}: transforms differ in their bits"
    finally:
        w.close()


@pytest.mark.parametrize("n", sorted(GRIDS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_state_and_transforms_read_behind_lean_launches(dtype, n):
    ref = _oracle_ticks(n, dtype)
    w = _world(n, dtype)
    try:
        for t in range(3, TICKS + 1, 3):
            w.step(H, 3)
            T = w.transforms()
            _same_bits(w.state(), ref[t - 1][0], f"{dtype} n={n} tick {t}")
            assert np.array_equal(T, ref[t - 1][1]) and not (_bits(T) != _bits(ref[t - 1][1])).any(), f"{dtype} n={n} tick {t}: transforms"
        fix = w.load_elision_stats()
    finally:
        w.close()
    print(dtype, n, fix)
    assert fix["establish"] > 0 and fix["lean"] >= TICKS // 3, fix       # at least one lean launch in every call


@pytest.mark.parametrize("n", sorted(GRIDS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_host_upload_behind_lean_launches(dtype, n):
    orc = _orc(dtype)
    s = _scene(n, dtype)
    ow = _oracle_world(orc, s)
    w = _world(n, dtype)
    bl, bq = 70, n - 1                      # a body inside the second tile; the last body (the tile of 8 lanes / of one lane)
    lvel = np.array([[0.25, -1.5, 0.75]], dtype)
    quat = np.array([[0.0, 0.0, 1.0, 0.0]], dtype)      # unit length exactly: the oracle's normalisation on set leaves it as it is
    try:
        w.step(H, 12)
        ow.run(orc.dtype.type(H), 12)
        before = w.load_elision_stats()
        assert before["lean"] > 0, before       # lean launches ran before the upload
        w.upload(pkg.batch.LVEL, lvel, first=bl)
        w.upload(pkg.batch.QUAT, quat, first=bq)
        orc.lib.orc_body_set_linear_vel(ow.w, bl, *[float(x) for x in lvel[0]])
        orc.lib.orc_body_set_quaternion(ow.w, bq, orc.arr(quat[0])[1])
        _same_bits(w.state(), ow.state(), f"{dtype} n={n} behind the upload")
        for t in range(12, TICKS):
            w.step(H, 1)
            ow.tick(orc.dtype.type(H))
            _same_bits(w.state(), ow.state(), f"{dtype} n={n} tick {t + 1}")
        w.step(H, 3)                        # and lean launches again behind it
        ow.run(orc.dtype.type(H), 3)
        _same_bits(w.state(), ow.state(), f"{dtype} n={n} tick {TICKS + 3}")
        after = w.load_elision_stats()
    finally:
        w.close()
        ow.close()
    print(dtype, n, before, after)
    assert after["lean"] > before["lean"], (before, after)


@pytest.mark.parametrize("n", sorted(GRIDS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_four_ticks_per_launch(dtype, n):
    ref = _oracle_ticks(n, dtype)
    w = _world(n, dtype, setup=lambda w: (w.set_ticks_per_launch(4), w.set_body_collisions(False)))
    try:
        for t in range(4, TICKS + 1, 4):
            w.step(H, 4)
            _same_bits(w.state(), ref[t - 1][0], f"{dtype} n={n} tick {t}")
            assert np.array_equal(w.transforms(), ref[t - 1][1]), f"{dtype} n={n} tick {t}: transforms"
    finally:
        w.close()


@pytest.mark.parametrize("n", sorted(GRIDS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_forces_applied_before_a_tick(dtype, n):
    orc = _orc(dtype)
    s = _scene(n, dtype)
    ow = _oracle_world(orc, s)
    force = np.zeros((n, 3), dtype)
    force[64:128, 0] = 1.5
    force[[7, 130, n - 1], 2] = -0.25
    torque = np.zeros((n, 3), dtype)
    torque[[3, 64 + 5, n - 1]] = (0.1, 0.0, -0.2)
    w = _world(n, dtype)
    try:
        for rnd in range(2):                # accumulators, a tick with them, a tick without; then the same again behind lean-less launches
            w.upload(pkg.batch.FORCE, force); w.upload(pkg.batch.TORQUE, torque)
            for b in np.where(force.any(axis=1))[0]:
                orc.lib.orc_body_add_force(ow.w, int(b), *[float(x) for x in force[b]])
            for b in np.where(torque.any(axis=1))[0]:
                orc.lib.orc_body_add_torque(ow.w, int(b), *[float(x) for x in torque[b]])
            w.step(H, 1); ow.tick(orc.dtype.type(H))
            _same_bits(w.state(), ow.state(), f"{dtype} n={n} round {rnd}: the tick with accumulators")
            assert not w.download(pkg.batch.FORCE).any() and not w.download(pkg.batch.TORQUE).any(), "the accumulators were not cleared"
            w.step(H, 1); ow.tick(orc.dtype.type(H))
            _same_bits(w.state(), ow.state(), f"{dtype} n={n} round {rnd}: the tick behind it")
    finally:
        w.close()
        ow.close()
