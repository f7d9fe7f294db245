"""integrate_free's launches with uniform mass and inertia read 1 / Ib.k, 1 / h and the isotropy flag that the host computed once
(csrc/dmx_launch_consts.hpp) where the tick used to divide per lane: not a bit may change.  200 bodies (three full tiles and one of
8 lanes) and 321 (five tiles and one lane), f32 and f64, 24 ticks in one call -- the out-of-place first launch of a chunk, the
establishing launches and the lean ones of the fixed-axis words (dmxBatchLoadElisionStats must show both) -- compared with the CPU
oracle by value (array_equal) and on the bit patterns, as tests/test_gpu_elision.py compares.
  unit          m = 1, I = identity: the kernel with the short tick, which no longer computes anything ahead of its loads
  aniso_gyro0   m = 2.5, I = (0.3, 1.7, 0.9), no gyroscopic torque: the short tick
  aniso_gyro1   ... the explicit gyroscopic torque: the general tick fed the host's 1 / Ib.k
  aniso_gyro2   ... the implicit one: the host's 1 / h as well
  quat_scaled   unit constants, one body's quaternion scaled by 3: its wavefront takes the general tick inside the kernel with the
                short tick (the fallback reads the host's constants), the other tiles do not
  inertia_zero  a uniform inertia with a zero component: the rule says off, the launch loads the constants per lane and divides per
                lane.  1 / 0 = inf makes the rotated inverse inertia NaN (inf * 0) in oracle and device alike; there both must hold a
                NaN (its sign and payload are the processor's), everywhere else the bits must agree.  No other variant may hold a NaN.
Which kernels ran is read from dmxBatchTorqueFreeStats: launches with the short tick built in where its rule says on, the general
kernel elsewhere -- for inertia_zero in particular."""
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
VARIANTS = ["unit", "aniso_gyro0", "aniso_gyro1", "aniso_gyro2", "quat_scaled", "inertia_zero"]
SHORT = {"unit", "aniso_gyro0", "quat_scaled"}          # csrc/dmx_torque_free.hpp's rule says on
SCALED_BODY = 64 + 40


def _scene(variant, n, dtype):
    """-> (scene, gyro mode)"""
    s = pkg.scenes.box_grid(*GRIDS[n], seed=23, spin=True, box_mass=False, plane=False).astype(dtype)
    assert s.n == n
    gyro = 2
    if variant.startswith("aniso"):
        s.mass[:] = 2.5
        s.inertia[:] = np.array([0.3, 1.7, 0.9], dtype)
        gyro = int(variant[-1])
    elif variant == "quat_scaled":
        s.quat[SCALED_BODY] = 3.0 * np.array([0.8, 0.0, 0.6, 0.0])
    elif variant == "inertia_zero":
        s.inertia[:, 1] = 0.0
        gyro = 0
    return s, gyro


@functools.lru_cache(maxsize=None)
def _oracle(variant, n, dtype):
    from oracle.orc_ctypes import Oracle
    s, gyro = _scene(variant, n, dtype)
    orc = Oracle(dtype)
    ow = orc.world()
    orc.lib.orc_world_set_gyro_mode(ow.w, gyro)
    ow.add_boxes(s.pos, s.quat, s.lvel, s.avel, s.mass[:, 0], s.inertia, s.sides)
    ow.run(orc.dtype.type(H), TICKS)
    assert ow.n_contacts() == 0
    st = ow.state()
    ow.close()
    for a in st:
        a.setflags(write=False)
    return st


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(got, ref, what, nan_allowed):
    for name, a, b in zip(("pos", "quat", "lvel", "avel"), got, ref):
        assert a.dtype == b.dtype and a.shape == b.shape
        nan = np.isnan(b)
        assert nan_allowed or not nan.any(), f"{what}: the oracle's {name} holds a NaN"
        assert np.array_equal(np.isnan(a), nan), f"{what}: {name} is NaN where the oracle is not, or the other way round"
        assert np.array_equal(a[~nan], b[~nan]), f"{what}: {name}: values differ, max abs diff {np.max(np.abs(a[~nan] - b[~nan]))}"
        diff = (_bits(a) != _bits(b)) & ~nan
        assert not diff.any(), f"{what}: {name}: {int(diff.sum())} components differ in their bits (first at {np.argwhere(diff)[0]})"


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n", sorted(GRIDS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_launches_fed_host_constants_are_the_oracle(dtype, n, variant):
    ref = _oracle(variant, n, dtype)
    s, gyro = _scene(variant, n, dtype)
    w = pkg.BatchWorld(n, dtype=dtype)
    try:
        w.set_gyro_mode(gyro)
        w.load_scene(s)
        w.step(H, TICKS)
        w.synchronize()
        got, tf, fix = w.state(), w.torque_free_stats(), w.load_elision_stats()
    finally:
        w.close()
    what = f"{variant} {dtype} n={n}"
    print(what, tf, fix)
    assert fix["establish"] > 0 and fix["lean"] > 0, (what, fix)
    if variant in SHORT:
        assert tf["short"] > 0 and tf["general"] == 0, (what, tf)
    else:
        assert tf["short"] == 0 and tf["general"] > 0, (what, tf)
    _same_bits(got, ref, what, nan_allowed=variant == "inertia_zero")


def test_the_scenes_are_what_the_docstring_says():
    for n in GRIDS:
        s, _ = _scene("quat_scaled", n, "float32")
        big = (np.abs(s.quat) > 2).any(axis=1)
        assert np.flatnonzero(big).tolist() == [SCALED_BODY] and abs(np.linalg.norm(s.quat[SCALED_BODY]) - 3.0) < 1e-6
        s, gyro = _scene("aniso_gyro2", n, "float64")
        assert gyro == 2 and (s.mass == 2.5).all() and (s.inertia == np.array([0.3, 1.7, 0.9])).all() and s.avel.any()
        s, _ = _scene("inertia_zero", n, "float64")
        assert (s.inertia[:, 1] == 0).all() and (s.inertia[:, 0] == 1).all()
    assert 200 % 64 == 8 and 321 % 64 == 1
