"""integrate_free's short tick for bodies without torque (dmxBatchSetTorqueFree, csrc/dmx_torque_free.hpp) must not change a single
bit.  200 bodies -- three full tiles and one of 8 lanes -- of unit mass and identity inertia under gravity along y with seeded spin,
f32 and f64; every run is made with the path on (the default) and switched off, and the two states must be equal byte for byte;
the launch counts (dmxBatchTorqueFreeStats) say that kernels with the short tick ran where the rule says on and only there;
both must equal the CPU oracle in their bits (where the oracle holds a NaN the device must hold one too: a NaN's sign and payload
are the processor's, not the tick's).
  runs      12 ticks, one per launch (the out-of-place first launch of a collision-proof chunk, the establishing launches and the
            lean ones of the fixed-axis words), and 3 launches of 4 ticks; each with the body-collision proof on and off
  variants  plain; avel lanes holding -0.0, a denormal, +inf and NaN (the short tick keeps them as the general one does); one lane of
            the second tile with a NaN quaternion, one with its quaternion scaled by 3 (a component beyond 2: their wavefronts fall
            back to the general tick, the other tiles do not); a uniform anisotropic inertia with gyro 2 (the rule says off) and with
            gyro 0 (on); an inertia of 0 in one component (off); a force accumulator set on one body (the kernel with accumulators,
            which has no short tick); mixed masses (constants loaded per body: no short tick)."""
import functools

import numpy as np
import pytest

from __graft_entry__ import load_package

pkg = load_package()
B_ = pkg.batch
pytestmark = pytest.mark.gpu

H = 1.0 / 60.0
N = 200
TICKS = 12
DTYPES = ["float32", "float64"]
GRAVITY = (0.0, -9.8, 0.0)
# the variants for which csrc/dmx_torque_free.hpp's rule says on: uniform constants, no accumulators, no gyroscopic torque, 1/I finite
RULE_ON = {"plain", "avel_specials", "quat_nan", "quat_scaled", "aniso_gyro0"}
VARIANTS = ["plain", "avel_specials", "quat_nan", "quat_scaled", "aniso_gyro2", "aniso_gyro0", "inertia_zero", "force", "mixed_mass"]


def _scene(variant, dtype):
    """-> (scene, gyro mode, force or None)"""
    s = pkg.scenes.box_grid(20, 10, seed=11, spin=True, box_mass=False, plane=False).astype(dtype)
    assert s.n == N
    dt = np.dtype(dtype)
    gyro, force = 2, None
    if variant == "avel_specials":
        for body, comp, val in ((3, 0, -0.0), (70, 1, np.finfo(dt).smallest_subnormal * 3), (130, 2, np.inf), (195, 0, np.nan),
                                (66, 2, -0.0), (193, 1, -np.finfo(dt).smallest_subnormal)):
            s.avel[body, comp] = val
    elif variant == "quat_nan":
        s.quat[64 + 5, 2] = np.nan
    elif variant == "quat_scaled":
        s.quat[64 + 40] = 3.0 * np.array([0.8, 0.0, 0.6, 0.0])
    elif variant in ("aniso_gyro2", "aniso_gyro0"):
        s.inertia[:] = np.array([0.4, 1.7, 3.1], dt)
        gyro = 2 if variant == "aniso_gyro2" else 0
    elif variant == "inertia_zero":
        s.inertia[:, 1] = 0.0
        gyro = 0
    elif variant == "force":
        force = np.zeros((N, 3), dt)
        force[77] = (0.5, 2.0, -0.25)
    elif variant == "mixed_mass":
        s.mass[::3, 0] = 2.0
    return s, gyro, force


def _device(variant, dtype, on, proof, per_launch):
    s, gyro, force = _scene(variant, dtype)
    w = pkg.BatchWorld(N, dtype=dtype, gravity=GRAVITY)
    try:
        w.set_gyro_mode(gyro)
        w.set_torque_free(on)
        w.set_ticks_per_launch(per_launch)
        w.set_body_collisions(proof)
        w.load_scene(s)
        if force is not None:
            w.upload(B_.FORCE, force)
        for _ in range(TICKS // per_launch):
            w.step(H, per_launch)
        w.synchronize()
        return w.state(), w.torque_free_stats()
    finally:
        w.close()


@functools.lru_cache(maxsize=None)
def _oracle(variant, dtype):
    from oracle.orc_ctypes import Oracle
    s, gyro, force = _scene(variant, dtype)
    orc = Oracle(dtype)
    ow = orc.world(gravity=GRAVITY)
    orc.lib.orc_world_set_gyro_mode(ow.w, gyro)
    ow.add_boxes(s.pos, s.quat, s.lvel, s.avel, s.mass[:, 0], s.inertia, s.sides)
    if force is not None:
        for b in np.flatnonzero(force.any(axis=1)):
            orc.lib.orc_body_add_force(ow.w, int(b), *[float(x) for x in force[b]])
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


def _same_bytes(got, want, what):
    for name, a, b in zip(("pos", "quat", "lvel", "avel"), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape
        diff = _bits(a) != _bits(b)
        assert not diff.any(), (f"{what}: {name} differs in {int(diff.sum())} components, first at body/component {np.argwhere(diff)[0]}: "
                                f"{a[tuple(np.argwhere(diff)[0])]!r} against {b[tuple(np.argwhere(diff)[0])]!r}")


def _same_as_oracle(got, ref, what):
    for name, a, b in zip(("pos", "quat", "lvel", "avel"), got, ref):
        assert a.dtype == b.dtype and a.shape == b.shape
        nan = np.isnan(b)
        assert np.array_equal(np.isnan(a), nan), f"{what}: {name} is NaN where the oracle is not, or the other way round"
        diff = (_bits(a) != _bits(b)) & ~nan
        assert not diff.any(), (f"{what}: {name} differs from the oracle in {int(diff.sum())} components, first at body/component "
                                f"{np.argwhere(diff)[0]}: {a[tuple(np.argwhere(diff)[0])]!r} against {b[tuple(np.argwhere(diff)[0])]!r}")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_on_is_off_is_the_oracle(dtype, variant):
    ref = _oracle(variant, dtype)
    for per_launch in (1, 4):
        for proof in (False, True):
            what = f"{variant} {dtype}, {TICKS // per_launch} launches of {per_launch}, proof {'on' if proof else 'off'}"
            off, off_stats = _device(variant, dtype, False, proof, per_launch)
            on, on_stats = _device(variant, dtype, True, proof, per_launch)
            # which kernels ran: switched off, none with the short tick; switched on, every contact-free launch where the rule says
            # on and none where it says off (the quaternion guard inside such a launch is per wavefront and not counted: that the
            # lanes it must reject are rejected, and only those, is tests/test_torque_free.py's on the host)
            launches = TICKS // per_launch
            assert off_stats["short"] == 0 and off_stats["general"] > 0, (what, off_stats)
            if variant in RULE_ON:
                assert on_stats["short"] > 0 and on_stats["general"] == 0, (what, on_stats)
                if not proof:
                    assert on_stats["short"] == launches, (what, on_stats)
            elif variant == "force":
                # the accumulators act in the first tick alone (the kernel with accumulators, or the exact tick under the proof);
                # the launches behind it are the plain scene's
                assert on_stats["short"] > 0, (what, on_stats)
                if not proof:
                    assert on_stats["general"] == 1, (what, on_stats)
            else:
                assert on_stats["short"] == 0 and on_stats["general"] > 0, (what, on_stats)
            _same_bytes(on, off, what + ": path on against path off")
            _same_as_oracle(off, ref, what + ", path off")
            _same_as_oracle(on, ref, what + ", path on")


def test_the_scene_is_what_the_docstring_says():
    """the variants plant what they claim, in the lanes they claim (so that a fallback wavefront and a short one exist side by side)"""
    s, _, _ = _scene("quat_nan", "float32")
    bad = np.isnan(s.quat).any(axis=1)
    assert np.flatnonzero(bad).tolist() == [69]
    s, _, _ = _scene("quat_scaled", "float32")
    big = (np.abs(s.quat) > 2).any(axis=1)
    assert np.flatnonzero(big).tolist() == [104] and abs(np.linalg.norm(s.quat[104]) - 3.0) < 1e-6
    s, _, _ = _scene("avel_specials", "float32")
    assert np.signbit(s.avel[3, 0]) and s.avel[3, 0] == 0 and np.isinf(s.avel[130, 2]) and np.isnan(s.avel[195, 0])
    assert 0 < s.avel[70, 1] < np.finfo(np.float32).tiny
    s, _, _ = _scene("plain", "float64")
    assert (s.mass == 1).all() and (s.inertia == 1).all() and s.avel.any() and N % 64 == 8


def test_the_switch_validates_its_argument():
    w = pkg.BatchWorld(64, dtype="float32")
    try:
        for bad in (-1, 2):
            with pytest.raises(pkg.batch.DmxError):
                pkg.batch._check(w.lib.dmxBatchSetTorqueFree(w.h, bad), "dmxBatchSetTorqueFree")
        w.set_torque_free(False)
        w.set_torque_free(True)
    finally:
        w.close()
