"""integrate_free_lean, the straight-line kernel of a lean contact-free launch (dmxBatchSetLeanKernel, csrc/dmx_lean_tick.hpp,
csrc/dmx_kernels.hip), must not change a single bit, and must run exactly where launch_step's rule says: a lean launch
(dmx_fixed.hpp) with the constants as arguments and the short tick on, one tick, no accumulators.
  shapes    n in {1, 63, 64, 65, 255, 257, 2048 + 17}: a partial last tile, a partial workgroup, the surplus workgroups of a grid
            rounded up to 8, and -- at 2 065 bodies, 9 workgroups in a grid of 16 -- two tile groups, so that the reverse sweep differs
            from the forward one; 257 slots of which 132 are active (ghost slots)
  runs      6 one-tick calls with the body-body proof off (1 establishing launch, 5 lean ones in alternating directions); the same
            with a download behind every tick; the same with the proof on
  scenes    every tile fixed; one body with lateral velocity (its tile runs the shared tile body beside straight-line tiles);
            pos.x = -0.0 with lvel.x = +0.0 (the bit clears in the tick that makes it +0.0 and comes back); a NaN quaternion component
            and a quaternion with |q.k| > 2 (the guard fails); a signalling NaN and a -0.0 in avel; gyro modes 0, 1, 2 with isotropic
            inertia; a host upload of one body between two lean launches (the chain breaks and is established anew)
Every run is made with the kernel on (the default) and switched off: the two states must be equal byte for byte, both must equal
the CPU oracle (where the oracle holds a NaN the device must hold one too: a NaN's sign and payload are the processor's), and
dmxBatchLoadElisionStats must be the same for both."""
import functools

import numpy as np
import pytest

from __graft_entry__ import load_package

pkg = load_package()
B_ = pkg.batch
pytestmark = pytest.mark.gpu

H = 1.0 / 60.0
TICKS = 6
DTYPES = ["float32", "float64"]
GRAVITY = (0.0, -9.8, 0.0)
SIZES = [1, 63, 64, 65, 255, 257, 2048 + 17]
GHOSTS = (257, 132)            # slots, active (a multiple of 4, as dmxBatchSetActiveCount asks)
SCENES = ["fixed", "lateral", "neg_zero_x", "quat_guard", "avel_specials", "gyro0", "gyro1", "upload_between"]
RUNS = ["plain", "download", "proof"]


def _snan(dt):
    return np.array([0x7fa00001], np.uint32).view(np.float32)[0] if dt == np.float32 else np.array([0x7ff4000000000001], np.uint64).view(np.float64)[0]


@functools.lru_cache(maxsize=None)
def _full(dtype):
    return pkg.scenes.box_grid(59, 35, seed=7, spin=True, box_mass=False, plane=False).astype(dtype)


def _scene(name, dtype, n):
    """-> (scene, gyro mode); m = 1, I = identity (the reference's AddBody), dropped at rest with seeded spin"""
    f = _full(dtype)
    s = pkg.scenes.Scene(*(np.array(a[:n], copy=True) for a in (f.pos, f.quat, f.lvel, f.avel, f.mass, f.inertia, f.sides, f.gtype)), None)
    dt = np.dtype(dtype).type
    gyro = {"gyro0": 0, "gyro1": 1}.get(name, 2)
    mid, late = n // 2, (3 * n) // 4
    if name == "lateral":
        s.lvel[mid, 0] = 0.01
    elif name == "neg_zero_x":
        s.pos[mid, 0] = -0.0
        s.lvel[mid, 0] = 0.0
    elif name == "quat_guard":
        s.quat[mid, 2] = np.nan
        s.quat[late] = 3.0 * np.array([0.8, 0.0, 0.6, 0.0])
    elif name == "avel_specials":
        s.avel[mid, 1] = _snan(dt)
        s.avel[late, 0] = -0.0
    return s, gyro


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bytes(got, want, what, rows=slice(None)):
    for name, a, b in zip(("pos", "quat", "lvel", "avel"), got, want):
        a, b = a[rows], b[rows]
        assert a.dtype == b.dtype and a.shape == b.shape
        diff = _bits(a) != _bits(b)
        assert not diff.any(), f"{what}: {name} differs in {int(diff.sum())} components, first at body/component {np.argwhere(diff)[0]}"


def _same_as_oracle(got, ref, what, rows=slice(None)):
    for name, a, b in zip(("pos", "quat", "lvel", "avel"), got, ref):
        a, b = a[rows], b[rows]
        assert a.dtype == b.dtype and a.shape == b.shape
        nan = np.isnan(b)
        if not nan.any():
            assert np.array_equal(a, b), f"{what}: {name} differs from the oracle, max abs diff {np.max(np.abs(a - b))}"
        assert np.array_equal(np.isnan(a), nan), f"{what}: {name} is NaN where the oracle is not, or the other way round"
        diff = (_bits(a) != _bits(b)) & ~nan
        assert not diff.any(), f"{what}: {name} differs from the oracle in {int(diff.sum())} components, first at {np.argwhere(diff)[0]}"


UPLOAD_AT = 3                  # "upload_between": body n // 3 gets a new lvel after this many ticks
NEW_LVEL = (0.0, 1.25, 0.0)


@functools.lru_cache(maxsize=None)
def _oracle(name, dtype, n):
    from oracle.orc_ctypes import Oracle
    s, gyro = _scene(name, dtype, n)
    orc = Oracle(dtype)
    ow = orc.world(gravity=GRAVITY)
    orc.lib.orc_world_set_gyro_mode(ow.w, gyro)
    ow.add_boxes(s.pos, s.quat, s.lvel, s.avel, s.mass[:, 0], s.inertia, s.sides)
    if name == "upload_between":
        ow.run(orc.dtype.type(H), UPLOAD_AT)
        orc.lib.orc_body_set_linear_vel(ow.w, n // 3, *[float(v) for v in NEW_LVEL])
        ow.run(orc.dtype.type(H), TICKS - UPLOAD_AT)
    else:
        ow.run(orc.dtype.type(H), TICKS)
    assert ow.n_contacts() == 0
    st = ow.state()
    ow.close()
    for a in st:
        a.setflags(write=False)
    return st


def _device(name, dtype, n, run, on, n_active=None, setup=None, per_call=1, force=None):
    """-> (state, lean-kernel stats, load-elision stats)"""
    s, gyro = _scene(name, dtype, n)
    w = pkg.BatchWorld(n, dtype=dtype, gravity=GRAVITY)
    try:
        w.set_gyro_mode(gyro)
        w.set_lean_kernel(on)
        w.set_body_collisions(run == "proof")
        if setup:
            setup(w)
        w.load_scene(s)
        if n_active is not None:
            w.set_active_count(n_active)
        for t in range(0, TICKS, per_call):
            if name == "upload_between" and t == UPLOAD_AT:
                w.upload(B_.LVEL, np.array([NEW_LVEL], dtype), first=n // 3)
            if force is not None:
                w.upload(B_.FORCE, force)
            w.step(H, per_call)
            if run == "download":
                w.download(B_.POS)
        w.synchronize()
        lk = w.lean_kernel_stats()          # (the elision stats settle the batch: the kernel's counts first)
        return w.state(), lk, w.load_elision_stats()
    finally:
        w.close()


def _check_counts(lk, le, on, run, name, what):
    # the rule: every lean launch of these scenes (uniform unit constants, isotropic inertia, no accumulators, one tick) takes the
    # kernel when the switch is on, and no other launch does; off, none
    total = lk["lean_kernel"] + lk["other"]
    assert total > 0, (what, lk)
    if not on:
        assert lk["lean_kernel"] == 0, (what, lk)
        return
    assert lk["lean_kernel"] == le["lean"], (what, lk, le)       # (whatever a download or the proof does to the chain)
    if run == "plain":
        breaks = 1 if name == "upload_between" else 0
        assert lk == {"lean_kernel": TICKS - 1 - breaks, "other": 1 + breaks}, (what, lk)


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_on_is_off_is_the_oracle(dtype, name):
    for n in SIZES:
        ref = _oracle(name, dtype, n)
        for run in RUNS:
            what = f"{name} {dtype} n={n} {run}"
            off, off_lk, off_le = _device(name, dtype, n, run, False)
            on, on_lk, on_le = _device(name, dtype, n, run, True)
            _check_counts(off_lk, off_le, False, run, name, what)
            _check_counts(on_lk, on_le, True, run, name, what)
            assert on_le == off_le, (what, on_le, off_le)
            _same_bytes(on, off, what + ": kernel on against kernel off")
            _same_as_oracle(off, ref, what + ", kernel off")
            _same_as_oracle(on, ref, what + ", kernel on")


@pytest.mark.parametrize("dtype", DTYPES)
def test_ghost_slots_are_left_alone(dtype):
    n, act = GHOSTS
    ref = _oracle("lateral", dtype, n)
    s, _ = _scene("lateral", dtype, n)
    start = (s.pos, s.quat, s.lvel, s.avel)
    for run in RUNS:
        what = f"ghost slots {dtype} {run}"
        off, off_lk, off_le = _device("lateral", dtype, n, run, False, n_active=act)
        on, on_lk, on_le = _device("lateral", dtype, n, run, True, n_active=act)
        _check_counts(on_lk, on_le, True, run, "lateral", what)
        assert on_le == off_le, (what, on_le, off_le)
        _same_bytes(on, off, what)
        _same_as_oracle(on, ref, what, rows=slice(0, act))
        _same_bytes(on, start, what + ": ghost slots", rows=slice(act, n))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_kernel_is_taken_nowhere_the_rule_says_no(dtype):
    n = 257
    dt = np.dtype(dtype)
    cases = {}

    def run_with(mutate=None, setup=None, per_call=1, force=None, on=True, gyro=None):
        w = pkg.BatchWorld(n, dtype=dtype, gravity=GRAVITY)
        try:
            sc, g = _scene("fixed", dtype, n)
            if mutate:
                mutate(sc)
            w.set_gyro_mode(g if gyro is None else gyro)
            w.set_lean_kernel(on)
            if setup:
                setup(w)
            w.load_scene(sc)
            for _ in range(0, 8, per_call):
                if force is not None:
                    w.upload(B_.FORCE, force)
                w.step(H, per_call)
            w.synchronize()
            return w.lean_kernel_stats(), w.load_elision_stats()
        finally:
            w.close()

    def mix_mass(sc):
        sc.mass[::3, 0] = 2.0

    def aniso(sc):
        sc.inertia[:] = np.array([0.4, 1.7, 3.1], dt)

    force = np.zeros((n, 3), dt)
    force[77] = (0.0, 2.0, 0.0)
    cases["mixed masses"] = run_with(mutate=mix_mass)
    cases["anisotropic inertia, gyro 2"] = run_with(mutate=aniso, gyro=2)
    cases["anisotropic inertia, gyro 1"] = run_with(mutate=aniso, gyro=1)
    cases["force accumulators at every launch"] = run_with(force=force)
    cases["4 ticks per launch"] = run_with(setup=lambda w: w.set_ticks_per_launch(4), per_call=4)
    cases["switch off"] = run_with(on=False)
    for what, (lk, le) in cases.items():
        assert lk["lean_kernel"] == 0 and lk["other"] > 0, (what, lk, le)
    # ... and the same loop with nothing in the way takes it at every lean launch; anisotropic inertia with gyro 0 has no torque either
    lk, le = run_with()
    assert lk == {"lean_kernel": 7, "other": 1} and le["lean"] == 7, (lk, le)
    lk, le = run_with(mutate=aniso, gyro=0)
    assert lk == {"lean_kernel": 7, "other": 1} and le["lean"] == 7, (lk, le)


def test_the_scenes_are_what_the_docstring_says():
    s, _ = _scene("quat_guard", "float32", 257)
    assert np.flatnonzero(np.isnan(s.quat).any(axis=1)).tolist() == [128]
    assert np.flatnonzero((np.abs(s.quat) > 2).any(axis=1)).tolist() == [192]
    s, _ = _scene("neg_zero_x", "float64", 65)
    assert np.signbit(s.pos[32, 0]) and s.pos[32, 0] == 0 and not np.signbit(s.lvel[32, 0])
    s, _ = _scene("avel_specials", "float32", 2065)
    assert np.isnan(s.avel[1032, 1]) and _bits(s.avel)[1032, 1] == 0x7fa00001 and np.signbit(s.avel[1548, 0])
    s, _ = _scene("fixed", "float64", 2065)
    assert (s.mass == 1).all() and (s.inertia == 1).all() and s.avel.any() and not s.lvel.any()
    assert pkg.scenes.box_grid(59, 35, plane=False).n == 2048 + 17


def test_the_switch_validates_its_argument():
    w = pkg.BatchWorld(64, dtype="float32")
    try:
        for bad in (-1, 2):
            with pytest.raises(pkg.batch.DmxError):
                pkg.batch._check(w.lib.dmxBatchSetLeanKernel(w.h, bad), "dmxBatchSetLeanKernel")
        w.set_lean_kernel(False)
        w.set_lean_kernel(True)
    finally:
        w.close()
