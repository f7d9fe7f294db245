"""The ODE API, z-up: ODE's own convention and what most ODE programs set up -- dWorldSetGravity(w, 0, 0, -g) and
dCreatePlane(s, 0, 0, 1, 0).  The C harness (tests/harness/ode_tick_harness.c, HARNESS_GRAVITY / HARNESS_PLANE) makes the
reference's sequence of calls in the z_up image of the scenes the y-up tests use (tests/rotated_worlds.py), against an oracle
world with the same gravity, plane and poses: dWorldQuickStep bit for bit, dWorldStep within the 1e-5 `_rel` bound of
tests/test_ode_compat.py and tests/test_gpu_lcp_grid.py."""
import functools
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import rotated_worlds as rw
from __graft_entry__ import load_package
from test_gpu_lcp_grid import _pyramid, _stats
from test_ode_compat import _build_harness, _oracle_poses, _rel, _scene_text

pkg = load_package()
pytestmark = pytest.mark.gpu

NAME = "z_up"
DT = 1.0 / 120.0
GRAVITY = rw.rotate_gravity(NAME)                          # (0, 0, -9.8)
PLANE = rw.rotate_plane(NAME, (0.0, 1.0, 0.0, 0.0))        # (0, 0, 1, 0)
BODY_R = rw.rotate_static(NAME, ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), pkg.scenes._rot_z(0.0)))[2]     # R itself: what an upright body becomes
ENV = {"HARNESS_GRAVITY": " ".join(repr(v) for v in GRAVITY), "HARNESS_PLANE": " ".join(repr(v) for v in PLANE)}
_TMP = tempfile.mkdtemp(prefix="rotated_ode_")


@functools.lru_cache(maxsize=None)
def _exe(single):
    return _build_harness(_TMP, single)


def _z_up(statics, bodies):
    """the z_up image of a y-up scene: static boxes turned, bodies moved (they start with rotation R: BODY_R)"""
    return ([rw.rotate_static(NAME, s) for s in statics],
            [(kind, size, tuple(float(c) for c in rw.rotate_vectors(NAME, pos))) for kind, size, pos in bodies])


def _run(single, text, stepper, env=None):
    """-> (poses (n, 16), stderr) of one harness process in the z-up world"""
    p = subprocess.run([_exe(single)], input=text, capture_output=True, text=True, timeout=600,
                       env={**os.environ, "HARNESS_STEPPER": stepper, **ENV, **(env or {})})
    assert p.returncode == 0, p.stderr[-2000:]
    return np.array([[float(v) for v in line.split()] for line in p.stdout.strip().splitlines()]), p.stderr


def test_the_z_up_world_is_odes_own():
    assert GRAVITY == (0.0, 0.0, -9.8) and PLANE == (0.0, 0.0, 1.0, 0.0)
    assert BODY_R == [0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]


@pytest.mark.parametrize("stepper", ["quick", "exact"])
@pytest.mark.parametrize("single", [False, True], ids=["f64", "f32"])
def test_pen_of_24_bodies_on_the_single_launch_tick(single, stepper):
    """the reference's pen, turned z-up, with 24 of the spawner's bodies: every tick is one launch (the small tick says so).
    120 ticks: the bodies have landed (17-26 contacts) and float32 is still comparable -- two float32 solvers on a pile drift
    apart by a factor of 100 in the next 80 ticks whatever the orientation (dWorldStep against the oracle, this scene, float32:
    2.3e-6 y-up and 2.9e-6 z-up after 120 ticks, 1.8e-4 both after 200; float64: 3e-13 / 6e-13 and 2e-10 / 2e-10)"""
    dtype = "float32" if single else "float64"
    steps = 120
    statics, bodies = _z_up(pkg.scenes.reference_map(), pkg.scenes.reference_spawn(24, seed=21, y_range=(1.2, 5.0)))
    got, err = _run(single, _scene_text(DT, steps, False, statics, bodies, body_R=BODY_R), stepper, env={"DMX_SMALL_TICK_REPORT": "1"})
    rep = {}
    for line in re.findall(r"small tick: (.*)", err):
        for kv in line.split():
            k, v = kv.split("=")
            rep[k] = rep.get(k, 0) + int(v)
    assert rep.get("small") == steps and rep.get("general") == 0, (rep, err[-500:])
    ref, ow = _oracle_poses(dtype, DT, steps, False, statics, bodies, exact=stepper == "exact", gravity=GRAVITY, body_R=BODY_R)
    assert ow.n_contacts() >= 12                                         # landed (17 under QuickStep, 24-26 under dWorldStep)
    assert np.all(np.isfinite(got)) and got[:, 14].min() > 0.4         # on the floor, whose top is now at z = 0.5
    if stepper == "quick":
        assert np.array_equal(got.astype(ref.dtype), ref), np.abs(got - ref).max()
    else:
        err_rel = _rel(got.astype(ref.dtype), ref)
        print(f"z-up pen, dWorldStep, {dtype}: rel err vs the oracle's exact stepper {err_rel:.3e}")
        assert err_rel <= 1e-5


@pytest.mark.parametrize("single", [False, True], ids=["f64", "f32"])
def test_pyramid_through_the_grid_solve(single):
    """tests/test_gpu_lcp_grid.py's pyramid of 30 boxes, turned z-up: one island of hundreds of rows, four ticks of dWorldStep,
    each one grid solve"""
    dtype = "float32" if single else "float64"
    steps = 4
    y_up = _pyramid(4)
    statics, bodies = _z_up(pkg.scenes.reference_map()[:1], y_up)
    got, err = _run(single, _scene_text(DT, steps, False, statics, bodies, body_R=BODY_R), "exact", env={"DMX_LCP_REPORT": "1"})
    st = _stats(err)
    assert st["solves"] == steps and st["last_m"] >= 600 and st["last_nu"] == 2 * st["last_nbd"] and st["fallback"] == 0
    ref, ow = _oracle_poses(dtype, DT, steps, False, statics, bodies, exact=True, gravity=GRAVITY, body_R=BODY_R)
    # (boxes of one layer touch their neighbours at depth 0: which of those contacts exist after a tick is decided by the last
    # bit of two solvers that agree to 1e-5, so the row counts agree to a few contacts, not to the row)
    print(f"z-up pyramid {dtype}: oracle rows {3 * ow.n_contacts()}, device rows {st['last_m']}")
    assert abs(3 * ow.n_contacts() - st["last_m"]) <= 0.02 * st["last_m"]
    assert _rel(got.astype(ref.dtype), ref) <= 1e-5
    assert np.max(np.abs(got[:, 14] - np.array([b[2][1] for b in y_up]))) < 2e-3          # and the pyramid stands, along z


@pytest.mark.parametrize("single", [False, True], ids=["f64", "f32"])
def test_48_by_48_boxes_over_the_plane_z_0(single):
    """2 304 bodies (more than 2 048: dSpaceCollide's pairs come from the device search) on a 48 x 48 grid in the (x, y) plane
    of a z-up world -- 48 bodies in every (x, z) column of the hashed grid -- three ticks of QuickStep"""
    dtype = "float32" if single else "float64"
    rng = np.random.default_rng(48)
    PITCH = 0.8               # the spawner's boxes have sides of 0.2-1.0 m: neighbours' AABBs overlap from the first tick, some boxes too
    y_up = []
    for k in range(48 * 48):
        kind, size, _ = pkg.scenes.reference_spawn(1, seed=2000 + k)[0]
        y_up.append((kind, size, (PITCH * (k % 48) - 24 * PITCH, 0.55 + 0.3 * rng.random(), PITCH * (k // 48) - 24 * PITCH)))
    _, bodies = _z_up([], y_up)
    pos = np.array([b[2] for b in bodies])
    assert len(np.unique(np.round(pos[:, 0] / PITCH))) == 48 and np.ptp(pos[:, 2]) < 0.3      # 48 columns of 48 bodies each
    steps = 3
    got, _ = _run(single, _scene_text(DT, steps, True, [], bodies, body_R=BODY_R), "quick")
    ref, ow = _oracle_poses(dtype, DT, steps, True, [], bodies, gravity=GRAVITY, plane=PLANE, body_R=BODY_R)
    assert ow.n_body_pairs() > 100 and ow.n_contacts() > 100
    assert np.array_equal(got.astype(ref.dtype), ref), np.abs(got - ref).max()
