"""The whole tick against the oracle, bit for bit, in worlds that are not y-up (tests/rotated_worlds.py: y_up as control, z_up,
x_up, down, tilted).  The product tells (x, z) from y in many places -- safe zones are discs in (x, z), the hashed grid works per
(x, z) column, `ballistic` asks for gravity along y alone, the per-tile "lateral axis fixed" words are kept for x and z,
near_static is an AABB test, the hull tile form filters with one dot product -- each an optimisation that must stay correct for
any gravity and plane.  ODE's own convention is z-up.

a. twelve of the fuzz scenes (tests/test_gpu_fuzz.py::_scene), the seed's full parameters, friction included, in the four
   rotated orientations, 150 ticks;
b. scenes aimed at one path each, in all five orientations, each asserting through collision_stats() that the path was reached.
   A grid laid out "horizontally" in y-up shares (x, z) columns once the world is turned, bp_safe_zone calls it crowded and every
   tick is exact -- correct, but the fused kernels never run.  So the fused-path scenes are a single row of 96 bodies (two tiles
   and a 32-lane tail) laid along the axis that stays lateral: box_grid(1, n) for z_up, box_grid(n, 1) for x_up.  What the
   stats showed about the paths a turned world reaches is in DESIGN.md section 3; the one path an orientation cannot reach
   (free flight at 60 Hz under lateral gravity) is asserted as careful_ticks == steps.

Parity needs no equivariance: device and oracle get the same rotated numbers (tests/test_rotated_worlds_reference.py pins the
oracle's own behaviour under rotation)."""
import dataclasses
import functools

import numpy as np
import pytest

import rotated_worlds as rw
from __graft_entry__ import load_package
from test_gpu_fuzz import _scene

pkg = load_package()
B = pkg.batch
pytestmark = pytest.mark.gpu
H = rw.H
N_ROW = 96


def _same(got, ref, what=""):
    for name, a, r in zip(("pos", "quat", "lvel", "avel"), got, ref):
        assert np.all(np.isfinite(r)), f"{what}: oracle {name} not finite"
        assert np.array_equal(a, r), (f"{what} {name}: max abs diff {np.max(np.abs(a - r))} at body "
                                      f"{int(np.argmax(np.abs(a - r).max(axis=1)))} of {len(a)}")


# ---------------------------------------------------------------------------------------------------------------------- a
FUZZ_SEEDS = tuple(range(12))      # both precisions; 1, 4, 7, 10 without static boxes; 0, 3, 6, 9 with hulls


@pytest.mark.parametrize("name", rw.ROTATED)
@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_random_scene_matches_oracle_in_a_rotated_world(seed, name):
    scene, dtype, p, nb = _scene(seed)
    scene, g = rw.rotate_scene(scene, name, dtype)
    steps = 150
    w = rw.device_world(pkg, scene, dtype, p, g)
    w.step(H, steps)
    w.synchronize()
    ow = rw.oracle_world(scene, dtype, p, g)
    ow.run(H, steps)
    _same(w.state(), ow.state(), f"seed {seed} {dtype} {name} (boxes/spheres {nb}; {p})")
    assert w.last_contact_count() == ow.n_contacts()
    w.close()


# ---------------------------------------------------------------------------------------------------------------------- b
LATERAL_GRAVITY = ("z_up", "x_up", "tilted")      # gravity has a component in the (x, z) plane of the safe-zone discs
WIDE = 8.0                                        # their rows: 20 m between neighbours where the others have the grid's 2.5 m


def _row(name, wide=True, **kw):
    """a single row of N_ROW boxes whose rotated (x, z) positions stay apart -> (scene, the axis the row lies along).

    Where gravity acts inside the (x, z) plane, falling IS leaving the safe zone: a zone's radius is at most 0.75 r_max - r_i / 2
    (the hashed grid's cell bounds it, however far the neighbours are: about 0.5 m for these boxes), and a body released from
    rest falls 1.44 m in the 32 ticks of the shortest fast chunk.  So while such a world's bodies fall every chunk is rolled back
    and stepped exactly, and the fused kernels run once they rest.  At the grid's 2.5 m pitch the z_up row on the plane got no
    clean chunk in 150 ticks; WIDE times as far apart it does."""
    along = 0 if name == "x_up" else 2
    scene = pkg.scenes.box_grid(N_ROW, 1, **kw) if name == "x_up" else pkg.scenes.box_grid(1, N_ROW, **kw)
    if wide and name in LATERAL_GRAVITY:
        scene.pos[:, along] *= WIDE
    return scene, along


def _run_both(scene, dtype, g, steps, setup=None, count_pairs=False, h=H):
    """-> (device state, collision_stats, device contact count, oracle state, oracle contact count, oracle body pairs summed)"""
    w = rw.device_world(pkg, scene, dtype, None, g)
    if setup:
        setup(w)
    w.step(h, steps)
    w.synchronize()
    got, st, nc = w.state(), w.collision_stats(), w.last_contact_count()
    w.close()
    ow = rw.oracle_world(scene, dtype, None, g)
    pairs = 0
    if count_pairs:
        for _ in range(steps):
            ow.tick(h)
            pairs += ow.n_body_pairs()
    else:
        ow.run(h, steps)
    out = got, st, nc, ow.state(), ow.n_contacts(), pairs
    ow.close()
    return out


FREE_STEPS = 200
FREE_FLIGHT = [(name, dtype, ticks, hz) for name in rw.ORIENTATIONS for dtype in ("float64", "float32") for ticks in (1, 8)
               for hz in (60, 240)]


@functools.lru_cache(maxsize=None)
def _free_flight(name, dtype, ticks, hz):
    scene, along = _row(name, wide=False, seed=77, y_range=(20.0, 26.0), spin=True, box_mass=True, plane=False)
    rng = np.random.default_rng(9)
    across = 2 - along
    scene.lvel[:, along] = np.where(np.arange(scene.n) % 2 == 0, 0.25, -0.25)      # neighbours close in on one another by pairs
    scene.lvel[:, across] = rng.uniform(-0.25, 0.25, scene.n)
    scene, g = rw.rotate_scene(scene, name, dtype)
    got, st, _, ref, _, pairs = _run_both(scene, dtype, g, FREE_STEPS, lambda w: w.set_ticks_per_launch(ticks), count_pairs=True,
                                          h=1.0 / hz)
    print(f"free flight {name} {dtype} tpl {ticks} {hz} Hz: {st}, oracle body pairs {pairs}")
    return got, st, ref, pairs


@pytest.mark.parametrize("name,dtype,ticks,hz", FREE_FLIGHT)
def test_free_flight_checked(name, dtype, ticks, hz):
    """integrate_free with the safe-zone check fused in: no plane, the row drifting sideways into its neighbours, 200 ticks.
    x_up, z_up and tilted are not ballistic (gravity has an x or a z component), so the check rides every tick; down is ballistic
    with gravity +y.

    At 60 Hz a world with lateral gravity cannot reach the kernel at all: from rest a body falls 1.44 m in the shortest chunk's
    32 ticks (0.96 m under `tilted`), further in every later one, and no zone is wider than 0.75 r_max -- every chunk is rolled
    back and every tick exact, which is asserted as such.  At 240 Hz the first chunks fit (9 cm), and the
    later ones are rolled back, rebuilt and retried as the bodies gather speed."""
    got, st, ref, _ = _free_flight(name, dtype, ticks, hz)
    _same(got, ref, f"free flight {name} {dtype} tpl {ticks} {hz} Hz")
    if name in LATERAL_GRAVITY and hz == 60:
        assert st["careful_ticks"] == FREE_STEPS and st["fast_ticks"] == 0, st
    else:
        assert st["fast_ticks"] > 0, st


def test_free_flight_met_rollbacks_or_rebuilds():
    """over the orientations: the drifting row violated its zones somewhere -- zones rebuilt, exact ticks taken, body pairs met"""
    runs = [_free_flight(*case) for case in FREE_FLIGHT]
    assert sum(st["rebuilds"] for _, st, _, _ in runs) > 0
    assert sum(st["careful_ticks"] for _, st, _, _ in runs) > 0
    assert sum(pairs for _, _, _, pairs in runs) > 0
    for name in LATERAL_GRAVITY:            # the checked kernel ran under lateral gravity, and its check fired
        mine = [st for case, (_, st, _, _) in zip(FREE_FLIGHT, runs) if case[0] == name and case[3] == 240]
        assert all(0 < st["fast_ticks"] < FREE_STEPS and st["rebuilds"] > 1 for st in mine), (name, mine)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", rw.ORIENTATIONS)
def test_row_dropped_on_the_plane(name, dtype):
    """step_plane: the row dropped from 0.7-3 m onto the rotated ground plane"""
    scene, _ = _row(name, seed=5, y_range=(0.7, 3.0), spin=True, box_mass=True, plane=True)
    scene, g = rw.rotate_scene(scene, name, dtype)
    steps = 150
    got, st, nc, ref, nco, _ = _run_both(scene, dtype, g, steps)
    print(f"plane {name} {dtype}: {st}, contacts {nc}")
    _same(got, ref, f"plane {name} {dtype}")
    assert nc == nco and nc > 0
    assert st["fast_ticks"] > 0, st


def _row_over_floor_and_post(name):
    scene, along = _row(name, seed=5, y_range=(0.7, 3.0), spin=True, box_mass=True, plane=False)
    k = 10
    span = float(np.ptp(scene.pos[:, along])) + 100.0
    floor = ((span, 1.0, span), (0.0, -0.5, 0.0), pkg.scenes._rot_z(0.0))
    post = ((0.7, 1.0, 0.7), (float(scene.pos[k, 0]) + 0.2, 0.45, float(scene.pos[k, 2]) - 0.1), pkg.scenes._rot_z(0.3))
    return dataclasses.replace(scene, static_boxes=[floor, post])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", rw.ORIENTATIONS)
def test_row_dropped_on_a_static_floor_and_a_post(name, dtype):
    """np_static -> step_contacts: the same row over a rotated floor box and one rotated post; the fused path, the exact tick it
    replaces (set_static_path) and the oracle give the same bits"""
    scene, g = rw.rotate_scene(_row_over_floor_and_post(name), name, dtype)
    steps = 150
    states = {}
    for fused in (True, False):
        got, st, nc, ref, nco, _ = _run_both(scene, dtype, g, steps, lambda w: w.set_static_path(fused))
        print(f"static {name} {dtype} fused={fused}: {st}, contacts {nc}")
        _same(got, ref, f"static {name} {dtype} fused={fused}")
        assert nc == nco and nc > 0
        if fused:
            assert st["fast_ticks"] > 0, st
        else:
            assert st["careful_ticks"] > 0, st
        states[fused] = got
    _same(states[True], states[False], f"static {name} {dtype} fused against exact")


@pytest.mark.parametrize("pipeline", [B.EXACT_STAGED, B.EXACT_ONE_WORKGROUP], ids=["staged", "one-workgroup"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", rw.ORIENTATIONS)
def test_pile_in_the_rotated_pen(name, dtype, pipeline):
    """the exact tick: 24 of the spawner's boxes and spheres piling up over the rotated floor and walls, body pairs and islands"""
    scene, statics, _ = pkg.scenes.reference_pen(24, seed=7, y_range=(1.5, 6.0))
    scene, g = rw.rotate_scene(dataclasses.replace(scene, static_boxes=statics), name, dtype)
    steps = 120
    got, st, nc, ref, nco, pairs = _run_both(scene, dtype, g, steps, lambda w: w.set_exact_pipeline(pipeline), count_pairs=True)
    print(f"pen {name} {dtype} pipeline {pipeline}: {st}, contacts {nc}, oracle body pairs {pairs}")
    _same(got, ref, f"pen {name} {dtype} pipeline {pipeline}")
    assert nc == nco and nc > 24 and pairs > 0
    assert st["pair_ticks"] > 0 and st["careful_ticks"] > 0, st


@functools.lru_cache(maxsize=None)
def _small_hull():
    rng = np.random.default_rng(40)
    return pkg.hull.build(rng.normal(size=(40, 3)) * np.array([0.3, 0.2, 0.25]))


@pytest.mark.parametrize("floor_box", [False, True], ids=["plane", "floor-box"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", rw.ORIENTATIONS)
def test_row_of_hulls(name, dtype, floor_box):
    """np_convex_plane, and the static hull forms with their filter: sixteen small hulls (a 40-point random hull), tipped and
    spinning, on the rotated plane / on a rotated floor box"""
    nx, nz = (16, 1) if name == "x_up" else (1, 16)
    scene = pkg.scenes.hull_grid(_small_hull(), nx, nz, seed=11, y_range=(0.7, 1.4), spin=True, tilt=0.6, floor_box=floor_box)
    scene, g = rw.rotate_scene(scene, name, dtype)
    steps = 150
    got, st, nc, ref, nco, _ = _run_both(scene, dtype, g, steps)
    print(f"hulls {name} {dtype} floor_box={floor_box}: {st}, contacts {nc}")
    _same(got, ref, f"hulls {name} {dtype} floor_box={floor_box}")
    assert nc == nco and nc > 0
    assert st["fast_ticks"] > 0, st


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name,nx,nz", [("z_up", 4, 40), ("z_up", 40, 4), ("x_up", 4, 40), ("x_up", 40, 4)])
def test_bucket_growth_in_its_natural_habitat(name, nx, nz, dtype):
    """what a z-up user produces by default: a resting grid whose bodies share (x, z) columns of the hashed grid -- in z_up
    box_grid(40, 4) puts 40 bodies in each of 4 columns and box_grid(4, 40) 4 in each of 40; in x_up it is the other way round"""
    scene = pkg.scenes.box_grid(nx, nz, seed=3, y_range=(0.5, 0.6), spin=False, box_mass=True, plane=True)
    scene, g = rw.rotate_scene(scene, name, dtype)
    lateral = np.round(scene.pos[:, [0, 2]].astype(np.float64) / 1.25)          # half the pitch: the heights differ by 0.1 m at most
    assert len({tuple(c) for c in lateral}) == (nz if name == "z_up" else nx)
    steps = 20
    got, st, nc, ref, nco, _ = _run_both(scene, dtype, g, steps)
    print(f"columns {name} {nx}x{nz} {dtype}: {st}, contacts {nc}")
    _same(got, ref, f"columns {name} {nx}x{nz} {dtype}")
    assert nc == nco and nc > 0
    assert st["careful_ticks"] == steps and st["crowded"] == scene.n, st        # columns shared: every body crowded, every tick exact
