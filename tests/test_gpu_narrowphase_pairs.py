"""The device narrowphase, pair by pair, against the oracle: thousands of ISOLATED pairs in adversarial poses
(tests/pair_population.py; tests/test_pair_population.py holds their coverage conditions) in one world, stepped ONE tick, every
body's state compared with the oracle's bit for bit, the tick's contact count too.  A contact wrong in position, normal, depth,
count or order changes the velocity bits of its two bodies and of nothing else, so a mismatch names its pair; the message carries
what rebuilds that pair alone.  A second tick follows, from poses that are no longer the generator's round numbers.

What each parametrisation reaches (csrc/): ex_narrow, ex_narrow_convex (wave_box_convex, wave_sphere_convex, wave_convex_plane),
ex_narrow_hull_pairs (wg_convex_convex) in both slot orders; step_plane's box / sphere colliders and np_convex_plane (on_plane);
np_static and np_convex_static_tile against ex_narrow's / ex_narrow_convex's static entries (set_static_path); np_convex_static by
launch_np_static's own rule (a 2 400-point hull) and by DMX_HULL_WAVE_PER_BODY; the filters off and on (DMX_HULL_FILTER = 0, 2)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pair_population as pp
from pair_population import pkg

pytestmark = pytest.mark.gpu
H = pp.H
DTYPES = ["float64", "float32"]
TICKS = 2
HULL_POPS = ("hull_hull", "sphere_hull", "box_hull")
DEFAULT_SHAPE = "ell65"


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _pop(name, shape=None, first=None):
    p = pp.get(name, shape)
    return p if first is None else p.first(first)


@functools.lru_cache(maxsize=None)
def _oracle_ticks(name, shape, first, dtype, far, max_contacts):
    """the oracle's side, computed once per (population, precision, place, max_contacts) and shared: per tick the state, the contact
    count and the joints' (body1, body2, pos, normal, depth)"""
    pop = _pop(name, shape, first)
    orc, ow, sc = pp.oracle_world(pop, dtype, pp.FAR if far else None, max_contacts)
    out = []
    for _ in range(TICKS):
        ow.tick(orc.dtype.type(H))
        state = ow.state()
        for a in state:
            a.setflags(write=False)
        out.append((state, ow.n_contacts(), None))
    return sc, out


def _explain(pop, sc, dtype, far, max_contacts, tick, bad_bodies, before=None):
    """the differing cells: classes in slot order, poses and sizes as repr (the scene's own values, in its precision), the oracle's
    contacts of that cell in the failing tick"""
    cells = sorted({int(pop.cell[b]) for b in bad_bodies})
    orc, ow, _ = pp.oracle_world(pop, dtype, pp.FAR if far else None, max_contacts)
    for _ in range(tick + 1):
        ow.tick(orc.dtype.type(H))
    js = ow.joints()
    lines = [f"{len(cells)} differing cells of {pop.name} ({dtype}, far={far}, max_contacts={max_contacts}, tick {tick + 1}): {cells[:40]}"]
    for c in cells[:6]:
        lines.append(pop.describe([c], sc) + ("" if before is None else "   (the scene as loaded; the failing tick started from:)"))
        if before is not None:
            for i in np.flatnonzero(pop.cell == c):
                lines.append("    slot %d before the failing tick: pos=%r quat=%r lvel=%r avel=%r" % ((int(i),) + tuple(a[i] for a in before)))
        for j in js:
            if pop.cell[j[0]] == c:
                lines.append(f"    oracle contact: bodies ({j[0]}, {j[1]}) pos={j[2]!r} normal={j[3]!r} depth={j[4]!r}")
    if sc.static_boxes:
        lines.append(f"  static boxes: {sc.static_boxes!r}"[:4000])
    if sc.plane is not None:
        lines.append(f"  plane: {sc.plane!r}")
    if pop.hull is not None:
        lines.append(f"  hull: pair_population.hull_shape({pop.hull.name!r})")
    return "\n".join(lines)


def _one_tick_parity(name, dtype, shape=None, first=None, far=False, max_contacts=8, pipeline=None, static_fused=None, summary=None):
    """load, set max_contacts, step 1/60 once, compare state (values and bit patterns), contact count, unsupported pairs; then a
    second tick, compared again.  Returns the device's states, tick by tick."""
    pop = _pop(name, shape, first)
    sc, ref = _oracle_ticks(name, shape, first, dtype, far, max_contacts)
    w = pkg.BatchWorld(sc.n, dtype=dtype)
    try:
        w.set_max_contacts(max_contacts)
        if pipeline is not None:
            w.set_exact_pipeline(pipeline)
        if static_fused is not None:
            w.set_static_path(fused=static_fused)
        w.load_scene(sc)
        states = []
        for t in range(TICKS):
            w.step(np.dtype(dtype).type(H), 1)
            w.synchronize()
            got = w.state()
            want, n_contacts, _ = ref[t]
            bad = np.zeros(sc.n, bool)
            for a, b in zip(got, want):
                assert a.dtype == b.dtype
                bad |= np.any(_bits(a) != _bits(b), axis=1) | np.any(a != b, axis=1)        # -0.0 / +0.0 differ in bits only; NaN in value only
            if bad.any():
                worst = max(float(np.nanmax(np.abs(a.astype(float) - b.astype(float)))) for a, b in zip(got, want))
                raise AssertionError(f"{int(bad.sum())} bodies differ from the oracle (max abs diff {worst:g})\n"
                                     + _explain(pop, sc, dtype, far, max_contacts, t, np.flatnonzero(bad), ref[t - 1][0] if t else None))
            assert w.last_contact_count() == n_contacts, f"tick {t + 1}: {w.last_contact_count()} contacts on the device, {n_contacts} in the oracle"
            states.append(got)
        assert w.collision_stats()["unsupported_pairs"] == 0
        print(f"PARITY {pop.name} {dtype} far={far} maxc={max_contacts} pipeline={pipeline} fused={static_fused}: "
              f"{int(pop.cell.max()) + 1} cells, {sc.n} bodies, contacts {ref[0][1]} then {ref[1][1]}")
        return states
    finally:
        w.close()


def _key(key):
    return dict(name=key[0], shape=key[1])


# ---------------------------------------------------------------------------------------------------- every population, both precisions
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("key", pp.ALL, ids=pp.pop_id)
def test_population(key, dtype):
    _one_tick_parity(dtype=dtype, **_key(key))


@pytest.mark.parametrize("key", pp.ALL, ids=pp.pop_id)
def test_population_far_from_the_origin_f32(key):
    """every population translated by (4 096, 0, -2 560) m, float32: positions round to 0.25-0.5 mm"""
    _one_tick_parity(dtype="float32", far=True, **_key(key))


_MAXC_KEYS = [k for k in pp.ALL if k[0] in ("box_box", "box_hull", "hull_hull", "on_statics")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("max_contacts", [4, 1])           # (8 is test_population's)
@pytest.mark.parametrize("key", _MAXC_KEYS, ids=pp.pop_id)
def test_max_contacts(key, max_contacts, dtype):
    """4: cull_points picks among dBoxBox's clipped points by angle; the hull walks stop at the cap; 1: the deepest / first only"""
    _one_tick_parity(dtype=dtype, max_contacts=max_contacts, **_key(key))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["staged", "one_workgroup"])
@pytest.mark.parametrize("key", [("box_box", None), ("hull_hull", DEFAULT_SHAPE), ("on_plane", None)], ids=pp.pop_id)
def test_exact_pipeline_forms(key, form, dtype):
    """the exact tick's bookkeeping forced to its staged and to its one-workgroup form (whose limit is 1 024 slots: the first 512 pairs)"""
    if form == "staged":
        _one_tick_parity(dtype=dtype, pipeline=pkg.batch.EXACT_STAGED, **_key(key))
    else:
        _one_tick_parity(dtype=dtype, pipeline=pkg.batch.EXACT_ONE_WORKGROUP, first=1024, **_key(key))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fused", [True, False])
def test_static_paths(fused, dtype):
    """np_static / np_convex_static_tile (fused) against the static entries of ex_narrow / ex_narrow_convex (every body the exact tick's)"""
    _one_tick_parity("on_statics", dtype, static_fused=fused)


def test_a_hull_too_large_for_the_tile_form_takes_np_convex_static():
    """launch_np_static's own rule, restated: the tile form stages the hull's points and up to 64 static boxes (24 reals each) in LDS
    and is taken while that fits 64 KB; 2 400 points in float64 with 64 static boxes do not, so the wavefront-per-body kernel runs"""
    pop = pp.on_statics("ell2400")
    real, sbox_reals, staged_max = 8, 24, 64
    lds = (3 * len(pop.hull.points) + min(len(pop.static_boxes), staged_max) * sbox_reals) * real
    assert len(pop.hull.points) == 2400 and len(pop.static_boxes) == 64
    assert lds == 69888 and lds > 64 * 1024
    _one_tick_parity("on_statics", "float64", shape="ell2400")


# ---------------------------------------------------------------------------------------------------- knobs read once per process
_KNOBS = {"wave_per_body": {"DMX_HULL_WAVE_PER_BODY": "1"}, "filter_0": {"DMX_HULL_FILTER": "0"}, "filter_2": {"DMX_HULL_FILTER": "2"}}
_CHILD_POPS = {"on_statics": ("on_statics", None), "box_hull": ("box_hull", DEFAULT_SHAPE), "on_plane": ("on_plane", None)}


def _child(name, shape, out):
    """in the child process: both precisions against the oracle, the device's states saved for the parent"""
    keep = {}
    for dtype in DTYPES:
        for t, st in enumerate(_one_tick_parity(name, dtype, shape=shape)):
            for f, a in zip(("pos", "quat", "lvel", "avel"), st):
                keep[f"{dtype}_{t}_{f}"] = a
    np.savez(out, **keep)


@pytest.mark.parametrize("knob", sorted(_KNOBS))
@pytest.mark.parametrize("which", sorted(_CHILD_POPS))
def test_knob_in_a_child_process(which, knob, tmp_path):
    """DMX_HULL_WAVE_PER_BODY=1 (np_convex_static whatever the hull's size), DMX_HULL_FILTER=0 (the conservative filters let every
    point through) and =2 (the fused hull path keeps its contacts without confirming the pair on the hull's exact AABB): each equals the oracle, and equals
    the default run bit for bit -- a filter may never change a bit.  One child at a time, each with its own time limit."""
    name, shape = _CHILD_POPS[which]
    here = os.path.dirname(os.path.abspath(__file__))
    out = str(tmp_path / "child.npz")
    code = ("import sys, json; sys.path[:0] = [%r, %r]; import test_gpu_narrowphase_pairs as t; "
            "t._child(*json.loads(%r)); print('CHILD-OK')") % (here, os.path.dirname(here), json.dumps([name, shape, out]))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240, env={**os.environ, **_KNOBS[knob]})
    assert p.returncode == 0 and "CHILD-OK" in p.stdout, (p.stdout[-3000:] + p.stderr[-3000:])
    got = np.load(out)
    for dtype in DTYPES:
        for t, st in enumerate(_one_tick_parity(name, dtype, shape=shape)):
            for f, a in zip(("pos", "quat", "lvel", "avel"), st):
                b = got[f"{dtype}_{t}_{f}"]
                assert np.array_equal(_bits(a), _bits(b)), f"{knob} changed bits of {f} ({which}, {dtype}, tick {t + 1})"
