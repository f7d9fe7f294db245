"""The device's float32 contacts against FLOAT64, without the float32 oracle in between.

tests/test_gpu_narrowphase_pairs.py holds the device in float32 to the float32 oracle bit for bit, and tests/test_collider_geometry.py
holds that oracle within a band of float64 geometry: a chain that leans on the float32 oracle staying independent of csrc/.  Here each
population of tests/pair_population.py, near the origin and translated by (4 096, 0, -2 560) m, is loaded into a float32 `BatchWorld`
and -- the same float32 VALUES -- into a float64 one, both at cfm 1e-5, and stepped one tick:

  * the float64 device state equals the float64 oracle's bit for bit, the tick's contact count too;
  * on the COMPARABLE cells -- decided by the two oracles' joints alone (pair_population.precision_tick: the same contacts in the same
    slots within the band), never by the device -- the float32 device state is within the tolerance of the float64 device state.  The
    tolerance is 4 x what the float32 ORACLE was measured to deviate from the float64 one (pair_population.TICK_MEASURED, asserted on
    the CPU by tests/test_pair_population.py): no number here was taken from the device;
  * the float32 device's contact count is the float32 oracle's, and differs from the float64 device's by exactly what the cells that
    are not comparable account for.

Also over `set_static_path(fused=True / False)` for `on_statics` and `on_plane` (np_static, np_convex_static_tile against the exact
tick's static entries) and, in a child process each since the knob is read once, with the hull filters off and on (DMX_HULL_FILTER =
0, 2): a filter slack below float32's real error would drop a contact that float64 keeps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pair_population as pp
from pair_population import pkg

pytestmark = pytest.mark.gpu
PLACES = [False, True]
PLACE_IDS = ["near", "far"]
FIELDS = ("lvel", "avel", "pos", "quat")


def _device_tick(sc, dtype, static_fused=None):
    """one tick of the scene on the device at cfm 1e-5 -> (state, contact count)"""
    w = pkg.BatchWorld(sc.n, dtype=dtype)
    try:
        w.set_cfm(pp.CFM_BOTH)
        if static_fused is not None:
            w.set_static_path(fused=static_fused)
        w.load_scene(sc)
        w.step(np.dtype(dtype).type(pp.H), 1)
        w.synchronize()
        state = w.state()
        assert w.collision_stats()["unsupported_pairs"] == 0
        return state, w.last_contact_count()
    finally:
        w.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _check(key, far, static_fused=None):
    key = tuple(key)
    r = pp.precision_tick(key, far)
    pop = r["pop"]
    tag = f"{pp.pop_id(key)} {'far' if far else 'near'} fused={static_fused}"
    s64, n64 = _device_tick(r["sc64"], "float64", static_fused)
    s32, n32 = _device_tick(r["sc32"], "float32", static_fused)
    # the float64 device is the float64 oracle
    for name, a, b in zip(("pos", "quat", "lvel", "avel"), s64, r["state64"]):
        bad = np.flatnonzero(np.any(_bits(a) != _bits(b), axis=1))
        assert len(bad) == 0, f"{tag}: float64 device differs from the float64 oracle in {name} of {len(bad)} bodies, cells {sorted({int(pop.cell[b]) for b in bad})[:10]}"
    assert n64 == r["total64"], f"{tag}: {n64} contacts on the float64 device, {r['total64']} in the float64 oracle"
    # the float32 device against the float64 device, on the cells the two oracles call comparable
    dev = pp.deviation(s32, s64, r["body_ok"], r["units"])
    tol = pp.tick_tolerance(key[0], far)
    print(f"DEVICE-PRECISION {tag}: comparable {int(r['comparable'].sum())} of {r['cells']} cells; float32 device - float64 device, "
          "lvel / avel / pos / quat " + " / ".join(f"{v:.3g}" for v in dev) + "; float32 oracle - float64 oracle "
          + " / ".join(f"{v:.3g}" for v in r["dev"]) + "; tolerance " + " / ".join(f"{v:.3g}" for v in tol))
    for i, (name, got, t) in enumerate(zip(FIELDS, dev, tol)):
        if got > t:
            a, b = np.asarray(s32[(2, 3, 0, 1)[i]], float), np.asarray(s64[(2, 3, 0, 1)[i]], float)
            worst = np.where(r["body_ok"], np.max(np.abs(a - b), axis=1), 0.0)
            cells = sorted({int(pop.cell[b]) for b in np.argsort(-worst)[:4]})
            raise AssertionError(f"{tag}: {name} of the float32 device is {got:.3g} units from the float64 device (tolerance {t:.3g})\n"
                                 + pop.describe(cells, r["sc32"]))
    # contact counts: the float32 oracle's; against float64 the difference is what the not comparable cells account for
    assert n32 == r["total32"], f"{tag}: {n32} contacts on the float32 device, {r['total32']} in the float32 oracle"
    odd = ~r["comparable"]
    assert np.array_equal(r["contacts32"][~odd], r["contacts64"][~odd])
    assert n32 - n64 == int(r["contacts32"][odd].sum() - r["contacts64"][odd].sum())
    return dev


@pytest.mark.parametrize("far", PLACES, ids=PLACE_IDS)
@pytest.mark.parametrize("key", pp.ALL, ids=pp.pop_id)
def test_population(key, far):
    _check(key, far)


@pytest.mark.parametrize("far", PLACES, ids=PLACE_IDS)
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", ["on_statics", "on_plane"])
def test_static_paths(name, fused, far):
    """np_static / np_convex_static_tile / np_convex_plane (fused) and the exact tick's static entries, each against float64"""
    _check((name, None), far, static_fused=fused)


# ---------------------------------------------------------------------------------------------------- the hull filters, read once per process
_KNOBS = {"filter_0": {"DMX_HULL_FILTER": "0"}, "filter_2": {"DMX_HULL_FILTER": "2"}}
_CHILD_POPS = {"on_statics": ("on_statics", None), "box_hull": ("box_hull", "ell65"), "on_plane": ("on_plane", None)}


def _child(key):
    for far in PLACES:
        _check(key, far)


@pytest.mark.parametrize("knob", sorted(_KNOBS))
@pytest.mark.parametrize("which", sorted(_CHILD_POPS))
def test_hull_filters_in_a_child_process(which, knob):
    """DMX_HULL_FILTER=0 (every point goes through) and =2 (the fused hull path keeps its contacts without confirming the pair on the
    hull's exact AABB): float32 stays within the same tolerance of float64 either way, near and far.  One child at a time."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys, json; sys.path[:0] = [%r, %r]; import test_gpu_precision_pairs as t; "
            "t._child(json.loads(%r)); print('CHILD-OK')") % (here, os.path.dirname(here), json.dumps(list(_CHILD_POPS[which])))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240, env={**os.environ, **_KNOBS[knob]})
    assert p.returncode == 0 and "CHILD-OK" in p.stdout, (p.stdout[-3000:] + p.stderr[-3000:])
    print(p.stdout[-2000:])
