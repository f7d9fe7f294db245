"""The public surface of the single-launch tick of small worlds (include/dmx_batch.h: dmxBatchSetSmallTick,
dmxBatchSmallTickStats): declared in the header, exported by both shipped libraries, bound in _lib.py, and wrapped by
batch.py with a name per counter.  No GPU needed: nothing here creates a batch."""
import os
import re
import subprocess

import pytest

from __graft_entry__ import load_package, ROOT

pkg = load_package()
PKG = os.path.join(ROOT, "rl-ode-physics_amd")
HEADER = os.path.join(ROOT, "include", "dmx_batch.h")
FUNCS = ("dmxBatchSetSmallTick", "dmxBatchSmallTickStats")


def _header():
    return open(HEADER).read()


def _define(name):
    m = re.search(r"^#define\s+%s\s+(\d+)" % name, _header(), re.M)
    assert m, f"{name} is not defined in include/dmx_batch.h"
    return int(m.group(1))


def test_functions_and_constants_are_declared():
    h = _header()
    assert re.search(r"\bint\s+dmxBatchSetSmallTick\s*\(\s*dmxBatchID\s+\w*\s*,\s*int\s+\w+\s*\)\s*;", h)
    assert re.search(r"\bint\s+dmxBatchSmallTickStats\s*\(\s*dmxBatchID\s+\w*\s*,\s*int64_t\s+\w+\[DMX_SMALL_TICK_NSTATS\]\s*\)\s*;", h)
    assert _define("DMX_SMALL_TICK_OFF") == 0
    assert _define("DMX_SMALL_TICK_AUTO") == 1
    # out[0], out[1] and one counter per reason: mode, row order, subset, bodies, islands, SOR rows, LDS fit
    assert _define("DMX_SMALL_TICK_NSTATS") == 9


def test_stat_indices_in_the_header_match_the_python_names():
    h = _header()
    names = pkg.batch.SMALL_TICK_STATS
    assert len(names) == _define("DMX_SMALL_TICK_NSTATS") and len(set(names)) == len(names)
    for k, name in enumerate(names):
        m = re.search(r"\bDMX_SMALL_TICK_STAT_%s\s*=\s*(\d+)" % name.upper(), h)
        assert m and int(m.group(1)) == k, name
    assert names[:2] == ("small", "general")


@pytest.mark.parametrize("libname", ["libode_mi355.so", "libode_mi355_single.so"])
def test_functions_are_exported_by_both_libraries(libname):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, libname)], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for f in FUNCS:
        assert f in exported, f"{libname} does not export {f}"


def test_functions_are_bound_in_lib_py():
    for f in FUNCS:
        assert f in pkg._lib.BATCH_SYMBOLS
    lib = pkg._lib.load()
    import ctypes as C
    assert lib.dmxBatchSetSmallTick.argtypes == [C.c_void_p, C.c_int]
    assert lib.dmxBatchSmallTickStats.argtypes == [C.c_void_p, C.c_void_p]
    # a null batch is an argument error, not a crash (DMX_EINVAL), with or without a device
    assert lib.dmxBatchSetSmallTick(None, pkg.batch.SMALL_TICK_AUTO) < 0
    assert lib.dmxBatchSmallTickStats(None, None) < 0


def test_batch_py_exposes_the_mode_and_the_counters():
    B = pkg.batch
    assert (B.SMALL_TICK_OFF, B.SMALL_TICK_AUTO) == (0, 1)
    assert callable(B.BatchWorld.set_small_tick) and callable(B.BatchWorld.small_tick_stats)
    assert B.SMALL_TICK_STATS == ("small", "general", "mode", "row_order", "subset", "bodies", "islands", "sor_rows", "lds_fit")
