"""Boundary row (b): the reference's own src/main.c links against libode_mi355*.so as it stands.  The d* symbols an object
file of main.c leaves undefined -- compiled against this repository's include/ode/ode.h and include/ode/common.h, in
both ODE precisions, with raylib / raymath / rlgl / raygui / ENet from the test-only prototype stubs under tests/stubs --
are recorded in tests/golden/main_c_ode_names.json (names only); each must be exported by the library of its precision.
The argument types of main.c's ODE calls are checked by compiling tests/harness/ode_tick_harness.c, which makes the same
calls (tests/test_ode_compat.py); the dContact layout main.c indexes is checked below."""
import json
import os
import subprocess

import pytest

from __graft_entry__ import ROOT, load_package

NAMES = json.load(open(os.path.join(ROOT, "tests", "golden", "main_c_ode_names.json")))


@pytest.mark.parametrize("precision", ["dDOUBLE", "dSINGLE"])
def test_main_c_undefined_symbols_are_exported(precision):
    wanted = NAMES["undefined_symbols"][precision]
    assert len(wanted) >= 30, wanted                       # the 32 ODE entry points main.c calls
    assert set(wanted) <= set(NAMES["called"])
    pkg = load_package()
    lib = pkg._lib.LIB_PATH if precision == "dDOUBLE" else pkg._lib.LIB_PATH.replace("libode_mi355.so", "libode_mi355_single.so")
    exported = set(subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout.split())
    missing = [s for s in wanted if s not in exported]
    assert not missing, missing


def test_dcontact_layout_as_main_c_indexes_it(tmp_path):
    """NearCallback (main.c:676-691) declares dContact contacts[MAX_CONTACTS], hands &contacts[0].geom to dCollide with a
    byte stride of sizeof(dContact), and reads .geom.depth / writes .surface.{mode,mu,bounce,bounce_vel}: the offsets the
    library's dCollide writes at must be the ones a C client compiled against the header computes."""
    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "ode/ode.h"\n'
        'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(dContact), offsetof(dContact, geom), offsetof(dContactGeom, pos),\n'
        '  offsetof(dContactGeom, normal), offsetof(dContactGeom, depth), offsetof(dContactGeom, g1), sizeof(dReal)); return 0; }\n')
    for precision, rsize in (("dDOUBLE", 8), ("dSINGLE", 4)):
        exe = str(tmp_path / ("layout_" + precision))
        subprocess.run(["gcc", "-std=gnu99", "-D" + precision, "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
        sz, o_geom, o_pos, o_normal, o_depth, o_g1, real = map(int, subprocess.run([exe], capture_output=True, text=True).stdout.split())
        assert real == rsize
        assert o_pos == 0 and o_normal == 4 * rsize and o_depth == 8 * rsize          # dVector3 = dReal[4]
        assert o_g1 >= o_depth + rsize and o_geom > 0 and sz >= o_geom + o_g1 + 16
