"""The C face of the angular motors: tests/harness/amotor_abi_check.c compiles (C99, -pedantic -Werror) against include/dmx_batch.h and
include/ode/ode.h and links against both libraries -- every new symbol in both ODE precisions; dmxAMotor's layout is _lib.dmxAMotor's
and batch.AMOTOR_DTYPE's; dmxJoint, dmxHingeLimot and dmxContactJoint keep their sizes; the enum values are ODE's; the header, the
bindings' symbol list and the libraries' exports agree.  CPU only: no device is touched."""
import ctypes as C
import os
import re
import subprocess

import pytest

import amotor_dense as am
from __graft_entry__ import load_package, ROOT

pkg = load_package()
PKG = os.path.join(ROOT, "rl-ode-physics_amd")
WIDTHS = [("dDOUBLE", "ode_mi355"), ("dSINGLE", "ode_mi355_single")]
BATCH_NAMES = ["dmxBatchSetAMotors", "dmxBatchAMotorFromWorld", "dmxBatchAMotorAngles"]
ODE_NAMES = ["dJointCreateAMotor", "dJointSetAMotorMode", "dJointGetAMotorMode", "dJointSetAMotorNumAxes", "dJointGetAMotorNumAxes",
             "dJointSetAMotorAxis", "dJointGetAMotorAxis", "dJointGetAMotorAxisRel", "dJointSetAMotorAngle", "dJointGetAMotorAngle",
             "dJointGetAMotorAngleRate", "dJointSetAMotorParam", "dJointGetAMotorParam", "dJointAddAMotorTorques"]
OFFSETS = [0, 4, 8, 20, 24, 96, 120, 144, 168, 192, 216, 240]


@pytest.mark.parametrize("width,lib", WIDTHS)
def test_layout_enums_and_entry_points(width, lib, tmp_path):
    exe = str(tmp_path / "amotor_abi_check")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-D" + width, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "harness", "amotor_abi_check.c"), "-o", exe, "-L" + PKG, "-l" + lib, "-Wl,-rpath," + PKG, "-lm"],
                   check=True)
    p = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120)
    got = {k: int(v) for k, v in (line.split() for line in p.stdout.splitlines())}
    st, dt = pkg._lib.dmxAMotor, pkg.batch.AMOTOR_DTYPE
    names = [f[0] for f in st._fields_]
    assert names == list(dt.names) == list(am.AMOTOR_DTYPE.names)
    assert got["sizeof"] == C.sizeof(st) == dt.itemsize == am.AMOTOR_DTYPE.itemsize == 264
    assert [got[f] for f in names] == [getattr(st, f).offset for f in names] == [dt.fields[f][1] for f in names] == OFFSETS
    assert [am.AMOTOR_DTYPE.fields[f][1] for f in names] == OFFSETS
    # the layouts this feature leaves as they are
    assert (got["joint"], got["limot"], got["contact"]) == (pkg.batch.JOINT_DTYPE.itemsize, pkg.batch.HINGE_LIMOT_DTYPE.itemsize,
                                                            pkg.batch.CONTACT_JOINT_DTYPE.itemsize) == (112, 64, 112)


def test_header_bindings_and_exports_agree():
    header = open(os.path.join(ROOT, "include", "dmx_batch.h")).read()
    ode = open(os.path.join(ROOT, "include", "ode", "ode.h")).read()
    B = pkg.batch
    assert int(re.search(r"DMX_JOINT_AMOTOR = (\d+)", header).group(1)) == B.JOINT_AMOTOR == am.AMOTOR == 5
    assert (int(re.search(r"DMX_AMOTOR_USER = (\d+)", header).group(1)), int(re.search(r"DMX_AMOTOR_EULER = (\d+)", header).group(1))) \
        == (B.AMOTOR_USER, B.AMOTOR_EULER) == (am.USER, am.EULER) == (0, 1)
    assert re.search(r"dJointTypeAMotor = 9\b", ode) and re.search(r"dAMotorUser = 0, dAMotorEuler = 1\b", ode)
    assert re.search(r"dParamGroup = 0x100\b", ode) and re.search(r"dParamLoStop2 = 0x100\b", ode) and re.search(r"dParamLoStop3 = 0x200\b", ode)
    for name in BATCH_NAMES:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in pkg._lib.BATCH_SYMBOLS
    for name in ODE_NAMES:
        assert re.search(r"\b%s\(" % name, ode), name
    for _, lib in WIDTHS:
        so = C.CDLL(os.path.join(PKG, "lib" + lib + ".so"), mode=os.RTLD_LOCAL)
        for name in BATCH_NAMES + ODE_NAMES:
            assert hasattr(so, name), (lib, name)
