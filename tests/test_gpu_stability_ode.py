"""The ODE face of damping, the maximum angular speed and the contact correction scalars (include/ode/ode.h: dWorldSetDamping & co.,
the dBodySet... forms, dWorldSetContactSurfaceLayer, dWorldSetContactMaxCorrectingVel), through tests/harness/stability_tick_harness.c:
a C program against the ODE header, built for both widths of dReal, whose twin drives the same scene through include/dmx_batch.h.

The two print every body's state after every tick; the outputs are compared as text -- bit for bit.  The ODE run also checks, in C,
that every getter returns what was set, that a body created after dWorldSetDamping inherits the world's values while an earlier one
keeps its own, and that values out of range are ignored (a line "FAIL ..." otherwise).  A run that touches no knob must differ:
the knobs act.  A second case makes 520 more bodies after three ticks, more than the world's first batch holds: the world
moves to a larger batch and must carry the table and the two scalars over (the twin has that capacity from the start)."""
import os
import subprocess

import numpy as np
import pytest

from __graft_entry__ import ROOT

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "rl-ode-physics_amd")
WIDTHS = [("dDOUBLE", "ode_mi355"), ("dSINGLE", "ode_mi355_single")]
_BUILT = {}


def build(width, lib, tmp_path_factory):
    if width not in _BUILT:
        exe = str(tmp_path_factory.mktemp("build") / "stability_tick_harness")
        subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-D" + width, "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "harness", "stability_tick_harness.c"), "-o", exe, "-L" + PKG, "-l" + lib, "-Wl,-rpath," + PKG,
                        "-lm"], check=True)
        _BUILT[width] = exe
    return _BUILT[width]


def run(exe, *args):
    p = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "FAIL" not in p.stdout, p.stdout + p.stderr
    return p.stdout, p.stderr


@pytest.mark.parametrize("stepper", ["step", "quick"])
@pytest.mark.parametrize("width,lib", WIDTHS)
def test_ode_face_against_its_batch_twin(width, lib, stepper, tmp_path_factory):
    exe = build(width, lib, tmp_path_factory)
    ode, err = run(exe, "ode", stepper)
    batch, _ = run(exe, "batch", stepper)
    assert ode == batch, "the ODE face and the batch API disagree"
    assert err.count("out of range; ignored") == 7                       # the seven refused setters said so
    plain, err = run(exe, "ode", stepper, "plain")
    plain_batch, _ = run(exe, "batch", stepper, "plain")
    assert plain == plain_batch and err == ""
    a = np.array([[float(x) for x in line.split()] for line in ode.splitlines()]).reshape(6, 6, 13)        # tick, body, field
    p = np.array([[float(x) for x in line.split()] for line in plain.splitlines()]).reshape(6, 6, 13)
    assert np.all(np.isfinite(a)) and not np.array_equal(a[0, :5], p[0, :5])
    assert np.array_equal(a[:, 5, 7:13], p[:, 5, 7:13]) and np.array_equal(a[0, 5], p[0, 5])                # the kinematic body: untouched by any knob
    assert abs(np.linalg.norm(a[0, 4, 10:13]) - 0.75) <= 1e-6 and np.linalg.norm(p[0, 4, 10:13]) > 2.0      # the free spinner ends on its own cap
    assert abs(np.linalg.norm(a[0, 1, 10:13]) - 1.5) <= 1e-6                                                 # ... body 1 on the world's


@pytest.mark.parametrize("stepper", ["step", "quick"])
@pytest.mark.parametrize("width,lib", WIDTHS)
def test_a_world_that_outgrows_its_batch_carries_the_knobs_over(width, lib, stepper, tmp_path_factory):
    exe = build(width, lib, tmp_path_factory)
    ode, _ = run(exe, "ode", stepper, "grow")
    batch, _ = run(exe, "batch", stepper, "grow")
    assert ode == batch, "the ODE face and the batch API disagree after the world has grown"
    small, _ = run(exe, "ode", stepper)
    rows = [[float(x) for x in line.split()] for line in ode.splitlines()]
    assert len(rows) == 3 * 6 + 3 * 8                                    # two of the new bodies are printed from tick 3 on
    assert ode.splitlines()[:18] == small.splitlines()[:18]
    # the knobs are still in force after the move: the resting bodies' ticks are those of the world that never grew (their islands are
    # their own); the last new body, made spinning at 3 rad/s about y, is damped by 12.5 % a tick and capped at the world's 1.5 rad/s
    # in its first tick, and falls more slowly than g h per tick once it is past the 0.25 m/s threshold
    after = rows[18:]
    assert [r for k, r in enumerate(after) if k % 8 < 6] == [[float(x) for x in line.split()] for line in small.splitlines()[18:]]
    last = np.array(after[7::8])
    assert np.allclose(np.linalg.norm(last[:, 10:13], axis=1), 1.5 * 0.875 ** np.arange(3), rtol=1e-6)
    assert -3 * 9.8 / 60.0 + 0.01 < last[-1, 8] < -0.3
