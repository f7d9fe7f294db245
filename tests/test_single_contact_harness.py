"""The one-lane island forms' row builder against the general path's, on the host: tests/harness/single_contact_harness.cpp runs
single_contact / single_contact_row (csrc/dmx_island_rows.hpp, what solve_singles_body and solve_singles_lds_body build rows with)
and contact_rows<T> with cb2 = -1 over 4096 seeded one-body contacts in float and in double, and requires J[0..6), c, cfm and the
bounds of every row to carry the same bits.  The program counts what its population covers and fails when a class is missing; the
classes are asserted here once more from its output.  CPU only."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ["direct", "indirect", "launch_surface", "own_surface", "mu_zero", "mu_finite", "mu_inf", "soft_erp_on", "soft_erp_off",
           "soft_cfm_on", "soft_cfm_off", "bounce_off", "bounce_taken", "bounce_below_vel", "layer_zero", "layer_above_depth",
           "maxcorr_inf", "maxcorr_binds", "negative_depth"]


def test_single_contact_builds_the_rows_contact_rows_writes(tmp_path):
    exe = str(tmp_path / "single_contact_harness")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-mfma",
                    "-Wall", "-Wno-unused-function", "-I" + os.path.join(ROOT, "rl-ode-physics_amd", "csrc"),
                    os.path.join(ROOT, "tests", "harness", "single_contact_harness.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, "4096"], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    for prec in ("float", "double"):
        m = re.search(rf"^{prec}: 4096 contacts, (\d+) rows compared, 0 contacts with a difference$", r.stdout, re.M)
        assert m and int(m.group(1)) > 4096, r.stdout
        cov = dict(re.findall(rf"^{prec} coverage (\w+) (\d+)$", r.stdout, re.M))
        assert sorted(cov) == sorted(CLASSES)
        for k in CLASSES:
            assert int(cov[k]) >= 20, (prec, k, cov[k])
