"""Damping / angular speed cap / contact correction: what the knobs cost, and what they do to the pen.

  knobs at defaults   the parent commit's build against this one, alternating, medians of --repeats runs; a leg is `inside` when this
                      build's median lies within the parent's own smallest .. largest run.
                      (a) through the ODE API (tests/harness/ode_tick_harness.c): the pen's settled dWorldStep tick at 48 and 512
                          bodies and its QuickStep tick at 400 and 512, both precisions -- scripts/time_autodisable.py's legs;
                      (b) the 24 cart-poles of scripts/time_sliders.py (48 bodies, the single-launch tick), both steppers and
                          precisions, each build in a process of its own that imports its own package;
                      (c) 12 four-stacks (48 bodies) with auto-disable on at thresholds of zero, without and with feedback: the AD
                          instantiations of small_world_tick, the same way.
  knobs on            this build, dmxBatchStepJoints: four-stacks of unit boxes (tests/autodisable_scenes.py's), 128 stacks (512 bodies)
                      on the general path and 12 stacks (48 bodies) on the single-launch tick, and the 24 cart-poles: no knob touched /
                      damping 1 % on every body (the damping pass runs) / damping and a cap of 100 rad/s (finish_body loads the table too).
  the pen             tests/harness/stability_pen_harness.c: the reference's 512-body pen settled for 600 ticks under QuickStep, then
                      --on-ticks ticks with auto-disable at ODE's default thresholds (0.01, 0.01, 10 steps): as it is, with
                      dWorldSetDamping(0.01, 0.01), with a surface layer of 1 mm, and with both.

usage: python scripts/time_stability.py --parent ROOT_OF_THE_PARENT_COMMITS_BUILT_CHECKOUT [--repeats 5] [--ticks 40] [--on-ticks 300]
                                        [--only defaults,cartpoles,adstacks,on,pen]"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import time_autodisable as ta  # noqa: E402  (puts the repository and tests/ on the path)
import numpy as np  # noqa: E402
import autodisable_scenes as sc  # noqa: E402

pkg = ta.pkg
B_ = pkg.batch

# one process per build: argv = root of the checkout, mode (untouched / damping / cap), ticks.  Prints four numbers: ms per tick of the
# 24 cart-poles for quick f32, quick f64, exact f32, exact f64 (time_sliders.run's loop with the knobs set after the joints)
CARTPOLES = r"""
import os, sys, time
root, mode, ticks = sys.argv[1], sys.argv[2], int(sys.argv[3])
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "scripts")); sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np
import time_sliders as ts
B_ = ts.B_
(_, B, art, lim) = list(ts.scenes())[1]
out = []
for stepper in ("quick", "exact"):
    for prec in ("float32", "float64"):
        w = B_.BatchWorld(B.n, prec)
        w.set_erp(0.2); w.set_cfm(1e-5)
        w.set_stepper(B_.STEPPER_EXACT if stepper == "exact" else B_.STEPPER_QUICK)
        w.upload(B_.POS, B.pos); w.upload(B_.QUAT_RAW, B.quat); w.upload(B_.LVEL, B.lvel); w.upload(B_.AVEL, B.avel)
        w.upload(B_.MASS, B.mass); w.upload(B_.INERTIA, B.inertia)
        w.upload_body_flags(B.flags)
        w.set_joints(ts.to_c(art, B_.JOINT_DTYPE))
        w.set_hinge_limots(ts.to_c(lim, B_.HINGE_LIMOT_DTYPE))
        if mode != "untouched":
            w.set_damping(0.01, 0.01, 0.0, 0.0)
        if mode == "cap":
            w.set_max_angular_speed(100.0)
        none = np.zeros(0, B_.CONTACT_JOINT_DTYPE)
        for _ in range(20):
            w.step_joints(ts.H, none)
        w.synchronize()
        t0 = time.perf_counter()
        for _ in range(ticks):
            w.step_joints(ts.H, none)
            w.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / ticks)
        assert w.small_tick_stats()["small"] > 0
        w.close()
print(" ".join(f"{x:.5f}" for x in out))
"""
# the same for 12 four-stacks (48 bodies, 192 contacts) with auto-disable on at thresholds of zero (the rule runs, nothing sleeps): the AD
# instantiations of small_world_tick, without and with feedback.  Prints eight numbers: (quick f32, quick f64, exact f32, exact f64) x (feedback off, on)
AD_STACKS = r"""
import os, sys, time
root, ticks = sys.argv[1], int(sys.argv[3])
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "scripts")); sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np
import autodisable_scenes as sc
from __graft_entry__ import load_package
B_ = load_package().batch
pos, lvel, js = [], [], []
for i in range(12):
    p, v, j = sc.stack(4, 3.0 * i, 4 * i)
    pos.append(p); lvel.append(v); js.append(j)
pos, lvel = np.vstack(pos), np.vstack(lvel)
jts = np.concatenate(js).astype(B_.CONTACT_JOINT_DTYPE)
out = []
for fb in (False, True):
    for stepper in (B_.STEPPER_QUICK, B_.STEPPER_EXACT):
        for prec in ("float32", "float64"):
            w = B_.BatchWorld(len(pos), prec, gravity=(0.0, -9.8, 0.0))
            w.set_cfm(1e-5); w.set_stepper(stepper)
            w.upload(B_.POS, pos); w.upload(B_.LVEL, lvel)
            w.set_auto_disable(0.0, 0.0, 10, 0.0)
            w.upload_body_flags(np.full(len(pos), B_.BODY_ALIVE | B_.BODY_AUTODISABLE, np.uint8))
            w.set_feedback(fb)
            for _ in range(20):
                w.step_joints(sc.H, jts)
            w.synchronize()
            t0 = time.perf_counter()
            for _ in range(ticks):
                w.step_joints(sc.H, jts)
                w.synchronize()
            out.append(1e3 * (time.perf_counter() - t0) / ticks)
            assert w.small_tick_stats()["small"] > 0 and w.auto_disable_stats()["asleep"] == 0
            w.close()
print(" ".join(f"{x:.5f}" for x in out))
"""
LEGS = ("QuickStep  f32", "QuickStep  f64", "dWorldStep f32", "dWorldStep f64")


def cartpoles_run(root, mode, ticks, code=CARTPOLES, count=4):
    p = subprocess.run([sys.executable, "-c", code, root, mode, str(ticks)], capture_output=True, text=True, cwd=root)
    if p.returncode != 0:
        raise RuntimeError(p.stderr[-800:])
    return [float(x) for x in p.stdout.split()[-count:]]


def verdict(po, mn):
    return "inside" if min(po) <= mn <= max(po) else ("faster than" if mn < min(po) else "OUTSIDE, slower than")


def defaults(a):
    tmp = tempfile.mkdtemp()
    print("== knobs at defaults (a): parent build against this build, the pen through the ODE API, ms per tick (dSpaceCollide + step + one pose read), medians of", a.repeats)
    parent_lib = os.path.join(a.parent, "rl-ode-physics_amd")
    for single in (False, True):
        old = ta.build(tmp, f"old_{int(single)}", "ode_tick_harness.c", parent_lib, single)
        new = ta.build(tmp, f"new_{int(single)}", "ode_tick_harness.c", ta.PKG, single)
        for stepper, n in (("exact", 48), ("exact", 512), ("quick", 400), ("quick", 512)):
            po, pn = [], []
            for _ in range(a.repeats):
                po.append(ta.run(old, n, stepper, a.ticks)[0]["ms_per_tick"])
                pn.append(ta.run(new, n, stepper, a.ticks)[0]["ms_per_tick"])
            mo, mn = statistics.median(po), statistics.median(pn)
            print(f"{'f32' if single else 'f64'} {'dWorldStep' if stepper == 'exact' else 'QuickStep '} {n:4d} bodies: parent {mo:.4f} "
                  f"[{min(po):.4f} .. {max(po):.4f}]  this build {mn:.4f} [{min(pn):.4f} .. {max(pn):.4f}]  {verdict(po, mn)} the parent's spread", flush=True)


def cartpoles(a):
    print("== knobs at defaults (b) and knobs on: 24 cart-poles (48 bodies, single-launch tick), ms per tick of 200, medians of", a.repeats)
    rows = {"parent": [], "untouched": [], "damping": [], "cap": []}
    for _ in range(a.repeats):
        rows["parent"].append(cartpoles_run(os.path.abspath(a.parent), "untouched", 200))
        for mode in ("untouched", "damping", "cap"):
            rows[mode].append(cartpoles_run(ROOT, mode, 200))
    for k, leg in enumerate(LEGS):
        col = {m: [r[k] for r in v] for m, v in rows.items()}
        po, mn = col["parent"], statistics.median(col["untouched"])
        print(f"{leg}: parent {statistics.median(po):.4f} [{min(po):.4f} .. {max(po):.4f}]  this build untouched {mn:.4f} [{min(col['untouched']):.4f} .. "
              f"{max(col['untouched']):.4f}] {verdict(po, mn)} the parent's spread;  damping {statistics.median(col['damping']):.4f} "
              f"[{min(col['damping']):.4f} .. {max(col['damping']):.4f}]  damping + cap {statistics.median(col['cap']):.4f} [{min(col['cap']):.4f} .. {max(col['cap']):.4f}]", flush=True)


def ad_stacks(a):
    print("== knobs at defaults (c): 12 four-stacks (48 bodies) with auto-disable on, thresholds 0 -- small_world_tick's AD instantiations, "
          "without and with feedback; ms per tick of 200, medians of", a.repeats)
    old, new = [], []
    for _ in range(a.repeats):
        old.append(cartpoles_run(os.path.abspath(a.parent), "-", 200, AD_STACKS, 8))
        new.append(cartpoles_run(ROOT, "-", 200, AD_STACKS, 8))
    for k in range(8):
        po, pn = [r[k] for r in old], [r[k] for r in new]
        mn = statistics.median(pn)
        print(f"{LEGS[k % 4]} feedback {'on ' if k >= 4 else 'off'}: parent {statistics.median(po):.4f} [{min(po):.4f} .. {max(po):.4f}]  this build {mn:.4f} "
              f"[{min(pn):.4f} .. {max(pn):.4f}]  {verdict(po, mn)} the parent's spread", flush=True)


def knobs_on(a):
    print("== knobs on: four-stacks through dmxBatchStepJoints, ms per tick incl. the wait for one pose, medians of", a.repeats, "runs of 60 ticks")
    for n_stacks, small in ((128, B_.SMALL_TICK_OFF), (12, B_.SMALL_TICK_AUTO)):
        pos, lvel, js = [], [], []
        for i in range(n_stacks):
            p, v, j = sc.stack(4, 3.0 * (i % 16), 4 * i)
            p[:, 2] += 3.0 * (i // 16); j["pos"][:, 2] += 3.0 * (i // 16)
            pos.append(p); lvel.append(v); js.append(j)
        pos, lvel = np.vstack(pos), np.vstack(lvel)
        jts = np.concatenate(js).astype(B_.CONTACT_JOINT_DTYPE)
        n = len(pos)

        def timed(w, ticks):
            out = []
            for _ in range(ticks):
                t0 = time.perf_counter()
                w.step_joints(sc.H, jts)
                w.download(B_.POS, count=1)
                out.append((time.perf_counter() - t0) * 1e3)
            return out

        for prec in ("float64", "float32"):
            for stepper in (B_.STEPPER_EXACT, B_.STEPPER_QUICK):
                rows = {"untouched": [], "damping": [], "damping + cap": []}
                path = None
                for _ in range(a.repeats):
                    for mode in rows:
                        w = B_.BatchWorld(n, prec, gravity=(0.0, -9.8, 0.0))
                        w.set_cfm(1e-5); w.set_stepper(stepper); w.set_small_tick(small)
                        w.upload(B_.POS, pos); w.upload(B_.LVEL, lvel)
                        if mode != "untouched":
                            w.set_damping(0.01, 0.01, 0.0, 0.0)
                        if mode == "damping + cap":
                            w.set_max_angular_speed(100.0)
                        timed(w, 3)                                # (first launches, allocations)
                        rows[mode].append(statistics.median(timed(w, 60)))
                        path = w.small_tick_stats()
                        w.close()
                name = f"{n:3d} bodies {'f32' if prec == 'float32' else 'f64'} {'dWorldStep' if stepper == B_.STEPPER_EXACT else 'QuickStep '}"
                print(name + ": " + "  ".join(f"{k} {statistics.median(v):.4f} [{min(v):.4f} .. {max(v):.4f}]" for k, v in rows.items()) +
                      f"  (small ticks {path['small']}, general {path['general']})", flush=True)


def pen(a):
    print("== the pen: 512 bodies settled", ta.SETTLE, "ticks, then", a.on_ticks, "ticks with auto-disable at ODE's defaults (0.01, 0.01, 10 steps)")
    tmp = tempfile.mkdtemp()
    settings = (("as it is", {}), ("damping 0.01 0.01", {"HARNESS_DAMPING": "0.01 0.01"}), ("surface layer 1 mm", {"HARNESS_SURFACE_LAYER": "0.001"}),
                ("damping and layer", {"HARNESS_DAMPING": "0.01 0.01", "HARNESS_SURFACE_LAYER": "0.001"}))
    for single in (False, True):
        exe = ta.build(tmp, f"pen_{int(single)}", "stability_pen_harness.c", ta.PKG, single)
        for stepper in ("exact", "quick"):
            for name, env in settings:
                _, line = ta.run(exe, 512, stepper, a.on_ticks, {"HARNESS_AUTODISABLE": "0.01 0.01 10", **env})
                print(f"{'f32' if single else 'f64'} {'dWorldStep' if stepper == 'exact' else 'QuickStep '} {name:20s}: {line}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--on-ticks", type=int, default=300)
    ap.add_argument("--only", default="defaults,cartpoles,adstacks,on,pen")
    a = ap.parse_args()
    for name, f in (("defaults", defaults), ("cartpoles", cartpoles), ("adstacks", ad_stacks), ("on", knobs_on), ("pen", pen)):
        if name in a.only.split(","):
            f(a)
