"""Auto-disable's A/B on the reference's pen through the ODE API (tests/harness/ode_tick_harness.c and, for the legs with the feature on,
tests/harness/autodisable_tick_harness.c): profiles/autodisable_ab.txt is this script's output.

  feature off   the parent commit's build against this one, alternating, medians of --repeats runs: the pen's settled dWorldStep tick
                at 48 and 512 bodies and its QuickStep tick at 400 and 512, both precisions.  A leg is `inside` when this build's median
                lies within the parent's own smallest .. largest run.
  feature on    this build, 512 bodies, settled for 600 ticks under QuickStep as scripts/time_dworldstep.py does, then --on-ticks ticks of
                dWorldStep or QuickStep with dWorldSetAutoDisableFlag(1): ms per tick while a body is awake, ms per tick once none is,
                the tick at which the last one fell asleep, for each threshold pair of --thresholds.

usage: python scripts/time_autodisable.py --parent DIR_WITH_THE_PARENT_BUILDS_LIBRARIES [--repeats 5] [--ticks 40] [--on-ticks 300]"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_ode_compat import _scene_text, pkg  # noqa: E402

PKG = os.path.join(ROOT, "rl-ode-physics_amd")
SETTLE = 600


def build(tmp, name, src, libdir, single):
    exe = os.path.join(tmp, name)
    cmd = ["gcc", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "harness", src), "-o", exe,
           "-L" + libdir, "-lode_mi355_single" if single else "-lode_mi355", "-Wl,-rpath," + os.path.abspath(libdir), "-lm"]
    if single:
        cmd.insert(1, "-DdSINGLE")
    subprocess.run(cmd, check=True)
    return exe


def run(exe, n, stepper, ticks, env=None):
    statics = pkg.scenes.reference_map()
    bodies = pkg.scenes.reference_spawn(n, seed=7, y_range=(1.2, 12.0))
    e = {**os.environ, "HARNESS_TIME_FROM": str(SETTLE + 4), **(env or {})}
    if stepper == "exact":
        e.update(HARNESS_STEPPER="exact", HARNESS_EXACT_AFTER=str(SETTLE))
    else:
        e.update(HARNESS_STEPPER="quick")
    p = subprocess.run([exe], input=_scene_text(1.0 / 120.0, SETTLE + ticks, False, statics, bodies), capture_output=True, text=True, env=e)
    if p.returncode != 0:
        raise RuntimeError(p.stderr[-800:])
    line = re.search(r"harness: (.*)", p.stderr).group(1)
    return {k: float(v) for k, v in re.findall(r"(\w+)=(-?[\d.]+)", line)}, line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--on-ticks", type=int, default=300)
    ap.add_argument("--thresholds", default="0.01,0.2")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp()
    print("== feature off: parent build against this build, ms per tick (dSpaceCollide + step + one pose read), medians of", a.repeats)
    for single in (False, True):
        old = build(tmp, f"old_{int(single)}", "ode_tick_harness.c", a.parent, single)
        new = build(tmp, f"new_{int(single)}", "ode_tick_harness.c", PKG, single)
        for stepper, n in (("exact", 48), ("exact", 512), ("quick", 400), ("quick", 512)):
            po, pn = [], []
            for _ in range(a.repeats):
                po.append(run(old, n, stepper, a.ticks)[0]["ms_per_tick"])
                pn.append(run(new, n, stepper, a.ticks)[0]["ms_per_tick"])
            mo, mn = statistics.median(po), statistics.median(pn)
            verdict = "inside" if min(po) <= mn <= max(po) else ("faster than" if mn < min(po) else "OUTSIDE, slower than")
            print(f"{'f32' if single else 'f64'} {'dWorldStep' if stepper == 'exact' else 'QuickStep '} {n:4d} bodies: parent {mo:.4f} "
                  f"[{min(po):.4f} .. {max(po):.4f}]  this build {mn:.4f} [{min(pn):.4f} .. {max(pn):.4f}]  {verdict} the parent's spread", flush=True)
    print("== feature on: this build, 512 bodies settled", SETTLE, "ticks, then", a.on_ticks, "ticks with auto-disable (idle steps 10)")
    for single in (False, True):
        exe = build(tmp, f"ad_{int(single)}", "autodisable_tick_harness.c", PKG, single)
        for stepper in ("exact", "quick"):
            for thr in a.thresholds.split(","):
                _, line = run(exe, 512, stepper, a.on_ticks, {"HARNESS_AUTODISABLE": f"{thr} {thr} 10"})
                print(f"{'f32' if single else 'f64'} {'dWorldStep' if stepper == 'exact' else 'QuickStep '} thresholds {thr}: {line}", flush=True)
    stacks(a)


def stacks(a):
    """What the pen cannot show when it never sleeps whole: the batch tick (dmxBatchStepJoints, no collision detection) of 128 four-stacks
    of unit boxes -- 512 bodies, 2048 resting contacts (tests/autodisable_scenes.py's, mu 0.5, depth 0), dWorldStep and QuickStep, both
    precisions -- with the feature off, on with thresholds of zero (the rule runs, nothing sleeps: the cost of the update itself),
    and on with thresholds of 0.2, before the stacks sleep (the first 9 ticks) and after (every island left out)."""
    import time
    import numpy as np
    import autodisable_scenes as sc
    B_ = pkg.batch
    print("== 128 four-stacks (512 bodies, 2048 contacts) through dmxBatchStepJoints, ms per tick incl. the wait for the state, medians of", a.repeats)
    pos, lvel, js = [], [], []
    for i in range(128):
        p, v, j = sc.stack(4, 3.0 * (i % 16), 4 * i)
        p[:, 2] += 3.0 * (i // 16); j["pos"][:, 2] += 3.0 * (i // 16)
        pos.append(p); lvel.append(v); js.append(j)
    pos, lvel = np.vstack(pos), np.vstack(lvel)
    jts = np.concatenate(js).astype(B_.CONTACT_JOINT_DTYPE)

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
            rows = {"off": [], "on, thresholds 0": [], "on, awake": [], "on, asleep": []}
            info = ""
            for _ in range(a.repeats):
                for mode in ("off", "zero", "sleep"):
                    w = B_.BatchWorld(512, prec, gravity=(0.0, -9.8, 0.0))
                    w.set_cfm(1e-5); w.set_stepper(stepper)
                    w.upload(B_.POS, pos); w.upload(B_.LVEL, lvel)
                    if mode != "off":
                        w.set_auto_disable(*((0.0, 0.0, 10, 0.0) if mode == "zero" else (0.2, 0.2, 10, 0.0)))
                        w.upload_body_flags(np.full(512, B_.BODY_ALIVE | B_.BODY_AUTODISABLE, np.uint8))
                    timed(w, 3)                                # (first launches, allocations)
                    if mode == "sleep":
                        rows["on, awake"].append(statistics.median(timed(w, 6)))
                        timed(w, 3)
                        st = w.auto_disable_stats()
                        rows["on, asleep"].append(statistics.median(timed(w, 60)))
                        info = f"asleep {st['asleep']} of 512 after 12 ticks, islands left out per tick {w.auto_disable_stats()['islands_skipped']}, path {w.small_tick_stats()}"
                    else:
                        rows["off" if mode == "off" else "on, thresholds 0"].append(statistics.median(timed(w, 60)))
                    w.close()
            name = f"{'f32' if prec == 'float32' else 'f64'} {'dWorldStep' if stepper == B_.STEPPER_EXACT else 'QuickStep '}"
            print(name + ": " + "  ".join(f"{k} {statistics.median(v):.4f} [{min(v):.4f} .. {max(v):.4f}]" for k, v in rows.items()), flush=True)
            print("    " + info, flush=True)


if __name__ == "__main__":
    if "--stacks-only" in sys.argv:
        sys.argv.remove("--stacks-only")
        _ap = argparse.ArgumentParser(); _ap.add_argument("--repeats", type=int, default=5)
        stacks(_ap.parse_args())
        sys.exit(0)
    main()
