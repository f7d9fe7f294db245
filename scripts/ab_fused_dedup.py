"""A/B of the one-body ticks (the fused ticks of csrc/dmx_step_fused.hpp and csrc/dmx_kernels.hip, the one-lane island forms of
csrc/dmx_islands_dev.hpp) when their duplicated statements become shared functions, against a built checkout of the parent commit:
both builds in the same visit to the GPU, the builds alternating, medians of --repeats runs per leg.  The rule is scripts/ab_lean_kernel.sh's: no leg may be slower than the parent by more than the parent's own spread (max - min)
on that leg.  No gain is claimed.  Every GPU step is a child process under a time limit of its own; the script stops at the first
that fails.  Every run is appended to --out as it is made; the medians, spreads and one verdict line per leg follow at the end.

  python scripts/ab_fused_dedup.py --parent BUILT_CHECKOUT_OF_THE_PARENT [--out bench_out/fused_dedup_ab.txt] [--repeats 5]
                                   [--only dump,floor,singles,small,bench,trace] [--budget SECONDS]
--budget: a visit to the GPU may be limited in time -- no repetition of a leg is begun once the leg has run that many seconds.  Runs
are appended to --out, and the summary is made from every RUN line in it: legs may be measured over several visits (--only) with
the same two builds, and the summary says how many runs each leg got (n).

legs, and the changed kernels each one times:
  dump     bench.py --dump-outputs of both builds in f32 and f64, compared with cmp (bits, not time)
  floor    scripts/time_floor.py in f32 and f64: boxes on a floor box (step_contacts NC = 4: two-launch form at 102 400 bodies, one
           launch at 10 000), teapot hulls on the plane (step_plane NC = 8) and on a floor box (step_contacts NC = 8)
  singles  dmxBatchStepJoints on 4096 one-body islands with contacts handed in, general path: unit boxes with four contacts each
           (solve_singles) and with eight, a hull's count (solve_singles_lds), f32 and f64
  small    the 48-body single-launch legs of scripts/time_stability.py (24 cart-poles; 12 four-stacks with auto-disable on):
           small_world_tick
  bench    bench.py --full --no-cpu-baseline (--steps 200 --warmup 20 --hbm-side 1024: the headline and hbm_resident are not legs
           here): configs[2] (step_plane<float, ., 2, 4>), configs[4] (step_contacts NC = 8, one-launch form), configs[0], both pens
  trace    one `rocprofv3 --kernel-trace --stats` pass per build, each in a run of its own, over the `singles` scenes and a short
           run of each `floor` scene kind: per-kernel averages of step_plane, step_contacts, solve_singles, solve_singles_lds"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
H = 1.0 / 60.0


# ---------------------------------------------------------------------------------------------------------- child legs
def child_singles(root, ticks):
    """prints `LEG <name> <ms per tick>` for the build of the checkout at root"""
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    from __graft_entry__ import load_package
    import autodisable_scenes as sc
    B_ = load_package().batch
    n = 4096
    for contacts in (4, 8):
        pos, lvel, js = [], [], []
        for i in range(n):
            x, z = 3.0 * (i % 64), 3.0 * (i // 64)
            p, v, j = sc.stack(1, x, i)
            if contacts == 8:           # four more at the edges' midpoints: a hull's eight contacts with the floor
                e = j.copy()
                e["pos"] = [(x + dx, 0.0, dz) for dx, dz in ((0.0, -0.5), (0.5, 0.0), (0.0, 0.5), (-0.5, 0.0))]
                j = np.concatenate([j, e])
            p[:, 2] += z; j["pos"][:, 2] += z
            pos.append(p); lvel.append(v); js.append(j)
        pos, lvel = np.vstack(pos), np.vstack(lvel)
        jts = np.concatenate(js).astype(B_.CONTACT_JOINT_DTYPE)
        for prec in ("float32", "float64"):
            w = B_.BatchWorld(n, prec, gravity=(0.0, -9.8, 0.0))
            w.set_cfm(1e-5); w.set_small_tick(B_.SMALL_TICK_OFF)
            w.upload(B_.POS, pos); w.upload(B_.LVEL, lvel)
            for _ in range(10):
                w.step_joints(H, jts)
            w.synchronize()
            t0 = time.perf_counter()
            for _ in range(ticks):
                w.step_joints(H, jts)
            w.synchronize()
            print(f"LEG singles_{contacts}_contacts_{'f32' if prec == 'float32' else 'f64'} {1e3 * (time.perf_counter() - t0) / ticks:.5f}", flush=True)
            w.close()


def child_trace(root):
    """what the kernel trace runs over: the singles scenes, and 40 ticks of a box floor, hulls on the plane and hulls on a floor"""
    child_singles(root, 20)
    import numpy as np
    from __graft_entry__ import load_package, ROOT as tree
    pkg = load_package()
    hull = pkg.hull.build(np.load(os.path.join(tree, "tests", "golden", "teapot_hull.npz"))["points"], 0.01)
    for dtype in ("float32", "float64"):
        scenes = [pkg.scenes.box_grid(100, 100, seed=4, y_range=(0.6, 1.0), spin=False, plane=True).astype(dtype),
                  pkg.scenes.box_grid(320, 320, seed=4, y_range=(1.2, 1.6), spin=False, plane=False).astype(dtype),
                  pkg.scenes.hull_grid(hull, 64, 64, seed=1, y_range=(0.6, 1.0), spin=False, tilt=0.2, floor_box=False, pitch=4.5).astype(dtype),
                  pkg.scenes.hull_grid(hull, 64, 64, seed=1, y_range=(0.6, 1.0), spin=False, tilt=0.2, floor_box=True, pitch=4.5).astype(dtype)]
        for k, scene in enumerate(scenes):
            w = pkg.BatchWorld(scene.n, dtype=dtype); w.load_scene(scene)
            if k == 1:
                w.set_static_boxes([((1000.0, 1.0, 1000.0), (0.0, 0.0, 0.0), pkg.scenes._rot_z(0.0))])
            if k >= 2:
                w.set_class_pairs(pkg.scenes.GEOM_CONVEX, pkg.scenes.GEOM_CONVEX, False)
            w.step(H, 100); w.synchronize()
            w.close()


# ---------------------------------------------------------------------------------------------------------- the driver
class Out:
    def __init__(self, path):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        self.f = open(path, "a")

    def line(self, text):
        print(text, flush=True)
        self.f.write(text + "\n"); self.f.flush()

    def run(self, leg, build, value, unit):
        self.line(f"RUN {build:6s} {leg:58s} {value:11.4f} {unit}")


def step(out, what, cmd, limit, env=None, cwd=None):
    """one GPU step under its own time limit; the first failure ends the script"""
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True, env=env, cwd=cwd)
    if p.returncode != 0:
        out.line(f"FAILED ({p.returncode}): {what}\n{p.stdout[-1500:]}\n{p.stderr[-1500:]}")
        sys.exit(1)
    return p.stdout


def repeats(out, a):
    for k in range(a.repeats):
        if a.budget and time.time() - a.leg_t0 > a.budget:
            out.line(f"## (the time budget of {a.budget} s ended this leg after {k} of {a.repeats} repetitions)")
            return
        yield k


def leg_dump(out, builds, a):
    out.line("## bench.py --steps 200 --warmup 20 --dump-outputs on both builds: cmp of the arrays")
    tmp = tempfile.mkdtemp()
    for dt in ("f32", "f64"):
        for name, tree in builds:
            step(out, f"dump {name} {dt}", [sys.executable, os.path.join(tree, "bench.py"), "--steps", "200", "--warmup", "20", "--dtype", dt,
                                            "--dump-outputs", os.path.join(tmp, f"{name}_{dt}")], 300, cwd=tree)
        for f in sorted(glob.glob(os.path.join(tmp, f"parent_{dt}", "*.npy"))):
            rc = subprocess.run(["cmp", f, os.path.join(tmp, f"this_{dt}", os.path.basename(f))]).returncode
            out.line(f"CMP {dt} {os.path.basename(f)} ({os.path.getsize(f)} bytes): cmp exit status {rc}")
            if rc != 0:
                sys.exit(1)
    shutil.rmtree(tmp, ignore_errors=True)


def leg_floor(out, builds, a):
    out.line("## scripts/time_floor.py, ms per tick of 240")
    for _ in repeats(out, a):
        for dt in ("f32", "f64"):
            for name, tree in builds:
                text = step(out, f"time_floor {name} {dt}", [sys.executable, os.path.join(ROOT, "scripts", "time_floor.py"), dt, "--root=" + tree], 300, cwd=tree)
                for label, ms in re.findall(r"^\s*(.+?):\s+([0-9.]+) ms/tick", text, re.M):
                    out.run(f"{dt} {re.sub(r'  +', ' ', label)}", name, float(ms), "ms/tick")


def leg_singles(out, builds, a):
    out.line("## dmxBatchStepJoints, 4096 one-body islands with contacts handed in, general path, ms per tick of 200")
    for _ in repeats(out, a):
        for name, tree in builds:
            text = step(out, f"singles {name}", [sys.executable, os.path.abspath(__file__), "--leg", "singles", "--root", tree], 200, cwd=tree)
            for label, ms in re.findall(r"^LEG (\S+) ([0-9.]+)", text, re.M):
                out.run(label, name, float(ms), "ms/tick")


def leg_small(out, builds, a):
    out.line("## scripts/time_stability.py's 48-body single-launch legs (24 cart-poles; 12 four-stacks with auto-disable on), ms per tick of 200")
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import time_stability as ts
    for _ in repeats(out, a):
        for name, tree in builds:
            for code, count, what in ((ts.CARTPOLES, 4, "cart-poles"), (ts.AD_STACKS, 8, "four-stacks AD")):
                text = step(out, f"small {what} {name}", [sys.executable, "-c", code, tree, "untouched", "200"], 200, cwd=tree)
                for k, x in enumerate(text.split()[-count:]):
                    out.run(f"{what} {ts.LEGS[k % 4]}{' feedback on' if k >= 4 else ''}", name, float(x), "ms/tick")


def leg_bench(out, builds, a):
    out.line("## bench.py --full --no-cpu-baseline --steps 200 --warmup 20 --hbm-side 1024, us per tick")
    for _ in repeats(out, a):
        for name, tree in builds:
            text = step(out, f"bench {name}", [sys.executable, os.path.join(tree, "bench.py"), "--full", "--no-cpu-baseline", "--steps", "200",
                                               "--warmup", "20", "--hbm-side", "1024"], 420, cwd=tree)
            o = json.loads([l for l in text.splitlines() if l.startswith("{")][-1])
            legs = list(o.get("configs", {}).items()) + [("pen_" + k, v) for k, v in o.get("reference_pen", {}).items()]
            for k, leg in legs:
                if "ms_per_step" not in leg:
                    out.line(f"FAILED: bench {name} {k}: {leg.get('error')}")
                    sys.exit(1)
                out.run(f"bench {k}", name, leg["ms_per_step"] * 1e3, "us/tick")


def leg_trace(out, builds, a):
    out.line("## rocprofv3 --kernel-trace --stats, one pass per build, over the singles scenes and 100 ticks of each floor scene kind: average us per call")
    for name, tree in builds:
        d = tempfile.mkdtemp()
        step(out, f"trace {name}", ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
                                    os.path.abspath(__file__), "--leg", "trace", "--root", tree], 400, cwd=tree)
        f = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)[0]
        for r in csv.DictReader(open(f)):
            m = re.search(r"(step_plane|step_contacts|solve_singles_lds|solve_singles)<[^(]*", r["Name"])
            if m:
                out.line(f"TRACE {name:6s} {float(r['AverageNs']) / 1e3:10.3f} us average over {int(r['Calls']):6d} calls  {m.group(0)[:90]}")
        shutil.rmtree(d, ignore_errors=True)


def summary(out, path):
    runs = {}
    for l in open(path):
        m = re.match(r"RUN (\w+)\s+(.+?)\s+([0-9.]+) (ms|us)/tick$", l)
        if m:
            runs.setdefault((m.group(2), m.group(1)), []).append(float(m.group(3)))
    out.line("## medians, spread = max - min; verdict: this build's median less the parent's against the parent's spread")
    worst = 0
    for leg in sorted({l for l, _ in runs}):
        p, t = runs.get((leg, "parent")), runs.get((leg, "this"))
        if not p or not t:
            continue
        mp, mt, sp = statistics.median(p), statistics.median(t), max(p) - min(p)
        ok = mt - mp <= sp
        worst += not ok
        out.line(f"VERDICT {leg:58s} parent {mp:11.4f} [{min(p):.4f} .. {max(p):.4f}] spread {sp:9.4f}  this {mt:11.4f} [{min(t):.4f} .. {max(t):.4f}]  "
                 f"this - parent {mt - mp:+9.4f}  n={len(p)}  -> " + ("not slower beyond the parent's spread" if ok else "SLOWER than the parent by more than its spread"))
    out.line(f"legs slower than the parent by more than its spread: {worst}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "fused_dedup_ab.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default="dump,floor,singles,small,bench,trace")
    ap.add_argument("--budget", type=float, default=0)
    ap.add_argument("--leg", help="(a child's: run one leg's scenes on the build of the checkout --root)")
    ap.add_argument("--root", help="(a child's)")
    a = ap.parse_args()
    if a.leg == "singles":
        child_singles(os.path.abspath(a.root), 200)
    elif a.leg == "trace":
        child_trace(os.path.abspath(a.root))
    else:
        if not a.parent:
            ap.error("--parent is required")
        builds = [("parent", os.path.abspath(a.parent)), ("this", ROOT)]
        out = Out(a.out)
        out.line(f"# the one-body ticks against the parent's build ({time.strftime('%Y-%m-%d')}), legs: {a.only}, repeats {a.repeats}")
        for name, f in (("dump", leg_dump), ("floor", leg_floor), ("singles", leg_singles), ("small", leg_small), ("bench", leg_bench), ("trace", leg_trace)):
            if name in a.only.split(","):
                a.leg_t0 = time.time()
                f(out, builds, a)
        summary(out, a.out)
