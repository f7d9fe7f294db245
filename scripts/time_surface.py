"""Timings for the extended contact surface (dmxBatchStepJointsSurface: mu2, fdir1, motion, slip), on one GPU.

usage: python scripts/time_surface.py ab PARENT_ROOT [--runs 5]
       python scripts/time_surface.py cost [--ticks 50] [--repeats 3]

ab    no bit set, against a checkout of the parent commit that has been built (PARENT_ROOT): the legs of profiles/approx1_ab.txt --
      scripts/time_dworldstep.py's 48- / 512-body dWorldStep pen and its 400- / 512-body QuickStep pen, scripts/time_sliders.py's 24
      cart-poles, float32 and float64 -- each tree's own scripts with its own libraries, the two builds alternately (parent, new,
      parent, new, ...), `runs` each; then per leg the medians, the parent's own spread and whether the new median lies inside it.
      Every child runs under a time limit of its own; a child that ends with any status but 0, or a leg without its figure, ends the
      script at once -- nothing more is started on the GPU, and no median is printed over fewer runs than asked for.
cost  an extended tick against the same contacts plain: scripts/time_friction.py's 1 200-row island and 256 two-box stacks with
      FDIR1 | MU2 | SLIP2 on every contact (mu 0.5 / mu2 0.2 / slip2 0.01, fdir1 orthogonal to the normal), both steppers, both
      precisions; ms per tick (step_joints + synchronize after 10 ticks of warm-up).  Reported, not gated."""
import argparse
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
H = 1.0 / 60.0
MU2, FDIR1, SLIP2 = 0x001, 0x002, 0x200


class LegFailed(RuntimeError):
    pass


def child(cmd, root, limit):
    """one child that uses the GPU, under a time limit of its own that also ends what the child started (`timeout -k 10`); any exit
    status but 0 -- a fault, an abort (134), a segmentation fault (139), the limit (124 / 137) included -- ends the whole script:
    nothing more is started on the card"""
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True, cwd=root)
    if p.returncode != 0 or "FAILED" in p.stdout:
        raise LegFailed(f"exit status {p.returncode} of {' '.join(cmd)} in {root}\n{p.stdout[-1500:]}\n{p.stderr[-2500:]}")
    return p.stdout


def legs(root):
    """one pass over the legs with the tree at `root` -> {leg: ms}; every leg must give its number"""
    out = {}
    py = sys.executable
    for single in (False, True):
        prec = "f32" if single else "f64"
        for name, bodies, env in (("dWorldStep pen", "48,512", []), ("QuickStep  pen", "400,512", ["--env", "HARNESS_STEPPER=quick"])):
            cmd = [py, os.path.join(root, "scripts", "time_dworldstep.py"), "--bodies", bodies] + (["--single"] if single else []) + env
            text = child(cmd, root, 300)
            found = {int(m.group(1)): float(m.group(2)) for m in re.finditer(r"bodies=(\d+) f\d+ timed_ticks=\d+ ms_per_tick=([\d.]+)", text)}
            for n in (int(v) for v in bodies.split(",")):
                if n not in found:
                    raise LegFailed(f"no figure for {name}, {n} bodies, {prec} in the output of {' '.join(cmd)}:\n{text[-1500:]}")
                out[f"{name}, {n:3d} bodies, {prec}"] = found[n]
    cmd = [py, os.path.join(root, "scripts", "time_sliders.py"), "--repeats", "1"]
    text = child(cmd, root, 300)
    found = {(m.group(1), m.group(2)): float(m.group(3))
             for m in re.finditer(r"24 cart-poles \(48 bodies\)\s+(\w+)\s+(float\d+)\s+median ([\d.]+) ms", text)}
    for stepper in ("quick", "exact"):
        for prec in ("float32", "float64"):
            if (stepper, prec) not in found:
                raise LegFailed(f"no figure for 24 cart-poles, {stepper}, {prec} in the output of {' '.join(cmd)}:\n{text[-1500:]}")
            out[f"24 cart-poles small tick, {stepper}, {prec}"] = found[(stepper, prec)]
    return out


def ab(parent_root, runs):
    got = {"parent": {}, "new": {}}
    for _ in range(runs):
        for which, root in (("parent", os.path.abspath(parent_root)), ("new", ROOT)):
            try:
                one = legs(root)
            except LegFailed as e:
                sys.exit(f"time_surface: stopped, nothing more is started: {e}")
            for leg, ms in one.items():
                got[which].setdefault(leg, []).append(ms)
    assert all(len(r) == runs for w in got.values() for r in w.values()) and list(got["parent"]) == list(got["new"])
    names = list(got["new"])
    for leg in names:
        for which in ("new", "parent"):
            r = got[which].get(leg, [])
            if r:
                print(f"{leg:44s} {which:6s} median {np.median(r):.4f} ms  min {min(r):.4f}  max {max(r):.4f}  runs " + " ".join(f"{x:.4f}" for x in r), flush=True)
    print()
    for leg in names:
        n, p = got["new"][leg], got["parent"].get(leg, [])
        if not p:
            continue
        mn, mp = float(np.median(n)), float(np.median(p))
        where = "inside" if min(p) <= mn <= max(p) else ("BELOW " if mn < min(p) else "ABOVE ")
        print(f"  {leg:44s} new {mn:.4f}   parent {min(p):.4f} .. {max(p):.4f} (median {mp:.4f}, spread {max(p) - min(p):.4f})   {where} {100 * (mn / mp - 1):+.1f} %")


def cost(ticks, repeats):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import time_friction as tf
    B_ = tf.B_

    def run(B, jts, srf, prec, stepper):
        w = B_.BatchWorld(B.n, prec)
        try:
            w.set_cfm(1e-5)
            w.set_stepper(B_.STEPPER_EXACT if stepper == "exact" else B_.STEPPER_QUICK)
            w.upload(B_.POS, B.pos); w.upload(B_.QUAT_RAW, B.quat); w.upload(B_.LVEL, B.lvel); w.upload(B_.AVEL, B.avel)
            w.upload(B_.MASS, B.mass); w.upload(B_.INERTIA, B.inertia)
            j = jts.astype(B_.CONTACT_JOINT_DTYPE)
            for _ in range(10):
                w.step_joints(H, j, srf)
            w.synchronize()
            t0 = time.perf_counter()
            for _ in range(ticks):
                w.step_joints(H, j, srf)
                w.synchronize()
            return 1e3 * (time.perf_counter() - t0) / ticks
        finally:
            w.close()

    for name, B, jts in tf.scenes():
        srf = np.zeros(len(jts), B_.CONTACT_SURFACE_DTYPE)
        srf["mu2"], srf["slip2"] = 0.2, 0.01
        d = np.cross(jts["normal"], (0.3, 0.5, 0.8))
        srf["fdir1"] = d / np.linalg.norm(d, axis=1)[:, None]
        ext = jts.copy()
        ext["mode"] |= MU2 | FDIR1 | SLIP2
        for stepper in ("quick", "exact"):
            for prec in ("float32", "float64"):
                for label, j, s in (("plain mu=0.5", jts, None), ("FDIR1|MU2|SLIP2", ext, srf)):
                    ms = sorted(run(B, j, s, prec, stepper) for _ in range(repeats))
                    print(f"time_surface  {name:30s} {stepper:5s} {prec}  {label:16s} median {ms[len(ms) // 2]:.4f} ms  min {ms[0]:.4f}  max {ms[-1]:.4f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="what", required=True)
    a1 = sub.add_parser("ab")
    a1.add_argument("parent_root")
    a1.add_argument("--runs", type=int, default=5)
    a2 = sub.add_parser("cost")
    a2.add_argument("--ticks", type=int, default=50)
    a2.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if a.what == "ab":
        ab(a.parent_root, a.runs)
    else:
        cost(a.ticks, a.repeats)


if __name__ == "__main__":
    main()
