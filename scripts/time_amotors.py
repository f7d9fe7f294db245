"""Timings for the angular motors (dmxBatchSetAMotors, DMX_JOINT_AMOTOR), on one GPU.

usage: python scripts/time_amotors.py ab PARENT_ROOT [--runs 5]
       python scripts/time_amotors.py cost [--ticks 200] [--repeats 5]

ab    no AMotor anywhere, against a checkout of the parent commit that has been built (PARENT_ROOT): the legs of
      scripts/time_surface.py's `ab` -- the 48- / 512-body dWorldStep pen, the 400- / 512-body QuickStep pen, 24 cart-poles on the
      single-launch tick -- and scripts/time_sliders.py's star of 100 sliders, float32 and float64, each tree's own scripts with its own
      libraries, the two builds alternately, `runs` each; then per leg the medians, the parent's own spread and whether the new median
      lies inside it.  A child that ends with any status but 0 ends the script at once: nothing more is started on the GPU.
cost  24 two-link arms (48 bodies: world - ball - link - ball - link), QuickStep and dWorldStep, float32 and float64, on the
      single-launch tick and on the general path: with the balls alone, and with an Euler AMotor beside every ball (three stops each,
      a third of them violated); ms per tick (step_joints + synchronize after 20 ticks of warm-up).  Then the prepare pass by itself as
      dmxBatchAMotorAngles runs it: one upload of the records, the kernel, one wait, one download -- an upper bound on the kernel.
      Reported, not gated."""
import argparse
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import time_surface as ts  # noqa: E402

H = 1.0 / 60.0


def legs(root):
    """time_surface.legs with the slider star read from the same run of time_sliders.py as the cart-poles -> {leg: ms}"""
    out = {}
    py = sys.executable
    for single in (False, True):
        prec = "f32" if single else "f64"
        for name, bodies, env in (("dWorldStep pen", "48,512", []), ("QuickStep  pen", "400,512", ["--env", "HARNESS_STEPPER=quick"])):
            cmd = [py, os.path.join(root, "scripts", "time_dworldstep.py"), "--bodies", bodies] + (["--single"] if single else []) + env
            text = ts.child(cmd, root, 300)
            found = {int(m.group(1)): float(m.group(2)) for m in re.finditer(r"bodies=(\d+) f\d+ timed_ticks=\d+ ms_per_tick=([\d.]+)", text)}
            for n in (int(v) for v in bodies.split(",")):
                if n not in found:
                    raise ts.LegFailed(f"no figure for {name}, {n} bodies, {prec} in the output of {' '.join(cmd)}:\n{text[-1500:]}")
                out[f"{name}, {n:3d} bodies, {prec}"] = found[n]
    cmd = [py, os.path.join(root, "scripts", "time_sliders.py"), "--repeats", "1"]
    text = ts.child(cmd, root, 300)
    for scene, label in (("24 cart-poles \\(48 bodies\\)", "24 cart-poles small tick"), ("star of 100 sliders", "star of 100 sliders")):
        found = {(m.group(1), m.group(2)): float(m.group(3)) for m in re.finditer(scene + r"\s+(\w+)\s+(float\d+)\s+median ([\d.]+) ms", text)}
        for stepper in ("quick", "exact"):
            for prec in ("float32", "float64"):
                if (stepper, prec) not in found:
                    raise ts.LegFailed(f"no figure for {label}, {stepper}, {prec} in the output of {' '.join(cmd)}:\n{text[-1500:]}")
                out[f"{label}, {stepper}, {prec}"] = found[(stepper, prec)]
    return out


def cost(ticks, repeats):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import amotor_dense as am
    import joint_dense as jd
    import lcp_dense as ld
    from __graft_entry__ import load_package
    B_ = load_package().batch

    def to_c(arr, dtype):
        out = np.zeros(len(arr), dtype)
        for f in dtype.names:
            out[f] = arr[f]
        return out

    rng = np.random.default_rng(13)
    n = 48
    pos = np.column_stack([3.0 * (np.arange(n) // 2), 3.0 - (np.arange(n) % 2), np.zeros(n)])
    B = ld.Bodies(pos, am.random_quats(rng, n), rng.normal(scale=0.3, size=(n, 3)), rng.normal(scale=0.3, size=(n, 3)),
                  rng.uniform(0.5, 2.0, n), rng.uniform(0.3, 1.0, (n, 3)))
    balls, art, mot = [], [], []
    for p in range(24):
        a, b = 2 * p, 2 * p + 1
        for b1, b2, anchor in ((a, -1, B.pos[a] + (0.0, 0.5, 0.0)), (b, a, B.pos[a] + (0.0, -0.5, 0.0))):
            ball = jd.from_world(B, jd.BALL, b1, b2, anchor)
            balls.append(ball)
            art.append(ball)
            mot.append(am.motors(1)[0])
            m = am.from_world(B, b1, b2, am.EULER, am.perpendicular_pair(rng))
            m["lo_stop"], m["hi_stop"] = -0.6, 0.6
            if len(art) % 3 == 0:
                m["lo_stop"][(len(art) // 3) % 3] = 0.1
            art.append(am.joint(b1, b2))
            mot.append(m)
    sets = {"balls alone": (np.array(balls, jd.ART_DTYPE), None), "balls + Euler AMotors": (np.array(art, jd.ART_DTYPE), np.array(mot, am.AMOTOR_DTYPE))}

    def run(a, m, prec, stepper, small, angles=False):
        w = B_.BatchWorld(B.n, prec)
        try:
            w.set_erp(0.2); w.set_cfm(1e-5)
            w.set_stepper(B_.STEPPER_EXACT if stepper == "exact" else B_.STEPPER_QUICK)
            w.set_small_tick(small)
            w.upload(B_.POS, B.pos); w.upload(B_.QUAT_RAW, B.quat); w.upload(B_.LVEL, B.lvel); w.upload(B_.AVEL, B.avel)
            w.upload(B_.MASS, B.mass); w.upload(B_.INERTIA, B.inertia)
            w.upload_body_flags(B.flags)
            w.set_joints(to_c(a, B_.JOINT_DTYPE))
            if m is not None:
                w.set_amotors(to_c(m, B_.AMOTOR_DTYPE))
            none = np.zeros(0, B_.CONTACT_JOINT_DTYPE)
            for _ in range(20):
                w.step_joints(H, none)
            w.synchronize()
            if angles:
                w.amotor_angles()
                t0 = time.perf_counter()
                for _ in range(ticks):
                    w.amotor_angles()
                return 1e3 * (time.perf_counter() - t0) / ticks
            t0 = time.perf_counter()
            for _ in range(ticks):
                w.step_joints(H, none)
                w.synchronize()
            dt = (time.perf_counter() - t0) / ticks
            st = w.small_tick_stats()
            assert bool(st["small"]) == (small == B_.SMALL_TICK_AUTO), st
            return 1e3 * dt
        finally:
            w.close()

    for small, path in ((B_.SMALL_TICK_AUTO, "single-launch tick"), (B_.SMALL_TICK_OFF, "general path")):
        for stepper in ("quick", "exact"):
            for prec in ("float32", "float64"):
                for label, (a, m) in sets.items():
                    ms = sorted(run(a, m, prec, stepper, small) for _ in range(repeats))
                    print(f"time_amotors  24 two-link arms  {path:18s} {stepper:5s} {prec}  {label:22s} median {ms[len(ms) // 2]:.4f} ms  "
                          f"min {ms[0]:.4f}  max {ms[-1]:.4f}", flush=True)
    a, m = sets["balls + Euler AMotors"]
    for prec in ("float32", "float64"):
        ms = sorted(run(a, m, prec, "quick", B_.SMALL_TICK_AUTO, angles=True) for _ in range(repeats))
        print(f"time_amotors  dmxBatchAMotorAngles (96 joints: upload, amotor_prepare, wait, download) {prec}  median {ms[len(ms) // 2]:.4f} ms  "
              f"min {ms[0]:.4f}  max {ms[-1]:.4f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="what", required=True)
    a1 = sub.add_parser("ab")
    a1.add_argument("parent_root")
    a1.add_argument("--runs", type=int, default=5)
    a2 = sub.add_parser("cost")
    a2.add_argument("--ticks", type=int, default=200)
    a2.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if a.what == "ab":
        ts.legs = legs          # (time_surface.ab with the slider star added)
        ts.ab(a.parent_root, a.runs)
    else:
        cost(a.ticks, a.repeats)


if __name__ == "__main__":
    main()
