"""Milliseconds per dmxBatchStepJoints tick of two worlds with slider joints: a star of 100 motorised sliders round a heavy hub (one
island of 600 rows: QuickStep's workgroup form, dWorldStep's grid solve) and 24 cart-poles (48 bodies, 24 islands of 11 rows: the
single-launch tick), both steppers, both precisions.  Timed is the step call up to the point where the new state can be read
(step_joints + synchronize); median, min and max over the timed ticks' repeats.
--feedback 1 switches dmxBatchSetFeedback on (the ticks leave every joint's force and torque on the device), 2 also reads it back
after every tick (joint_feedback), inside the timed region.
usage: python scripts/time_sliders.py [--ticks 200] [--repeats 5] [--feedback 0|1|2]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lcp_dense as ld  # noqa: E402
import slider_dense as sd  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
B_ = pkg.batch
H = 1.0 / 60.0


def to_c(arr, dtype):
    out = np.zeros(len(arr), dtype)
    for f in dtype.names:
        out[f] = arr[f]
    return out


def scenes():
    B, art, lim = sd.slider_star(100)
    yield "star of 100 sliders", B, art, lim
    parts = [sd.cart_pole(vel=1.0 if p % 2 else -1.0, fmax=5.0, lean=0.1 * (p % 5 - 2), at=(-2.0 + 0.7 * (p % 6), 1.0 + 1.5 * (p // 6), 0.0))
             for p in range(24)]
    B, art, lim = sd.merge(parts, dx=0.0)
    yield "24 cart-poles (48 bodies)", B, art, lim


def run(B, art, lim, prec, stepper, ticks, feedback=0):
    w = B_.BatchWorld(B.n, prec)
    try:
        w.set_erp(0.2); w.set_cfm(1e-5)
        w.set_stepper(B_.STEPPER_EXACT if stepper == "exact" else B_.STEPPER_QUICK)
        w.upload(B_.POS, B.pos); w.upload(B_.QUAT_RAW, B.quat); w.upload(B_.LVEL, B.lvel); w.upload(B_.AVEL, B.avel)
        w.upload(B_.MASS, B.mass); w.upload(B_.INERTIA, B.inertia)
        w.upload_body_flags(B.flags)
        w.set_joints(to_c(art, B_.JOINT_DTYPE))
        w.set_hinge_limots(to_c(lim, B_.HINGE_LIMOT_DTYPE))
        none = np.zeros(0, B_.CONTACT_JOINT_DTYPE)
        if feedback:
            w.set_feedback(True)
        for _ in range(20):
            w.step_joints(H, none)
        w.synchronize()
        t0 = time.perf_counter()
        for _ in range(ticks):
            w.step_joints(H, none)
            w.synchronize()
            if feedback == 2:
                w.joint_feedback()
        dt = (time.perf_counter() - t0) / ticks
        st = w.small_tick_stats()
        return 1e3 * dt, "small tick" if st["small"] else "general path"
    finally:
        w.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--feedback", type=int, default=0, help="1: feedback on; 2: on, and read back after every tick")
    a = ap.parse_args()
    for name, B, art, lim in scenes():
        for stepper in ("quick", "exact"):
            for prec in ("float32", "float64"):
                r = [run(B, art, lim, prec, stepper, a.ticks, a.feedback) for _ in range(a.repeats)]
                ms = sorted(x[0] for x in r)
                fb = f", feedback {a.feedback}" if a.feedback else ""
                print(f"{name:28s} {stepper:5s} {prec}  median {ms[len(ms) // 2]:.4f} ms  min {ms[0]:.4f}  max {ms[-1]:.4f}  ({r[0][1]}{fb})", flush=True)


if __name__ == "__main__":
    main()
