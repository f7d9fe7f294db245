"""What friction bounded by the normal force (DMX_CONTACT_APPROX1) costs a dmxBatchStepJoints tick: one pile-like island (a chain of
100 bodies, 400 contacts of three rows: 1 200 rows) and 256 two-box stacks (the single-launch tick's and the small islands' forms),
every contact mu = 0.5 with the bits against mu = 0.5 without, both steppers, both precisions.
usage: python scripts/time_friction.py [--ticks 100] [--repeats 5]
Prints ms per tick (step_joints + synchronize, after 10 ticks of warm-up; the state is uploaded afresh for every run)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lcp_dense as ld  # noqa: E402
import test_gpu_solver_dense as sd  # noqa: E402

B_ = sd.B_
H = 1.0 / 60.0
APPROX1 = 0x3000


def scenes():
    rng = np.random.default_rng(3)
    B, j = sd.chain(100, 400, 0.5, rng, speed=0.05)
    B.lvel[:, 1] -= 1.0
    yield "pile: 1 island of 1200 rows", B, j
    parts = [sd.chain(2, 8, 0.5, rng, speed=0.05) for _ in range(256)]
    off, Bs, js = 0, [], []
    for k, (b, jj) in enumerate(parts):
        b.pos[:, 0] += 3.0 * (k % 16)
        b.pos[:, 2] += 3.0 * (k // 16)
        jj = jj.copy()
        jj["pos"][:, 0] += 3.0 * (k % 16)
        jj["pos"][:, 2] += 3.0 * (k // 16)
        jj["body1"] += off
        jj["body2"] = np.where(jj["body2"] >= 0, jj["body2"] + off, -1)
        Bs.append(b); js.append(jj); off += b.n
    B = ld.Bodies(*[np.vstack([getattr(b, f) for b in Bs]) for f in ("pos", "quat", "lvel", "avel")],
                  np.concatenate([b.mass for b in Bs]), np.vstack([b.inertia for b in Bs]))
    yield "256 stacks of 24 rows", B, np.concatenate(js)


def run(B, jts, prec, stepper, ticks):
    w = B_.BatchWorld(B.n, prec)
    try:
        w.set_cfm(1e-5)
        w.set_stepper(B_.STEPPER_EXACT if stepper == "exact" else B_.STEPPER_QUICK)
        w.upload(B_.POS, B.pos); w.upload(B_.QUAT_RAW, B.quat); w.upload(B_.LVEL, B.lvel); w.upload(B_.AVEL, B.avel)
        w.upload(B_.MASS, B.mass); w.upload(B_.INERTIA, B.inertia)
        j = jts.astype(B_.CONTACT_JOINT_DTYPE)
        for _ in range(10):
            w.step_joints(H, j)
        w.synchronize()
        t0 = time.perf_counter()
        for _ in range(ticks):
            w.step_joints(H, j)
            w.synchronize()
        return 1e3 * (time.perf_counter() - t0) / ticks
    finally:
        w.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    for name, B, jts in scenes():
        for stepper in ("quick", "exact"):
            for prec in ("float32", "float64"):
                for label, mode in (("box mu=0.5", 0), ("APPROX1 mu=0.5", APPROX1)):
                    j = jts.copy()
                    j["mode"] |= mode
                    ms = sorted(run(B, j, prec, stepper, a.ticks) for _ in range(a.repeats))
                    print(f"time_friction  {name:30s} {stepper:5s} {prec}  {label:15s} median {ms[len(ms) // 2]:.4f} ms  min {ms[0]:.4f}  max {ms[-1]:.4f}", flush=True)


if __name__ == "__main__":
    main()
