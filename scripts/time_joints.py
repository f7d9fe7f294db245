"""Milliseconds per dmxBatchStepJoints tick of worlds made of 8-link ragdoll-like chains (ball and hinge joints in turn) that
fall onto the ground and lie there on sphere-ground contacts: 48 and 512 bodies, both steppers, both precisions.
The contacts of a tick are made on the host from the poses read back (a sphere of radius 0.5 per link against y = 0), outside
the timed region; timed is the step call up to the point where the new state can be read (step_joints + synchronize).
--feedback 1 switches dmxBatchSetFeedback on; 2 also reads the joints' and the contacts' feedback back after every tick, inside the
timed region.
usage: python scripts/time_joints.py [--bodies 48,512] [--settle 120] [--ticks 200] [--small-tick 0|1] [--mu 1.0] [--only f32:exact] [--feedback 0|1|2]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
B_ = pkg.batch
H = 1.0 / 120.0
LINKS, RADIUS = 8, 0.5


def scene(n, seed=3):
    """n / 8 chains side by side, each a zigzag of 8 links one unit apart, two to three units above the ground"""
    rng = np.random.default_rng(seed)
    pos = np.zeros((n, 3))
    for s in range(n):
        c, k = divmod(s, LINKS)
        pos[s] = (3.0 * (c % 8) + 0.3 * (k % 2), 2.0 + 0.9 * k * 0.12 + 0.5 * (k % 2), 9.0 * (c // 8) + 0.95 * k)
    quat = rng.normal(size=(n, 4))
    quat /= np.linalg.norm(quat, axis=1)[:, None]
    return pos, quat


def joints(w, n, pos):
    out = []
    for s in range(n):
        if s % LINKS == 0:
            continue
        mid = 0.5 * (pos[s] + pos[s - 1])
        if s % 2:
            out.append(w.joint_from_world(B_.JOINT_BALL, s, s - 1, mid))
        else:
            out.append(w.joint_from_world(B_.JOINT_HINGE, s, s - 1, mid, (1.0, 0.0, 0.0)))
    return np.array(out, B_.JOINT_DTYPE)


def contacts(pos, mu=1.0):
    low = np.nonzero(pos[:, 1] < RADIUS)[0]
    c = np.zeros(len(low), B_.CONTACT_JOINT_DTYPE)
    c["pos"] = pos[low] * (1.0, 0.0, 1.0)
    c["normal"] = (0.0, 1.0, 0.0)
    c["depth"] = RADIUS - pos[low, 1]
    c["body1"], c["body2"] = low, -1
    c["mu"] = mu
    return c


def run(n, prec, stepper, settle, ticks, small, mu=1.0, feedback=0):
    w = B_.BatchWorld(n, prec)
    try:
        pos, quat = scene(n)
        w.upload(B_.POS, pos); w.upload(B_.QUAT, quat)
        w.upload(B_.MASS, np.ones(n)); w.upload(B_.INERTIA, np.full((n, 3), 0.1))
        w.upload_body_flags(np.full(n, B_.BODY_ALIVE, np.uint8))
        w.set_cfm(1e-5)
        w.set_small_tick(B_.SMALL_TICK_AUTO if small else B_.SMALL_TICK_OFF)
        w.set_joints(joints(w, n, pos))
        if feedback:
            w.set_feedback(True)
        times, rows = [], 0
        for t in range(settle + ticks):
            w.set_stepper(B_.STEPPER_EXACT if (stepper == "exact" and t >= settle) else B_.STEPPER_QUICK)
            c = contacts(w.download(B_.POS).astype(np.float64), mu)
            t0 = time.perf_counter()
            w.step_joints(H, c)
            w.synchronize()
            if feedback == 2:
                w.joint_feedback(), w.contact_feedback(len(c))
            if t >= settle:
                times.append(time.perf_counter() - t0)
                rows = max(rows, len(c))
        ms = np.array(times) * 1e3
        pe, ae, mx = w.joint_errors()
        st = w.small_tick_stats()
        slow = int(np.sum(ms > 1.5 * ms.min()))
        print(f"bodies={n:4d} {'f32' if prec == 'float32' else 'f64'} {stepper:5s} small_tick={int(small)} mu={mu:g} feedback={feedback}  median {np.median(ms):.4f} ms  "
              f"min {ms.min():.4f}  p90 {np.percentile(ms, 90):.4f}  ({ticks} ticks, {w.joint_count()} joints, up to {rows} contacts, "
              f"{st['small']} small / {st['general']} general ticks, {slow} ticks above 1.5 x min, joint error {mx[0]:.2e})", flush=True)
    finally:
        w.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bodies", default="48,512")
    ap.add_argument("--settle", type=int, default=120)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--small-tick", type=int, default=1)
    ap.add_argument("--mu", type=float, default=1.0, help="the ground contacts' friction coefficient (inf: rows that never clamp)")
    ap.add_argument("--feedback", type=int, default=0, help="1: feedback on; 2: on, and read back after every tick")
    ap.add_argument("--only", default="", help="one precision and stepper, e.g. f32:exact")
    a = ap.parse_args()
    for n in [int(v) for v in a.bodies.split(",")]:
        for prec in ("float32", "float64"):
            for stepper in ("quick", "exact"):
                if a.only and a.only != f"{'f32' if prec == 'float32' else 'f64'}:{stepper}":
                    continue
                run(n, prec, stepper, a.settle, a.ticks, bool(a.small_tick), a.mu, a.feedback)


if __name__ == "__main__":
    main()
