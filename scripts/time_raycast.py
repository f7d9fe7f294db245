"""Times dmxBatchRayCastDevice (rays and results stay on the device): the grid walk against the brute-force form, the large
scene, and one pick ray into the reference's pen.  Wall time of enqueue + wait around each cast, medians of five after two
warm-up casts (the first one builds the grid; the build is timed on its own); kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python scripts/time_raycast.py --once` run.

    python scripts/time_raycast.py [--once] [--skip-large]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
B = pkg.batch


def rays_over(scene, n, seed, length=30.0):
    rng = np.random.default_rng(seed)
    lo, hi = scene.pos.min(0) - 1.0, scene.pos.max(0) + 1.0
    lo[1], hi[1] = 0.25, scene.pos[:, 1].max() + 4.0
    o = rng.uniform(lo, hi, size=(n, 3))
    d = rng.normal(size=(n, 3))
    return np.concatenate([o, d, np.full((n, 1), length)], 1)


def timed(w, t_rays, t_ids, t_hits, n, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        w.ray_cast_device(t_rays.data_ptr(), n, t_ids.data_ptr(), t_hits.data_ptr())
        w.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def case(name, scene, statics, n_rays, forms, dtype, reps, seed=1):
    import torch
    w = pkg.BatchWorld(scene.n, dtype=dtype)
    w.load_scene(scene.astype(dtype))
    if statics:
        w.set_static_boxes(statics)
    rays = rays_over(scene, n_rays, seed).astype(dtype)
    t_rays = torch.from_numpy(rays).cuda()
    t_ids = torch.zeros(n_rays, dtype=torch.int32, device="cuda")
    t_hits = torch.zeros((n_rays, 7), dtype=t_rays.dtype, device="cuda")
    torch.cuda.synchronize()
    res = {}
    ref_ids = None
    for form, label in forms:
        w.set_ray_form(form)
        pos = w.download(B.POS)
        w.upload(B.POS, pos)                       # the state "changed": the next cast builds the grid
        t0 = time.perf_counter()
        w.ray_cast_device(t_rays.data_ptr(), n_rays, t_ids.data_ptr(), t_hits.data_ptr())
        w.synchronize()
        first = (time.perf_counter() - t0) * 1e3
        if reps > 1:
            timed(w, t_rays, t_ids, t_hits, n_rays, 1)
        ms = statistics.median(timed(w, t_rays, t_ids, t_hits, n_rays, reps))
        ids = t_ids.cpu().numpy()
        same = "" if ref_ids is None else ("  == first form" if np.array_equal(ids, ref_ids) else "  DIFFERS from the first form")
        ref_ids = ids if ref_ids is None else ref_ids
        res[label] = ms
        print(f"{name:34s} {dtype:8s} {label:6s} {n_rays:8d} rays  first cast (with build) {first:9.3f} ms   median of {reps} {ms:9.3f} ms   "
              f"{n_rays / ms / 1e3:9.2f} Mrays/s   {100.0 * (ids != B.RAY_MISS).mean():5.1f} % hit{same}", flush=True)
    w.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--once", action="store_true", help="one cast per case and form (for a kernel trace)")
    ap.add_argument("--skip-large", action="store_true")
    a = ap.parse_args()
    reps = 1 if a.once else 5
    S = pkg.scenes
    lane, wave, brute = (B.RAY_FORM_LANE, "lane"), (B.RAY_FORM_WAVE, "wave"), (B.RAY_FORM_BRUTE, "brute")
    for dtype in ("float32", "float64"):
        r = case("4 096 boxes on the plane", S.config3(64), None, 65536, [lane, brute], dtype, reps)
        print(f"    lane is {r['brute'] / r['lane']:.1f} x faster than brute ({dtype})", flush=True)
        assert r["lane"] < r["brute"], "the grid walk loses to the all-pairs loop"
        if not a.skip_large:
            case("262 144 boxes on the plane", S.config3(512), None, 1048576, [lane], dtype, reps)
        pen, statics, _ = S.reference_pen(512)
        case("512 bodies in the reference's pen", pen, statics, 1, [wave, lane], dtype, reps)


if __name__ == "__main__":
    main()
