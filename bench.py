"""bench.py -- body-steps/s of the rigid-body step hot path on MI355X.

One "step" = one tick (collide -> QuickStep -> clear contacts, main.c:211-215) over the whole batch of synthetic bodies.

N = 1   BASELINE.json configs[1]: 1 048 576 free-falling boxes, no contacts, dt = 1/60, f32.  With --full, the same scene
        in f64 (`f64`), an HBM-resident size (`hbm_resident`: 16 Mi bodies, far beyond the 256 MB Infinity Cache), several
        ticks per launch (`fused`), the other configs (`configs`), the reference's pen and call (`reference_pen`,
        `reference_main_c`) and the CPU baselines ride along as extra objects of the one JSON line.
N > 1   BASELINE.json configs[3] as written: the SAME 1 048 576 bodies, in N disjoint slabs >= 10 m apart, one slab of
        1 048 576 / N bodies per GPU (strong scaling), the slabs' boundary rows all-gathered over RCCL / xGMI.  With --full,
        the weak-scaled run (one whole configs[1] slab per GPU) is the extra object `weak`.

A plain run (no --full) sets up, warms up, times the headline's --steps ticks and prints the line: nothing else.
--dump-outputs DIR then writes the state the headline's last timed tick left (pos, quat, lvel, avel of every body the rank
owns, in the run's dtype) as DIR/<name>.npy -- a fixed, seeded sample of the bodies when they exceed 64 MB; rank r of N > 1
writes DIR/rank<r>_<name>.npy.  The scenes are seeded, so the same arguments give the same inputs on every run.

`python bench.py --gpus N` starts by itself: without WORLD_SIZE in the environment the parent spawns the N rank
processes (before it makes any GPU call) and relays rank 0's JSON line; under `torch.distributed.run` the ranks are
already there.  On a box with fewer GPUs than ranks the ranks share cuda:0 and the collectives are staged through gloo --
a functional rehearsal, flagged as such in `data`, never a measurement.

Timing: W untimed warm-up ticks, then ONE block of exactly K ticks (the headline: `ms_per_step` = block time / K),
bracketed by barrier + torch.cuda.synchronize().  The --full companions time blocks of their own step counts; when one
of those is shorter than 50 ms it is repeated and the MEDIAN block is reported.  The closing timestamp is taken after
the local synchronize and before the closing barrier; the job's time is the MAX over ranks.
"""
import argparse
import hashlib
import json
import math
import os
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # this pool's driver only does dmabuf IPC (RCCL across processes)

H = 1.0 / 60.0
HBM_PEAK_GBS = 8000.0            # MI355X_MICROARCH.md: HBM3E peak 8.0 TB/s (spec)
VALU_PEAK_TFLOPS = 157.3         # MI355X_MICROARCH.md: peak FP32 vector (spec); FP64 vector is half of it
BYTES_PER_BODY_STEP = {"free": 30, "plane": 33,    # reals; SURVEY.md 8(d)
                       "convex": 30 + 2 * 7 * 8,   # + the 8 contact slots of 7 reals np_convex_static writes and step_contacts reads back
                       "small": 33}
# what bounds each kind's dominant kernel: HBM traffic for the contact-free pass; VALU issue / the
# Gauss-Seidel dependency chain for the fused contact kernels (12 kflop per 132 B, far above the ridge); launch and
# chain latency for a scene of 1 024 bodies, most of whose ticks are exact ticks (pair search, islands, level-scheduled sweeps)
BOUND_OF = {"free": "hbm", "plane": "valu", "convex": "valu", "small": "latency"}
KERNEL_OF = {"free": "integrate_free", "plane": "step_plane", "convex": "np_convex_static + step_contacts<8>",
             "small": "step_plane / ex_small_front + ex_narrow + ex_small_back + solve_island_wg"}
SOR_FLOP_PER_ROW_SWEEP = 50      # 20 sweeps x rows x ~50 flop
HULL_FLOP_PER_POINT = 36         # R p (15) + x (3) - box centre (3) -> box frame (15): np_convex_static, per hull point walked
MIN_REGION_S = 0.050             # (--full companions) blocks shorter than this are repeated; the median block is reported
MAX_BLOCKS = 401
DUMP_BYTES = 64_000_000          # --dump-outputs: at most this much in all (over the ranks)
DUMP_SEED = 20240601             # the fixed sample of bodies when the state exceeds DUMP_BYTES


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--config", type=int, default=0, choices=[0, 1, 2, 3, 4, 5],
                    help="BASELINE.json configs[] index + 1; 0 = the headline for --gpus (2 at N=1, 4 at N>1)")
    ap.add_argument("--dtype", default="f32", choices=["f32", "f64"])
    ap.add_argument("--side", type=int, default=0, help="grid side (bodies = side^2 on one GPU); 0 = config default")
    ap.add_argument("--exchange", default="boundary", choices=["boundary", "none"])
    ap.add_argument("--graph-steps", type=int, default=16, help="ticks per captured HIP graph when exchanging every tick (0 = eager)")
    ap.add_argument("--no-body-collisions", action="store_true", help="skip the body-body broadphase proof (caller asserts single-body islands)")
    ap.add_argument("--exchange-every-tick", action="store_true",
                    help="all-gather the boundary rows every tick even where the collision proof only needs them at chunk ends")
    ap.add_argument("--rehearse-on-one-gpu", action="store_true",
                    help="N>1 ranks all on cuda:0 with the collectives staged through gloo (chosen by itself when the box has "
                         "fewer GPUs than ranks): a functional rehearsal of the multi-GPU loop, not a measurement")
    ap.add_argument("--ticks-per-launch", type=int, default=1,
                    help="contact-free ticks fused into one launch for the HEADLINE run (default 1 = one launch per tick)")
    ap.add_argument("--fused-ticks", type=int, default=32,
                    help="also time the contact-free scene with this many ticks per launch (extra 'fused' object; 1 = skip)")
    ap.add_argument("--force-exchange", action="store_true", help="run the exchange path even with one rank (debug)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="headline only: no configs / f64 / hbm_resident / fused / weak objects")
    ap.add_argument("--no-configs", action="store_true", help="skip the `configs` object (BASELINE configs[0], [2], [4] timed beside the headline)")
    ap.add_argument("--hbm-side", type=int, default=4096, help="grid side of the hbm_resident extra (4096^2 = 16 Mi bodies)")
    ap.add_argument("--gyro", type=int, default=2, choices=[0, 1, 2], help="0 off, 1 explicit, 2 implicit (ODE default)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--full", action="store_true",
                    help="also run everything beside the headline: the other configs, f64, hbm_resident, fused, weak, the reference's "
                         "pen and call, the CPU baselines (each still subject to the --no-* switches above)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the state the headline's last timed tick left as DIR/<name>.npy (pos, quat, lvel, avel)")
    return ap.parse_args()


# ------------------------------------------------------------------------------------------------------------
# N > 1 from a plain invocation: the parent spawns the ranks and never touches the GPU itself
# ------------------------------------------------------------------------------------------------------------
def spawn_ranks(n):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, os.path.abspath(__file__)] + sys.argv[1:]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE if r == 0 else sys.stderr, text=(r == 0)))
    rc = 0
    live = set(range(n))
    while live and rc == 0:
        time.sleep(0.1)
        for r in sorted(live):
            code = procs[r].poll()
            if code is None:
                continue
            live.discard(r)
            if code != 0:
                print(f"bench.py: rank {r} exited with code {code}; stopping the other ranks", file=sys.stderr, flush=True)
                rc = code if code > 0 else 1
    if rc != 0:
        for r in live:                      # exactly the children started above
            procs[r].terminate()
        deadline = time.time() + 10
        for r in live:
            try:
                procs[r].wait(timeout=max(0.1, deadline - time.time()))
            except subprocess.TimeoutExpired:
                procs[r].kill()
        return rc
    out = procs[0].stdout.read()
    lines = [ln for ln in out.splitlines() if ln.strip().startswith("{")]
    if not lines:
        print("bench.py: rank 0 printed no JSON line", file=sys.stderr)
        return 1
    print(lines[-1], flush=True)
    return 0


# ------------------------------------------------------------------------------------------------------------
# committed rocprofv3 evidence for the kernel being timed (profiles/), tied to the kernel source it was measured on
# ------------------------------------------------------------------------------------------------------------
def kernel_source_id():
    """git blob hash (sha1 of 'blob <len>\\0' + bytes) of csrc/dmx_kernels.hip: what `git hash-object` prints"""
    data = open(os.path.join(ROOT, "rl-ode-physics_amd", "csrc", "dmx_kernels.hip"), "rb").read()
    return hashlib.sha1(b"blob %d\0" % len(data) + data).hexdigest()


def profile_evidence(kind, dtype, n):
    """(traffic bytes per launch, rocprof average kernel us, note) from profiles/hbm_pmc_<kind>_<dtype>_<n>.json --
    refused (None, None, why) when the file was measured on another version of dmx_kernels.hip"""
    path = os.path.join(ROOT, "profiles", f"hbm_pmc_{kind}_{dtype}_{n}.json")
    try:
        o = json.load(open(path))
    except (OSError, ValueError):
        # no counter pass for this workload: name the committed kernel-trace summary of the same command, if there is one
        trace = {"convex": "r04_c5_f32_kernel_stats.csv", "small": "r03_config1_trace.txt", "plane": "r04_c3_f32_kernel_stats.csv"}.get(kind)
        if trace and dtype == "f32" and os.path.exists(os.path.join(ROOT, "profiles", trace)):
            return None, None, f"profiles/{trace} (kernel trace; no PMC pass committed for this workload)"
        return None, None, "no PMC pass committed for this workload"
    have, want = o.get("kernels_blob"), kernel_source_id()
    if have != want:
        return None, None, f"stale: measured on dmx_kernels.hip {str(have)[:12]}, this build is {want[:12]}"
    return (o.get("traffic_bytes_per_launch"), o.get("rocprof_kernel_us"),
            f"profiles/{os.path.basename(path)} (rocprofv3 passes over this command on this kernel source, committed with the repository: another "
            f"run, possibly another box -- `stream_us_per_launch` is this run's own figure, boxes differ by a few per cent)")


# ------------------------------------------------------------------------------------------------------------
# CPU baseline: the oracle (the checker) timed on the host cores
# ------------------------------------------------------------------------------------------------------------
def cpu_baseline(scene, dtype, kind, budget_s):
    """Time the CPU oracle (oracle/, the checker) on a bounded sample of the same workload."""
    from oracle.orc_ctypes import Oracle
    orc = Oracle(dtype)
    ow = orc.world()
    if scene.plane is not None:
        ow.add_plane(*scene.plane)
    if scene.hull_points is not None:
        ow.set_hull(scene.hull_points)
        ow.add_convex(scene.pos, scene.quat, scene.lvel, scene.avel, scene.mass[:, 0], scene.inertia)
    else:
        ow.add_boxes(scene.pos, scene.quat, scene.lvel, scene.avel, scene.mass[:, 0], scene.inertia, scene.sides)
    t = ow.run(H, 2)                                   # probe
    steps = int(max(2, min(2000, budget_s / max(t / 2, 1e-9))))
    t = ow.run(H, steps)
    import ctypes.util
    have_ode = ctypes.util.find_library("ode") is not None      # say whether genuine ODE is on this host (it is never faked)
    return {"value": scene.n * steps / t, "unit": "body-steps/s", "cores": 1, "kind": "port",
            "sample": f"{scene.n} bodies x {steps} steps of the same scene ({kind}), oracle/ C restatement "
                      f"-O2 single thread, {t:.1f} s",
            "system_libode": have_ode}


def config_cpu_baseline(pkg, build_config, cfg, dtype, budget_s):
    """cpu_baseline of one `configs` leg: the oracle on a BOUNDED sample of the same workload -- the same scene builder at a
    smaller grid side where the full size would take minutes on one core (islands are independent: a block of the grid is
    the same per-body work), settled by the same number of ticks, then timed."""
    from oracle.orc_ctypes import Oracle
    side = {1: 32, 3: 128, 5: 16}[cfg]
    sc, _lay, kd, _wl, settle, stp, _hp = build_config(cfg, side)
    ow = Oracle(dtype).world()
    if sc.plane is not None:
        ow.add_plane(*sc.plane)
    if sc.hull_points is not None:
        ow.set_hull(sc.hull_points)
        if sc.hull_planes is not None:
            ow.set_hull_faces(sc.hull_planes)
    for sides, pos, R12 in (sc.static_boxes or []):
        ow.add_static_box(sides, pos, R12)
    if sc.hull_points is not None:
        ow.add_convex(sc.pos, sc.quat, sc.lvel, sc.avel, sc.mass[:, 0], sc.inertia)
    else:
        ow.add_boxes(sc.pos, sc.quat, sc.lvel, sc.avel, sc.mass[:, 0], sc.inertia, sc.sides)
    if settle:
        ow.run(H, settle)
    if stp:                                   # configs[0]: the workload IS these ticks from the start state
        steps = stp
    else:
        t = ow.run(H, 2)
        steps = int(max(2, min(400, budget_s / max(t / 2, 1e-9))))
    t = ow.run(H, steps)
    ow.close()
    return {"value": sc.n * steps / t, "unit": "body-steps/s", "ms_per_step": t * 1e3 / steps, "cores": 1, "kind": "port",
            "sample": f"{sc.n} bodies (grid side {side}) of the same scene builder, {settle} settling ticks, then {steps} timed ticks; oracle/ C "
                      f"restatement -O2 single thread, {t:.1f} s; body-steps/s is per body, so the sample's rate is the full scene's on one core"}


def cpu_baseline_all_cores(scene, dtype, kind, budget_s):
    """The same oracle, one independent slice of the scene per host core (islands are independent), one child
    process per core (oracle/cpu_worker.py); None if a child fails or overruns."""
    import tempfile
    import numpy as np
    cores = max(1, min(os.cpu_count() or 1, 64))
    per = scene.n // cores
    plane = np.array(scene.plane if scene.plane is not None else [], dtype=np.float64)
    with tempfile.TemporaryDirectory() as tmp:
        procs = []
        for c in range(cores):
            sl = slice(c * per, (c + 1) * per)
            path = os.path.join(tmp, f"slice{c}.npz")
            np.savez(path, pos=scene.pos[sl], quat=scene.quat[sl], lvel=scene.lvel[sl], avel=scene.avel[sl],
                     mass=scene.mass[sl, 0], inertia=scene.inertia[sl], sides=scene.sides[sl], plane=plane,
                     hull=scene.hull_points if scene.hull_points is not None else np.zeros((0, 3)))
            procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "oracle", "cpu_worker.py"), path, dtype,
                                           str(budget_s)], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True))
        rate = 0.0
        for p in procs:
            try:
                out, _ = p.communicate(timeout=5 * budget_s + 90)
                n, t = out.split()
                rate += float(n) / float(t)
            except Exception:      # noqa: BLE001 -- a baseline line must never take the bench down
                for q in procs:
                    if q.poll() is None:
                        q.kill()
                return None
    return {"value": rate, "unit": "body-steps/s", "cores": cores, "kind": "port",
            "sample": f"{cores} processes x {per} bodies of the same scene ({kind}), each the single-thread oracle for "
                      f"~{budget_s:.0f} s; rates summed"}


# ------------------------------------------------------------------------------------------------------------
# the reference's own tick through the ODE API: dSpaceCollide + dWorldStep(1/120) + dJointGroupEmpty (main.c:211-215)
# ------------------------------------------------------------------------------------------------------------
MATRIX_PEAK_TFLOPS = {"f32": 157.3, "f64": 78.6}     # MI355X_MICROARCH.md: f32-input MFMA = the f32 vector rate; FP64 matrix (spec)


def scene_text(dt, steps, statics, bodies):
    """the stdin of tests/harness/ode_tick_harness.c: dt steps use_plane / static boxes / bodies"""
    ident = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]
    lines = [f"{dt!r} {steps} 0", str(len(statics))]
    for size, pos, R in statics:
        lines.append(" ".join(repr(float(v)) for v in (*size, *pos, *R)))
    lines.append(str(len(bodies)))
    for kind, size, pos in bodies:
        lines.append(f"{kind} " + " ".join(repr(float(v)) for v in (*size, *pos, *ident)))
    return "\n".join(lines) + "\n"


def reference_main_c(pkg, dtype, cpu_budget_s, with_cpu=True):
    """The call the reference actually makes -- dWorldStep at h = 1/120 (main.c:208,213) -- through the ODE C API, from a C
    program that makes main.c's own sequence of calls (tests/harness/ode_tick_harness.c: it is compiled here against
    include/ode/ode.h and linked against the shipped library): the reference's floor and walls, 48 / 200 / 512 of the key-M
    spawner's boxes and spheres (512 = MAX_BODIES, inc/body.h:6), QuickStep while they come down, then dWorldStep for the timed
    ticks (wall time of dSpaceCollide + dWorldStep + dJointGroupEmpty + one pose read per tick, host included).  cpu_baseline:
    the oracle's exact stepper on the same scene from the same settled state."""
    import re
    import tempfile
    single = dtype == "float32"
    tag = "f32" if single else "f64"
    pkg_dir = os.path.join(ROOT, "rl-ode-physics_amd")
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "ode_tick_harness")
    cmd = ["gcc", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "harness", "ode_tick_harness.c"), "-o", exe,
           "-L" + pkg_dir, "-lode_mi355_single" if single else "-lode_mi355", "-Wl,-rpath," + pkg_dir, "-lm"]
    if single:
        cmd.insert(1, "-DdSINGLE")
    subprocess.run(cmd, check=True)
    out = {"call_sequence": "dSpaceCollide(space, 0, NearCallback) -> dWorldStep(world, 1/120) -> dJointGroupEmpty (main.c:211-215), "
                            "contact policy of main.c:674-693 (<= 8 contacts, bounce 0.2, mu = inf), through include/ode/ode.h from C",
           "dtype": tag, "dt": "1/120"}
    statics = pkg.scenes.reference_map()
    settle, ticks = 900, 60
    for n in (48, 200, 512):
        bodies = pkg.scenes.reference_spawn(n, seed=7, y_range=(1.2, 12.0))
        env = dict(os.environ, HARNESS_STEPPER="exact", HARNESS_EXACT_AFTER=str(settle), HARNESS_TIME_FROM=str(settle + 4), DMX_LCP_REPORT="1")
        p = subprocess.run([exe], input=scene_text(1.0 / 120.0, settle + ticks, statics, bodies), capture_output=True, text=True, env=env, timeout=600)
        leg = {"bodies": n}
        t = re.search(r"harness: timed_ticks=(\d+) ms_per_tick=([0-9.]+) collide_ms=([0-9.]+) step_ms=([0-9.]+)", p.stderr)
        if p.returncode != 0 or not t:
            leg["error"] = p.stderr[-400:]
            out[f"{n}_bodies"] = leg
            continue
        ms = float(t.group(2))
        leg.update({"ms_per_step": ms, "value": n / (ms * 1e-3), "unit": "body-steps/s", "steps": int(t.group(1)),
                    "collide_ms": float(t.group(3)), "step_ms": float(t.group(4)), "frame_budget_ms": 1e3 / 120.0})
        g = re.search(r"lcp grid: solves=(\d+) rounds=(\d+) max_rounds=(\d+) last_m=(\d+) last_nu=(\d+) last_nbd=(\d+) single=(\d+) "
                      r"fallback=(\d+) gflop=([0-9.]+)", p.stderr)
        if g:
            gf_tick = float(g.group(9)) / ticks
            leg["grid_solve"] = {"island_solves": int(g.group(1)), "pivoting_rounds": int(g.group(2)), "most_rounds_in_one_solve": int(g.group(3)),
                                 "last_island_rows": int(g.group(4)), "never_clamping_rows": int(g.group(5)), "bounded_rows": int(g.group(6)),
                                 "single_flip_rounds": int(g.group(7)), "gflop_per_tick": gf_tick}
            leg["roofline"] = {"bound": "mfma", "achieved": gf_tick / (float(t.group(4)) * 1e-3) * 1e-3, "peak": MATRIX_PEAK_TFLOPS[tag],
                               "unit": "TFLOP/s", "frac": gf_tick / (float(t.group(4)) * 1e-3) * 1e-3 / MATRIX_PEAK_TFLOPS[tag], "traffic": None,
                               "kernel": "lcp_panel + lcp_syrk (csrc/dmx_lcp.hip)",
                               "note": "algorithmic flops of the tick's factorisations (nu^3/3 + nu^2 nb + nu nb^2 once, nf^3/3 per pivoting "
                                       "round) over the wall time of the dWorldStep call: the solve is a chain of 64-wide panels, each one "
                                       "launch of a serial 64-pivot factorisation and one of matrix-core updates -- latency of the chain, "
                                       "not the matrix cores' rate, bounds it (profiles/r04_lcp_*)"}
        else:
            leg["grid_solve"] = None          # no island reached DMX_LCP_GRID_ROWS: every island was one workgroup's (lcp_island_wg)
        if with_cpu:
            try:
                from oracle.orc_ctypes import Oracle
                ow = Oracle(dtype).world()
                ow.add_reference_scene(statics, bodies)
                ow.set_stepper(False)
                ow.run(1.0 / 120.0, settle)
                ow.set_stepper(True)
                t1 = ow.run(1.0 / 120.0, 1)
                k = int(max(1, min(ticks - 1, cpu_budget_s / max(t1, 1e-6))))
                tk = ow.run(1.0 / 120.0, k)
                leg["cpu_baseline"] = {"value": n * k / tk, "unit": "body-steps/s", "ms_per_step": tk * 1e3 / k, "cores": 1, "kind": "port",
                                       "sample": f"the same {n} bodies settled by {settle} QuickStep ticks, then {k} ticks of the oracle's exact "
                                                 f"stepper (oracle/ C restatement, -O2, single thread), {tk:.2f} s"}
                ow.close()
            except Exception as e:      # noqa: BLE001
                leg["cpu_baseline"] = {"error": f"{type(e).__name__}: {e}"}
        out[f"{n}_bodies"] = leg
    return out


# ------------------------------------------------------------------------------------------------------------
# one rank
# ------------------------------------------------------------------------------------------------------------
class Ctx:
    """what every measurement of this process shares: package, torch, the process group, the launch stream"""


def tile_scene(np, base, reps_x):
    """`reps_x` copies of a grid scene side by side along x (the 16 Mi-body size without 117 M PRNG draws)"""
    if reps_x == 1:
        return base
    span = (base.pos[:, 0].max() - base.pos[:, 0].min()) + 2.5
    cat = lambda a: np.concatenate([a] * reps_x, axis=0)
    pos = cat(base.pos)
    pos[:, 0] += np.repeat(np.arange(reps_x, dtype=pos.dtype) * span, base.n)
    return type(base)(pos, cat(base.quat), cat(base.lvel), cat(base.avel), cat(base.mass), cat(base.inertia), cat(base.sides),
                      np.concatenate([base.gtype] * reps_x), base.plane, base.hull_points)


def measure(cx, a, scene, layout, kind, dtype, *, exchanging, every_tick=False, ticks_per_launch=1, settle_steps=0,
            steps=None, warmup=None, setup=None, one_block=False, dump=None):
    """Build the batch and the tick loop for `scene`, warm up, time blocks of `steps` ticks.  Any failure raises: a run
    that could not exchange is no run (there is no substitute path).  `dump(w, n_own)`, if given, is called once the
    timed ticks are settled, before the batch is freed."""
    torch, dist, pkg, np = cx.torch, cx.dist, cx.pkg, cx.np
    steps = a.steps if steps is None else steps
    warmup = a.warmup if warmup is None else warmup
    w = pkg.BatchWorld(layout.n_total if exchanging else scene.n, dtype=dtype, device=cx.device_index)
    st = None
    try:
        w.load_scene(scene)
        if exchanging:
            w.set_active_count(layout.n_active)     # the slots behind are ghosts of the neighbours' boundary rows
        w.set_gyro_mode(a.gyro)
        if setup is not None:
            setup(w)
        if ticks_per_launch > 1:
            w.set_ticks_per_launch(ticks_per_launch)
        collide = not a.no_body_collisions
        if not collide:
            w.set_body_collisions(False)
        w.set_stream(cx.stream.cuda_stream)
        c_loop = exchanging and not every_tick          # the sharded loop behind the C ABI (include/dmx_shard.h): the product path
        if c_loop:
            # collectives: the library's own RCCL binding (ncclAllGather on its side stream), or -- ranks sharing one GPU, which
            # RCCL does not allow -- callbacks that stage through host memory over the gloo group (REHEARSAL, flagged in `data`)
            # Should the library's communicator fail to come up on ANY rank (this path has never run on more than one GPU before the
            # driver's own run), every rank falls back on the torch.distributed exchange below -- same kernels, same loop in
            # Python -- and the line says so (`c_loop_error`): a scaling run without a number helps nobody.
            err = None
            try:
                st = pkg.shard.CShardedStepper(w, layout, cx.rank, cx.world, collectives="staged" if cx.rehearse else "rccl")
            except Exception as e:      # noqa: BLE001
                err = f"{type(e).__name__}: {e}"
            if cx.world > 1:
                flag = torch.tensor([0 if err is None else 1], dtype=torch.int32, device=cx.device if dist.get_backend() == "nccl" else "cpu")
                dist.all_reduce(flag, op=dist.ReduceOp.MAX)
                failed = int(flag.item()) != 0
            else:
                failed = err is not None
            if failed:
                if st is not None:
                    st.close()
                    st = None
                c_loop = False
                cx.c_loop_error = err or "another rank's communicator did not come up"
        rccl_info = None
        if exchanging and cx.world > 1:
            # what produced this run's collectives, rank by rank, in the log and in the JSON line: the library's own librccl (path,
            # communicator up) or the fallback
            mine = {"rank": cx.rank, "c_loop": bool(c_loop), "collectives": "staged (rehearsal)" if cx.rehearse else "rccl"}
            if c_loop and not cx.rehearse:
                try:
                    mine.update(st.rccl_info())
                except Exception as e:      # noqa: BLE001
                    mine["error"] = f"{type(e).__name__}: {e}"
            print(f"[bench rank {cx.rank}] shard loop: {mine}", file=sys.stderr, flush=True)
            rccl_info = [None] * cx.world
            dist.all_gather_object(rccl_info, mine)
        if not c_loop:
            ops = None
            if exchanging and cx.rehearse:
                ops = pkg.shard.StagedDeviceOps(w, cx.device, cx.stream)
            elif exchanging and cx.world == 1:
                ops = pkg.shard.DeviceOps(w, cx.device, cx.stream)      # --force-exchange: the collective degenerates to a copy
            st = pkg.shard.ShardedStepper(w, layout, cx.rank, cx.world, exchange="boundary" if exchanging else "none",
                                          device=cx.device, stream=cx.stream, collide=collide and exchanging,
                                          geometry=(scene.sides, scene.gtype, scene.mass[:, 0], scene.inertia), ops=ops,
                                          exchange_every_tick=every_tick,
                                          lazy=True)
        if settle_steps:
            st.run(H, settle_steps)             # let the bodies land: timed steps are all in contact
        st.run(H, warmup)
        graphed = False
        if not c_loop and st.exchange is not None and every_tick and a.graph_steps > 0:
            torch.cuda.synchronize()
            graphed = st.capture(H, a.graph_steps, cx.stream)
            st.run(H, a.graph_steps)            # one replay outside the timed region

        def block():
            cx.barrier()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(cx.stream)
            st.run(H, steps)
            e1.record(cx.stream)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            cx.barrier()
            return dt, e0.elapsed_time(e1) * 1e-3

        def exchanges():
            if c_loop:
                return st.stats()["exchanges"]
            return st.exchange.count if st.exchange is not None else 0
        ex0 = exchanges()
        first = block()
        est = cx.max_over_ranks([first[0]])[0]
        # (one_block: the workload is these ticks from this start state and no others -- configs[0]; a second block would time
        #  the settled scene that follows)
        nblocks = 1 if (one_block or est >= MIN_REGION_S) else min(MAX_BLOCKS, int(math.ceil(MIN_REGION_S / max(est, 1e-6))) | 1)
        blocks = [first] + [block() for _ in range(nblocks - 1)]
        t_close = time.perf_counter()
        if c_loop:
            st.settle()                         # the chunk the loop may have left open: validated before anything is reported
        else:
            st.close()
        torch.cuda.synchronize()
        t_close = cx.max_over_ranks([time.perf_counter() - t_close])[0]
        if dump is not None:
            dump(w, layout.n_active if exchanging else scene.n)
        n_ex = exchanges() - ex0
        if graphed:
            n_ex = nblocks * steps              # a captured graph counts its exchanges once, at capture
        wall = cx.max_over_ranks([b[0] for b in blocks])
        dev = [b[1] for b in blocks]
        dt = statistics.median(wall)
        stats = w.collision_stats()
        contacts = w.last_contact_count() if kind != "free" else 0
        # every timed tick and every chunk close, the last one included: total wall time over total ticks
        mean_dt = (sum(wall) + t_close) / nblocks
        return {"dt": dt, "mean_dt": mean_dt, "contacts": contacts,
                "dev_s": statistics.median(dev), "blocks": nblocks, "wall_min": min(wall), "wall_max": max(wall),
                "steps": steps, "n_exchanges": n_ex, "ticks_timed": nblocks * steps, "graphed": graphed, "stats": stats,
                "exchanging": c_loop or st.exchange is not None, "tpl": ticks_per_launch if kind == "free" else 1,
                "bodies": scene.n, "c_loop": c_loop, "c_loop_error": getattr(cx, "c_loop_error", None), "rccl_per_rank": rccl_info}
    finally:
        if st is not None and getattr(st, "exchange", None) is not None and st.exchange.fused:
            st.exchange.ops.disarm_pack()       # the send buffers die with the stepper: the batch must not keep aiming at them
        if st is not None and isinstance(st, pkg.shard.CShardedStepper):
            try:
                st.close()                      # (dmxShardDestroy detaches the batch from its send buffers)
            except Exception:       # noqa: BLE001 -- a failed run is already on its way out
                pass
        w.close()


def roofline_of(m, kind, rsize, evidence=None, hull_points=0):
    """the bound of the kind's dominant kernel: HBM bytes for the contact-free pass, vector flops for the fused contact kernels,
    latency (no fraction to quote: launches and dependency chains) for the small exact-tick scene"""
    tpl = m["tpl"]
    stream_s = m["dev_s"] / m["steps"] * tpl                 # stream time per launch: HIP events on the launch stream / launches
    alg_bytes = BYTES_PER_BODY_STEP[kind] * rsize * m["bodies"] * tpl
    gbs = alg_bytes / stream_s / 1e9
    bound = BOUND_OF[kind]
    r = {"bound": bound, "kernel": KERNEL_OF[kind], "per": "GPU (one rank's launches over one rank's bodies)",
         "stream_us_per_launch": stream_s * 1e6, "ticks_per_launch": tpl, "traffic": None}
    if bound == "hbm":
        r.update({"achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
                  "algorithmic_bytes_per_body_step": BYTES_PER_BODY_STEP[kind] * rsize,
                  # measured ceiling for this access pattern (a compute-free kernel, same reads and writes, non-zero slab contents;
                  # f32, 1 Mi bodies -- a static reference from profiles/, NOT measured by this run)
                  "bare_pattern_frac_reference": {"frac": 0.82, "plain_copy_frac": 0.84,
                                                  "evidence": "profiles/r03_ubench_fill_effect.txt"}})
    elif bound == "valu":
        rows = 3 * m["contacts"]
        flops = 20 * rows * SOR_FLOP_PER_ROW_SWEEP + m["bodies"] * hull_points * HULL_FLOP_PER_POINT
        peak = VALU_PEAK_TFLOPS * (1.0 if rsize == 4 else 0.5)
        tf = flops / stream_s / 1e12
        r.update({"achieved": tf, "peak": peak, "unit": "TFLOP/s", "frac": tf / peak,
                  "algorithmic_flops_per_tick": flops,
                  "flops_note": f"20 sweeps x {rows} rows ({m['contacts']} contacts x 3) x {SOR_FLOP_PER_ROW_SWEEP} flop (SURVEY 8d)"
                                + (f" + {hull_points} hull points x {HULL_FLOP_PER_POINT} flop per hull" if hull_points else ""),
                  "hbm_GBps_for_reference": gbs})
    else:
        r.update({"achieved": None, "peak": None, "unit": "us/tick", "frac": None,
                  "us_per_tick": m["dt"] / m["steps"] * 1e6,
                  "note": "a scene this small is launches and dependency chains: no bandwidth or flop fraction means anything; "
                          "see exact_ticks / fast_ticks and the kernel trace named in `evidence`"})
    if evidence is not None:
        traffic, k_us, note = evidence
        r["traffic"] = traffic
        r["rocprof_kernel_us"] = k_us
        r["evidence"] = note
    return r


def collide_text(m, a, kind):
    s = m["stats"]
    if a.no_body_collisions:
        t = "body-body contacts: none by assertion (check off)"
    else:
        t = (f"body-body contacts proven absent by broadphase safe zones (bounding spheres never touch, so no collider can return a "
             f"contact; AABB pairs are not enumerated on this path): {s['fast_ticks']} fast ticks, {s['careful_ticks']} exact-search "
             f"ticks, {s['rebuilds']} zone rebuilds, {s['pair_ticks']} ticks with AABB pairs")
    if kind == "plane":
        t += "; ground plane fused into the step kernel"
    if kind == "convex":
        t += ("; hull against the static floor box: one wavefront per hull (np_convex_static: vertices in the box, corners in the hull), "
              "then the fused solve with 8 contact slots in registers (step_contacts)")
    if kind == "small":
        t += "; ground plane fused into the step kernel; exact ticks run pair search, box-box narrowphase, islands and level-scheduled sweeps on the device"
    return t


def rank_main(a):
    # stdout carries exactly one line, the JSON: native libraries print banners there (RCCL's version block at
    # communicator set-up), so fd 1 points at stderr until the result is ready
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        if rank == 0:
            print(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={world}", file=sys.stderr)
        sys.exit(2)

    import numpy as np
    import torch
    import torch.distributed as dist
    from __graft_entry__ import load_package
    pkg = load_package()

    ndev = torch.cuda.device_count()            # (counting devices does not initialise the GPU)
    if ndev < 1:
        print("bench.py: no GPU visible; the HIP path has no CPU fallback", file=sys.stderr)
        sys.exit(1)
    cx = Ctx()
    cx.torch, cx.dist, cx.pkg, cx.np = torch, dist, pkg, np
    cx.rank, cx.world = rank, world
    cx.rehearse = world > 1 and (a.rehearse_on_one_gpu or ndev < world)
    if cx.rehearse and world > 6:
        print(f"bench.py: {world} ranks cannot share {ndev} GPU(s) (at most 6 processes per card on this pool)", file=sys.stderr)
        sys.exit(2)
    cx.device_index = 0 if cx.rehearse else local_rank
    cx.device = torch.device("cuda", cx.device_index)
    torch.cuda.set_device(cx.device_index)
    backend = None
    if world > 1 or a.force_exchange:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        import datetime
        if cx.rehearse:
            backend = "gloo"
            dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(minutes=5))
        else:
            backend = "nccl"
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=cx.device,
                                    timeout=datetime.timedelta(minutes=5))      # a wedged collective fails the run instead of hanging it
    cx.stream = torch.cuda.Stream()             # a real (non-null) stream: the batch launches on it and the timing
    torch.cuda.set_stream(cx.stream)            # events are recorded on it, so they bracket the kernels
    assert cx.stream.cuda_stream != 0

    def barrier():
        if world > 1:
            dist.barrier()

    def max_over_ranks(vals):
        if world == 1:
            return list(vals)
        t = torch.tensor(list(vals), dtype=torch.float64, device="cpu" if cx.rehearse else cx.device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return t.tolist()
    cx.barrier, cx.max_over_ranks = barrier, max_over_ranks

    dtype = "float32" if a.dtype == "f32" else "float64"
    rsize = np.dtype(dtype).itemsize
    config = a.config or (4 if world > 1 else 2)
    use_exchange = (world > 1 or a.force_exchange) and a.exchange == "boundary"

    def build_config(config, side_arg):
        """(scene, layout, kind, workload text, settle ticks, steps override, hull points) of BASELINE.json configs[config - 1]"""
        steps_override = None
        hull_points = 0
        settle = 0
        if config == 4:
            # configs[3] as BASELINE states it: the configs[1] scene (1 048 576 bodies) in `world` disjoint slabs, 10 m apart
            side = side_arg or 1024
            assert side % world == 0 and (side // world) >= 2, "the grid's rows must split evenly over the ranks"
            rows = side // world
            kind = "free"
            full = pkg.scenes.box_grid(side, side, seed=1, spin=True, plane=False, slabs=world, slab_gap=10.0)
            scene = full.slice(rank * side * rows, (rank + 1) * side * rows).astype(dtype)
            layout = pkg.shard.SlabLayout(side, rows)
            workload = (f"configs[3]: {side * side} free-falling boxes in {world} disjoint slabs >= 10 m apart, one slab of "
                        f"{side * rows} bodies per GPU, no contacts, dt=1/60")
        elif config == 2:
            side = side_arg or 1024
            kind = "free"
            scene = pkg.scenes.box_grid(side, side, seed=1 + rank, spin=True, plane=False).astype(dtype)
            scene.pos[:, 2] += rank * (side * pkg.scenes.PITCH + 10.0)
            layout = pkg.shard.SlabLayout(side, side)
            workload = f"configs[1]: {side * side} free-falling boxes per GPU, no contacts, dt=1/60"
        elif config == 5:
            side = side_arg or 128
            kind = "convex"
            workload = (f"configs[4]: {side * side} convex hulls of res/teapot.obj (1 265 points, 2 526 faces, scale 0.01) per GPU resting on a "
                        f"static box floor (the reference's floor is one, main.c:115): box-trimesh contacts (<= 8 per hull) and those only, as "
                        f"BASELINE names them -- the hull geoms' collide bits name the map, not one another (dGeomSetCollideBits, main.c:725: "
                        f"dmxBatchSetClassPairs(CONVEX, CONVEX, 0)); 20 SOR iterations, dt=1/60.  The same scene with the teapots colliding "
                        f"with one another too (hull-hull collider; tipped teapots roll into their neighbours) is `hull_pairs_on`")
            gold = np.load(os.path.join(ROOT, "tests", "golden", "teapot_hull.npz"))     # the hull's vertices (data fixture)
            hull = pkg.hull.build(gold["points"], 0.01)
            hull_points = int(hull.points.shape[0])
            scene = pkg.scenes.hull_grid(hull, side, side, seed=1 + rank, y_range=(0.6, 1.6), spin=False, tilt=0.2, floor_box=True).astype(dtype)
            scene.pos[:, 2] += rank * (side * pkg.scenes.HULL_PITCH + 10.0)
            layout = pkg.shard.SlabLayout(side, side)
            settle = 120
        elif config == 1:
            side = side_arg or 32
            kind = "small"
            steps_override = 600
            workload = (f"configs[0]: {side * side} free-falling boxes over a ground plane through the batch path, 600 ticks from the "
                        f"start state (they land from tick ~120 on, neighbours meet from ~340 on: box-plane and box-box contacts)")
            scene = pkg.scenes.box_grid(side, side, seed=1, spin=False, plane=True).astype(dtype)
            layout = pkg.shard.SlabLayout(side, side)
        else:
            side = side_arg or 512
            kind = "plane"
            workload = f"configs[2]: {side * side} boxes on the ground plane per GPU, 20 SOR iterations, dt=1/60"
            scene = pkg.scenes.box_grid(side, side, seed=1 + rank, y_range=(1.0, 3.0), spin=False, plane=True).astype(dtype)
            scene.pos[:, 2] += rank * (side * pkg.scenes.PITCH + 10.0)
            layout = pkg.shard.SlabLayout(side, side)
            settle = 120
        return scene, layout, kind, workload, settle, steps_override, hull_points

    scaling = "strong" if config == 4 else "weak"
    scene, layout, kind, workload, settle, steps_override, hull_points = build_config(config, a.side)
    side = layout.side

    if kind == "small":       # (configs[0] as the headline: the throw-away pass config_leg describes)
        measure(cx, a, scene, layout, kind, dtype, exchanging=False, settle_steps=settle, steps=steps_override, warmup=10, one_block=True)
    dumped = {}

    def keep_state(w, n_own):
        """the arrays a caller of the tick loop receives: the bodies' state after the last timed tick (a seeded sample when large)"""
        budget = DUMP_BYTES // world
        rows = budget // (13 * rsize)                       # pos 3 + quat 4 + lvel 3 + avel 3 reals per body
        idx = None if n_own <= rows else np.sort(np.random.default_rng(DUMP_SEED).choice(n_own, rows, replace=False))
        for name, field in (("pos", pkg.batch.POS), ("quat", pkg.batch.QUAT), ("lvel", pkg.batch.LVEL), ("avel", pkg.batch.AVEL)):
            arr = w.download(field, 0, n_own)
            dumped[name] = arr if idx is None else arr[idx]

    # the headline: exactly --steps timed ticks in one block (configs[0]: its 600 ticks from the start state)
    head = measure(cx, a, scene, layout, kind, dtype, exchanging=use_exchange, every_tick=a.exchange_every_tick,
                   ticks_per_launch=a.ticks_per_launch if kind == "free" else 1, settle_steps=settle, steps=steps_override,
                   warmup=10 if steps_override else None, one_block=True,
                   setup=(lambda w: w.set_class_pairs(pkg.scenes.GEOM_CONVEX, pkg.scenes.GEOM_CONVEX, False)) if kind == "convex" else None,
                   dump=keep_state if a.dump_outputs else None)
    if a.dump_outputs:
        os.makedirs(a.dump_outputs, exist_ok=True)
        prefix = f"rank{rank}_" if world > 1 else ""
        for name, arr in dumped.items():
            np.save(os.path.join(a.dump_outputs, f"{prefix}{name}.npy"), arr)

    def parallelism_text(m, bodies_per_gpu):
        if not m["exchanging"]:
            return f"islands sharded over {world} GPU(s), one slab per rank; no exchange" + (" (one rank)" if world == 1 else " (--exchange none)")
        every = m["n_exchanges"] >= m["ticks_timed"]
        loop = ("the rank loop behind the C ABI (dmxShardRun, include/dmx_shard.h) with " +
                ("its own RCCL communicator (ncclAllGather on the side stream, ncclAllReduce for the chunk flags)" if backend == "nccl"
                 else "collectives injected as host-staged callbacks: REHEARSAL")) if m.get("c_loop") else \
               f"the Python rank loop (rl-ode-physics_amd/shard.py) over torch.distributed backend {backend}"
        return (f"islands sharded over {world} GPU(s), one slab of {bodies_per_gpu} bodies per rank; {loop}; process group backend "
                f"{backend} ({'RCCL over xGMI' if backend == 'nccl' else 'gloo, staged through host memory: REHEARSAL'}), world size "
                f"{dist.get_world_size()}; boundary rows (2 x {layout.side} bodies x 13 reals per rank) all-gathered on a side stream"
                f"{', HIP-graph replay' if m['graphed'] else ''}: {m['n_exchanges']} exchanges issued in the {m['ticks_timed']} timed ticks "
                f"({'every tick' if every else 'at the end of every collision-proof chunk: inside a ballistic chunk nothing reads the ghost rows'})")

    total_bodies = scene.n * world
    data = "synthetic"
    if cx.rehearse:
        data += " (REHEARSAL: all ranks on one GPU, collectives staged through host memory; not a measurement)"
    out = {
        "metric": "body-steps/sec at 1M rigid bodies, dt=1/60",
        "value": total_bodies * head["steps"] / head["dt"], "unit": "body-steps/s", "n_gpus": world, "steps": a.steps,
        "warmup": a.warmup, "ms_per_step": head["dt"] * 1e3 / head["steps"], "higher_is_better": True, "scaling": scaling,
        "vs_baseline": None, "dtype": a.dtype, "data": data,
        "timing": {"blocks": head["blocks"], "block_ms_median": head["dt"] * 1e3, "block_ms_min": head["wall_min"] * 1e3,
                   "block_ms_max": head["wall_max"] * 1e3,
                   "note": "one block of exactly `steps` ticks, bracketed by barrier + synchronize"},
        "config": {"workload": workload, "bodies_per_gpu": scene.n, "bodies_total": total_bodies, "dt": "1/60",
                   "parallelism": parallelism_text(head, scene.n),
                   "collide": collide_text(head, a, kind),
                   "integrator": "QuickStep semantics: gravity + implicit gyroscopic torque + semi-implicit Euler + "
                                 "quaternion renormalise" + ("; box-plane contacts, 20 SOR sweeps" if kind == "plane" else "")
                                 + ("; box-convex contacts with the static floor box, 20 SOR sweeps" if kind == "convex" else "")
                                 + ("; box-plane and box-box contacts, 20 SOR sweeps" if kind == "small" else "")},
        "roofline": roofline_of(head, kind, rsize, profile_evidence(kind, a.dtype, scene.n), hull_points),
    }
    if head.get("rccl_per_rank"):
        out["config"]["shard_loop_per_rank"] = head["rccl_per_rank"]
    if head.get("c_loop_error"):
        out["config"]["c_loop_error"] = ("the rank loop behind the C ABI could not bring up its own RCCL communicator; this run used the same loop "
                                         "in Python over torch.distributed instead (that loop has no migration: it is valid for scenes without contacts across "
                                         "rank boundaries, which configs[3]'s disjoint slabs are -- an island reaching across two ranks raises there): "
                                         + str(head["c_loop_error"]))
    out["timing"]["ms_per_step_mean"] = head["mean_dt"] * 1e3 / head["steps"]
    out["timing"]["note"] += ("; ms_per_step_mean = (the block + the close of the last open chunk) / the timed ticks: every chunk close "
                              "(zone test, flag read) is in it")
    if world > 1 and config == 4:
        out["config"]["target_claim"] = (
            "north_star's >= 6x at 8 GPUs is judged on THIS line (value at N vs value at N = 1, both one launch per tick, ticks_per_launch 1). "
            "A 131 072-body slab is launch-bound (4.2 us per tick without, 4.7-4.8 us with the collision proof riding along, against "
            "19.5-19.9 us for the whole scene on one GPU; scripts/time_small_slab.py), so this line is expected near 4-4.5x; `fused.ticks_per_launch_2` is the same loop with two ticks per launch -- what the reference's own loop "
            "observes, since it reads poses every other physics tick (main.c:208, 218) -- and is the variant expected past 6x. Both are "
            "reported; neither is substituted for the other.")

    def hulls_map_only(w):
        w.set_class_pairs(pkg.scenes.GEOM_CONVEX, pkg.scenes.GEOM_CONVEX, False)

    def config_leg(cfg):
        """one BASELINE config timed beside the headline: a short leg of the same measure()"""
        sc, lay, kd, wl, stl, stp, hp = build_config(cfg, 0)
        cold = None
        if kd == "small":
            # configs[0] is ONE run of 600 ticks from the start state: its warm-up cannot be the run's first ticks (they are the
            # workload), so it is a throw-away pass over the same scene in a batch of its own -- the exact tick's kernels have been
            # launched once and the allocator's pools have grown when the timed pass begins.  The cold pass is reported beside it.
            cold = measure(cx, a, sc, lay, kd, dtype, exchanging=False, settle_steps=stl, steps=stp, warmup=10, one_block=True)
        m = measure(cx, a, sc, lay, kd, dtype, exchanging=False, settle_steps=stl, steps=stp or min(a.steps, 200),
                    warmup=10 if stp else min(a.warmup, 20), setup=hulls_map_only if kd == "convex" else None, one_block=kd == "small")
        leg = {"workload": wl, "bodies": sc.n, "dtype": a.dtype, "value": sc.n * m["steps"] / m["dt"], "unit": "body-steps/s",
               "ms_per_step": m["dt"] * 1e3 / m["steps"], "ms_per_step_mean": m["mean_dt"] * 1e3 / m["steps"], "steps": m["steps"],
               "blocks": m["blocks"], "contacts_last_tick": m["contacts"], "collide": collide_text(m, a, kd),
               "roofline": roofline_of(m, kd, rsize, profile_evidence(kd, a.dtype, sc.n), hp)}
        if cpu_baselines:
            try:
                leg["cpu_baseline"] = config_cpu_baseline(pkg, build_config, cfg, dtype, min(a.cpu_seconds, 3.0))
            except Exception as e:      # noqa: BLE001
                leg["cpu_baseline"] = {"error": f"{type(e).__name__}: {e}"}
        if cold is not None:
            leg["first_pass_in_the_process"] = {"ms_per_step": cold["dt"] * 1e3 / cold["steps"],
                                                "note": "the same 600 ticks the first time this process runs them: every kernel of the exact tick is "
                                                        "launched for the first time (code objects load lazily) and the batch's work arrays are allocated"}
        if kd == "convex":
            m2 = measure(cx, a, sc, lay, kd, dtype, exchanging=False, settle_steps=stl, steps=min(a.steps, 100), warmup=min(a.warmup, 20))
            leg["hull_pairs_on"] = {"ms_per_step": m2["dt"] * 1e3 / m2["steps"], "value": sc.n * m2["steps"] / m2["dt"], "unit": "body-steps/s",
                                    "contacts_last_tick": m2["contacts"], "collide": collide_text(m2, a, kd),
                                    "note": "every class collides with every class (the default): teapots that have rolled into one another "
                                            "are body pairs, every tick runs the pair search and the islands"}
        return leg

    extras = a.full and not a.no_extras          # a plain run is the headline and nothing else
    cpu_baselines = a.full and not a.no_cpu_baseline
    if extras and world == 1 and config == 2 and not a.side and not a.no_configs:
        # the other single-GPU BASELINE configs, each with the bound of ITS dominant kernel (configs[3] is the N > 1 headline)
        out["configs"] = {}
        for cfg in (1, 3, 5):
            try:
                out["configs"][f"configs[{cfg - 1}]"] = config_leg(cfg)
            except Exception as e:      # noqa: BLE001 -- a companion leg must not take the headline down; the failure is reported
                out["configs"][f"configs[{cfg - 1}]"] = {"error": f"{type(e).__name__}: {e}"}
        # ... and the reference's OWN scene, which BASELINE's configs do not name: its floor and three walls as static boxes
        # (main.c:115-121) and a pile of the key-M spawner's boxes and spheres (main.c:502-521) -- 400 bodies, and 512 = MAX_BODIES
        # (inc/body.h:6).  Once down the pile is ONE island: the tick is the exact pipeline + one workgroup's level-scheduled sweeps.
        out["reference_pen"] = {}
        for nb_pen in (400, 512):
            try:
                psc, pboxes, _ = pkg.scenes.reference_pen(nb_pen)
                psc = psc.astype(dtype)
                w = pkg.BatchWorld(psc.n, dtype=dtype, device=cx.device_index)
                try:
                    w.load_scene(psc); w.set_static_boxes(pboxes); w.set_gyro_mode(a.gyro)
                    w.step(H, 240); w.synchronize()             # the bodies are down (and the exact tick's kernels warm)
                    t0 = time.perf_counter(); w.step(H, 240); w.synchronize(); dtp = time.perf_counter() - t0
                    out["reference_pen"][f"{nb_pen}_bodies"] = {"ms_per_step": dtp * 1e3 / 240, "value": psc.n * 240 / dtp, "unit": "body-steps/s",
                                                                "steps": 240, "contacts_last_tick": int(w.last_contact_count()),
                                                                "collide": str(w.collision_stats())}
                finally:
                    w.close()
            except Exception as e:      # noqa: BLE001
                out["reference_pen"][f"{nb_pen}_bodies"] = {"error": f"{type(e).__name__}: {e}"}
        if cpu_baselines and "error" not in out["reference_pen"].get("400_bodies", {"error": 1}):
            try:        # the oracle on the same 400-body pile, same 240 settling ticks: one core
                from oracle.orc_ctypes import Oracle
                ow = Oracle(dtype).world()
                ow.add_reference_scene(pkg.scenes.reference_map(), sorted(pkg.scenes.reference_spawn(400, seed=7, y_range=(3.0, 12.0)), key=lambda s: -s[0]))
                ow.run(H, 240)
                tk = ow.run(H, 240)
                out["reference_pen"]["400_bodies"]["cpu_baseline"] = {
                    "value": 400 * 240 / tk, "unit": "body-steps/s", "ms_per_step": tk * 1e3 / 240, "cores": 1, "kind": "port",
                    "sample": f"the same 400 bodies and static boxes, 240 settling ticks, then 240 timed QuickStep ticks; oracle/ C restatement, {tk:.2f} s"}
                ow.close()
            except Exception as e:      # noqa: BLE001
                out["reference_pen"]["400_bodies"]["cpu_baseline"] = {"error": f"{type(e).__name__}: {e}"}
        # ... and the reference's own CALL: dWorldStep at 1/120 through the ODE API from C (main.c:211-215)
        try:
            out["reference_main_c"] = reference_main_c(pkg, dtype, min(a.cpu_seconds, 8.0), with_cpu=cpu_baselines)
            if dtype == "float32":
                out["reference_main_c"]["f64"] = reference_main_c(pkg, "float64", 0, with_cpu=False)
        except Exception as e:      # noqa: BLE001
            out["reference_main_c"] = {"error": f"{type(e).__name__}: {e}"}
    if extras and world > 1 and config == 4:
        # the weak-scaled companion: one whole configs[1] slab (1 048 576 bodies) per GPU
        wside = a.side or 1024
        wscene = pkg.scenes.box_grid(wside, wside, seed=1 + rank, spin=True, plane=False).astype(dtype)
        wscene.pos[:, 2] += rank * (wside * pkg.scenes.PITCH + 10.0)
        wl = pkg.shard.SlabLayout(wside, wside)
        m = measure(cx, a, wscene, wl, "free", dtype, exchanging=use_exchange)
        out["weak"] = {"scaling": "weak", "value": wscene.n * world * m["steps"] / m["dt"], "unit": "body-steps/s",
                       "ms_per_step": m["dt"] * 1e3 / m["steps"], "bodies_per_gpu": wscene.n, "bodies_total": wscene.n * world,
                       "blocks": m["blocks"], "parallelism": parallelism_text(m, wscene.n),
                       "roofline_frac_per_gpu": roofline_of(m, "free", rsize)["frac"]}
        if a.fused_ticks > 1 and not a.exchange_every_tick:
            # the strong-scaled slabs with 2 and with --fused-ticks ticks per launch (bit-identical results; the reference reads
            # poses every other physics tick, main.c:208, 218): what the launch-bound 131 072-body slab does when a launch carries
            # more than one tick.  Companions; the headline above stays one launch per tick.
            out["fused"] = {}
            for k in sorted({2, a.fused_ticks}):
                m = measure(cx, a, scene, layout, kind, dtype, exchanging=use_exchange, ticks_per_launch=k)
                out["fused"][f"ticks_per_launch_{k}"] = {"scaling": "strong", "value": total_bodies * m["steps"] / m["dt"],
                                                         "unit": "body-steps/s", "ms_per_step": m["dt"] * 1e3 / m["steps"],
                                                         "blocks": m["blocks"]}
        if use_exchange and not a.exchange_every_tick:
            # north_star's wording taken literally: the boundary rows all-gathered at EVERY tick, issued eagerly from the host
            # (a companion number, measured last: should it fail, the headline above stands and the failure is reported here)
            try:
                graph_steps, a.graph_steps = a.graph_steps, 0
                m = measure(cx, a, scene, layout, kind, dtype, exchanging=True, every_tick=True)
                out["exchange_every_tick"] = {"scaling": "strong", "value": total_bodies * m["steps"] / m["dt"], "unit": "body-steps/s",
                                              "ms_per_step": m["dt"] * 1e3 / m["steps"], "blocks": m["blocks"],
                                              "parallelism": parallelism_text(m, scene.n)}
            except Exception as e:      # noqa: BLE001 -- the companion only; every rank runs the same code and fails alike
                out["exchange_every_tick"] = {"error": f"{type(e).__name__}: {e}"}
            finally:
                a.graph_steps = graph_steps
    if extras and world == 1 and kind == "free" and not head["exchanging"] and head["tpl"] == 1:
        if a.fused_ticks > 1:
            # the same scene and step count with several ticks per launch (state in registers between ticks; results are
            # bit-identical, tests/test_gpu_parity.py).  Reported beside the headline, which stays one launch per tick.
            m = measure(cx, a, scene, layout, kind, dtype, exchanging=False, ticks_per_launch=a.fused_ticks)
            out["fused"] = {"ticks_per_launch": a.fused_ticks, "value": scene.n * m["steps"] / m["dt"], "unit": "body-steps/s",
                            "ms_per_step": m["dt"] * 1e3 / m["steps"], "blocks": m["blocks"],
                            "algorithmic_GBps": BYTES_PER_BODY_STEP[kind] * rsize * scene.n * m["steps"] / m["dt"] / 1e9,
                            "note": "one read + one write of the state per launch instead of per tick: past the per-tick HBM "
                                    "roofline, bounded by VALU issue"}
        if a.dtype == "f32" and config == 2 and not a.side:
            # the same scene in the reference's likely precision (dReal leans double: main.c:96, 625-630)
            s64 = scene.astype("float64")
            m = measure(cx, a, s64, layout, kind, "float64", exchanging=False)
            out["f64"] = {"dtype": "f64", "value": s64.n * m["steps"] / m["dt"], "unit": "body-steps/s",
                          "ms_per_step": m["dt"] * 1e3 / m["steps"], "blocks": m["blocks"],
                          "roofline": roofline_of(m, kind, 8, profile_evidence(kind, "f64", s64.n))}
            del s64
            # an HBM-resident size: 16 Mi f32 bodies = 2 GB per slab, 1.1 GB touched per tick (Infinity Cache: 256 MB)
            reps = max(1, (a.hbm_side * a.hbm_side) // scene.n)
            big = tile_scene(np, scene, reps)
            m = measure(cx, a, big, pkg.shard.SlabLayout(side, side * reps), kind, dtype, exchanging=False,
                        steps=min(a.steps, 200), warmup=min(a.warmup, 20))
            out["hbm_resident"] = {"dtype": a.dtype, "bodies": big.n, "value": big.n * m["steps"] / m["dt"], "unit": "body-steps/s",
                                   "ms_per_step": m["dt"] * 1e3 / m["steps"], "steps": m["steps"], "blocks": m["blocks"],
                                   "roofline": roofline_of(m, kind, rsize, profile_evidence(kind, a.dtype, big.n)),
                                   "note": f"{reps} copies of the headline scene side by side: {big.n * 17 * rsize / 1e6:.0f} MB of live state "
                                           "and constants per tick, beyond the 256 MB Infinity Cache, so the fraction is HBM traffic"}
            del big
    if rank == 0 and world == 1 and cpu_baselines:
        out["cpu_baseline"] = cpu_baseline(scene, dtype, kind, a.cpu_seconds)
        allc = cpu_baseline_all_cores(scene, dtype, kind, min(6.0, a.cpu_seconds))
        if allc is not None:
            out["cpu_baseline_all_cores"] = allc
    sys.stdout.flush()
    os.dup2(json_fd, 1)
    os.close(json_fd)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if backend is not None:
        dist.destroy_process_group()


def main():
    a = parse()
    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        sys.exit(spawn_ranks(a.gpus))           # the parent only starts and watches the ranks: no GPU call here
    rank_main(a)


if __name__ == "__main__":
    main()
