#!/bin/bash
# A/B of integrate_free_lean (csrc/dmx_kernels.hip, csrc/dmx_lean_tick.hpp: the straight-line kernel of a lean contact-free launch)
# against a built checkout of the parent commit, both builds in the same visit to the GPU -- all sections in one, or, where a visit
# has a time limit, AB_PARTS at a time with the same builds.  Every step runs under a time limit of its own, the script ends at the
# first step that fails.  The yardstick is the parent's build, run beside this one.
#
#   [AB_OUT=dir] [AB_RUNS=5] [AB_FULL=3] [AB_CANDIDATE=tree] [AB_PARTS="trace pmc time full dump"] scripts/ab_lean_kernel.sh PARENT_TREE
#
# 1. Kernel trace: one `rocprofv3 --kernel-trace --stats` pass per build (bench.py --steps 300 --warmup 40): the averages of the
#    contact-free kernels.
# 2. Counters per contact-free dispatch on the headline command, counter passes of their own (no tracing beside them), both builds:
#    SQ_INSTS_VALU and SQ_WAVES (their quotient: executed vector instructions per wavefront), FETCH_SIZE and WRITE_SIZE (the claim:
#    the bytes do not move).
# 3. Time: bench.py headline f32 and f64, the builds alternating, AB_RUNS runs each, and this build with DMX_LEAN_KERNEL=0 beside
#    them (it must read as the parent); AB_CANDIDATE, if given: a built copy of this tree with another launch bound
#    on integrate_free_lean (edited by hand), run in the same alternation.
#    `--full --no-cpu-baseline` AB_FULL times each (hbm_resident, fused, configs[0] / [2] / [4], the pen);
#    `--dump-outputs` of both builds in f32 and f64 compared with cmp.
# AB_PARTS picks sections; every call APPENDS its runs to $AB_OUT/ab_lean_kernel.runs and rewrites $AB_OUT/ab_lean_kernel.txt
# (default: bench_out/ab_lean_kernel/; copied to profiles/ab_lean_kernel.txt by hand) from all of them: every run, the medians and
# spreads (max - min) per leg, and the verdict lines -- each headline's median gain must exceed three times the larger of the two
# builds' spreads; no other leg may be slower than the parent by more than the parent's spread on it.
set -u
R=$(cd "$(dirname "$0")/.." && pwd)
PARENT=${1:?usage: scripts/ab_lean_kernel.sh PARENT_TREE (a built checkout of the parent commit)}
PARENT=$(cd "$PARENT" && pwd)
O=${AB_OUT:-$R/bench_out/ab_lean_kernel}; mkdir -p "$O"; O=$(cd "$O" && pwd)
OUT=$O/ab_lean_kernel.runs; touch "$OUT"
RUNS=${AB_RUNS:-5}
FULL=${AB_FULL:-3}
PARTS=${AB_PARTS:-trace pmc time full dump}
has() { case " $PARTS " in *" $1 "*) return 0;; esac; return 1; }
cd /tmp && export TMPDIR=/tmp

[ -s "$OUT" ] || echo "# integrate_free_lean: the straight-line kernel of a lean launch, against the parent's build ($(date -u +%Y-%m-%d)); times are bench.py ms_per_step as us per tick" >> "$OUT"

# ---- 1. kernel trace ------------------------------------------------------------------------------------------------------------
if has trace; then
echo "## rocprofv3 --kernel-trace --stats, one run per build (bench.py --steps 300 --warmup 40)" >> "$OUT"
trace() {   # label, tree
    local label=$1 tree=$2
    local d=$O/trace_$label; rm -rf "$d"
    timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d "$d" -- \
        python3 "$tree/bench.py" --steps 300 --warmup 40 > "$O/trace_$label.log" 2>&1 || { echo "FAILED: trace $label" | tee -a "$OUT"; return 1; }
    python3 - "$label" "$d" >> "$OUT" <<'EOF' || return 1
import csv, glob, sys
label, d = sys.argv[1:3]
f = glob.glob(d + "/**/*kernel_stats.csv", recursive=True)[0]
rows = [r for r in csv.DictReader(open(f)) if "integrate_free" in r["Name"]]
for r in sorted(rows, key=lambda r: -int(r["Calls"])):
    print(f"TRACE {label:8s} {float(r['AverageNs']) / 1e3:8.3f} us average over {int(r['Calls']):5d} calls  {r['Name'][:80]}")
EOF
}
trace parent "$PARENT" || exit 1
trace this "$R" || exit 1
fi

# ---- 2. bytes ------------------------------------------------------------------------------------------------------------------
if has pmc; then
echo "## counters per contact-free dispatch (integrate_free*), headline command (bench.py --no-extras --steps 40 --warmup 8), one rocprofv3 --pmc pass per line" >> "$OUT"
echo "## (the median is a lean launch's; FETCH_SIZE / WRITE_SIZE in KB; SQ_INSTS_VALU / SQ_WAVES = executed vector instructions per wavefront)" >> "$OUT"
pmc() {   # label, tree, counters ...
    local label=$1 tree=$2; shift 2
    local d=$O/pmc_${label}_$1; rm -rf "$d"
    timeout -k 10 300 rocprofv3 --pmc "$@" --output-format csv -d "$d" -- \
        python3 "$tree/bench.py" --no-cpu-baseline --no-extras --steps 40 --warmup 8 > "$d.log" 2>&1 || { echo "FAILED: pmc $label $*" | tee -a "$OUT"; tail -5 "$d.log"; return 1; }
    python3 - "$label" "$d" >> "$OUT" <<'EOF' || return 1
import collections, csv, glob, statistics, sys
label, d = sys.argv[1:3]
f = glob.glob(d + "/**/*counter_collection.csv", recursive=True)[0]
v = collections.defaultdict(list)
for r in csv.DictReader(open(f)):
    if "integrate_free" in r["Kernel_Name"]:
        v[r["Counter_Name"]].append(float(r["Counter_Value"]))
for k, x in v.items():      # every integrate_free dispatch of the run: a lean launch is the median, the one establishing launch per chunk the max
    print(f"PMC {label:8s} {k:14s} dispatches {len(x):3d}  median {statistics.median(x):12.1f}  min {min(x):12.1f}  max {max(x):12.1f}")
EOF
    tail -2 "$OUT" | grep "PMC $label" || true
}
for tree in parent this; do
    [ $tree = parent ] && T=$PARENT || T=$R
    pmc $tree "$T" SQ_INSTS_VALU SQ_WAVES || exit 1
    pmc $tree "$T" FETCH_SIZE || exit 1
    pmc $tree "$T" WRITE_SIZE || exit 1
done
fi

# ---- 3. time ---------------------------------------------------------------------------------------------------------------
# one bench.py run: label, tree, -- bench arguments
bench() {
    local label=$1 tree=$2; shift 2
    local log=$O/run_$(date +%s%N).log
    timeout -k 10 420 python3 "$tree/bench.py" "$@" > "$log" 2>&1 || { echo "FAILED: $label ($log)" | tee -a "$OUT"; tail -5 "$log"; return 1; }
    python3 - "$label" "$log" >> "$OUT" <<'EOF' || return 1
import json, sys
label, log = sys.argv[1:3]
o = json.loads([l for l in open(log) if l.startswith("{")][-1])
parts = [f"headline {o['ms_per_step'] * 1e3:8.3f} us/tick"]
for k in ("f64", "hbm_resident", "fused"):
    if k in o:
        parts.append(f"{k} {o[k]['ms_per_step'] * 1e3:9.3f} us/tick")
for k, leg in list(o.get("configs", {}).items()) + [("pen_" + k, v) for k, v in o.get("reference_pen", {}).items()]:
    parts.append(f"{k} {leg['ms_per_step'] * 1e3:9.3f} us/tick" if "ms_per_step" in leg else f"{k} ERROR {leg.get('error')}")
print(f"RUN {label:14s} " + "  ".join(parts))
EOF
    tail -1 "$OUT"
}
if has time; then
CAND=${AB_CANDIDATE:+$(cd "$AB_CANDIDATE" && pwd)}
echo "## f32 headline, the builds alternating; off = this build with DMX_LEAN_KERNEL=0${CAND:+; cand = the candidate build}" >> "$OUT"
for i in $(seq "$RUNS"); do
    bench "parent_f32" "$PARENT" || exit 1
    bench "this_f32" "$R" || exit 1
    DMX_LEAN_KERNEL=0 bench "off_f32" "$R" || exit 1
    [ -z "$CAND" ] || bench "cand_f32" "$CAND" || exit 1
done
echo "## f64 headline, alternating" >> "$OUT"
for i in $(seq "$RUNS"); do
    bench "parent_f64" "$PARENT" --dtype f64 || exit 1
    bench "this_f64" "$R" --dtype f64 || exit 1
    DMX_LEAN_KERNEL=0 bench "off_f64" "$R" --dtype f64 || exit 1
    [ -z "$CAND" ] || bench "cand_f64" "$CAND" --dtype f64 || exit 1
done
fi
if has full; then
echo "## --full --no-cpu-baseline: headline, f64, hbm_resident (16 Mi bodies: bound by HBM), fused (32 ticks per launch)," >> "$OUT"
echo "## configs[0] (1 024 boxes, mostly exact ticks), configs[2] (step_plane), configs[4] (hulls), the reference's pen" >> "$OUT"
for i in $(seq "$FULL"); do
    bench "parent_full" "$PARENT" --full --no-cpu-baseline || exit 1
    bench "this_full" "$R" --full --no-cpu-baseline || exit 1
done
fi

if has dump; then
echo "## bench.py --steps 200 --warmup 20 --dump-outputs on the parent's build and on this one: cmp of the four arrays" >> "$OUT"
for dt in f32 f64; do
    rm -rf "$O/dump_parent_$dt" "$O/dump_this_$dt"
    timeout -k 10 300 python3 "$PARENT/bench.py" --steps 200 --warmup 20 --dtype $dt --dump-outputs "$O/dump_parent_$dt" > "$O/dump_parent_$dt.log" 2>&1 || { echo "FAILED: parent dump $dt" | tee -a "$OUT"; exit 1; }
    timeout -k 10 300 python3 "$R/bench.py" --steps 200 --warmup 20 --dtype $dt --dump-outputs "$O/dump_this_$dt" > "$O/dump_this_$dt.log" 2>&1 || { echo "FAILED: dump $dt" | tee -a "$OUT"; exit 1; }
    for f in "$O/dump_parent_$dt"/*.npy; do
        cmp "$f" "$O/dump_this_$dt/$(basename "$f")"; rc=$?
        echo "CMP $dt $(basename "$f") ($(stat -c %s "$f") bytes): cmp exit status $rc" >> "$OUT"
        [ $rc -eq 0 ] || exit 1
    done
    rm -rf "$O/dump_parent_$dt" "$O/dump_this_$dt"
done
fi

python3 - "$OUT" > "$OUT.summary" <<'EOF' || exit 1
import re, statistics, sys
runs, pmc = {}, {}
for l in open(sys.argv[1]):
    if l.startswith("RUN "):
        label = l.split()[1]
        for k, v in re.findall(r"(headline|f64|hbm_resident|fused|configs\[\d\]|pen_\w+)\s+([0-9.]+) us/tick", l):
            runs.setdefault((label, k), []).append(float(v))
    m = re.match(r"PMC (\w+)\s+(\w+)\s+dispatches\s+\d+\s+median\s+([0-9.]+)", l)
    if m:
        pmc[(m.group(1), m.group(2))] = float(m.group(3))
print("## medians per contact-free dispatch")
for tree in ("parent", "this"):
    f, w = (pmc.get((tree, k)) for k in ("FETCH_SIZE", "WRITE_SIZE"))
    if None not in (f, w):
        print(f"BYTES {tree:7s} FETCH_SIZE {f:9.1f} KB  WRITE_SIZE {w:9.1f} KB")
    v, n = (pmc.get((tree, k)) for k in ("SQ_INSTS_VALU", "SQ_WAVES"))
    if None not in (v, n) and n > 0:
        print(f"VALU  {tree:7s} SQ_INSTS_VALU {v:12.1f}  SQ_WAVES {n:9.1f}  per wavefront {v / n:7.1f}")
print("## medians (us per tick), spread = max - min")
for (label, k), v in runs.items():
    print(f"MEDIAN {label:12s} {k:13s} n={len(v)}  median {statistics.median(v):9.3f}  min {min(v):9.3f}  max {max(v):9.3f}  spread {max(v) - min(v):7.3f}")
def verdict(name, base, new, key):
    b, n = runs.get((base, key)), runs.get((new, key))
    if not b or not n:
        return
    mb, mn, sp = statistics.median(b), statistics.median(n), max(max(b) - min(b), max(n) - min(n))
    print(f"VERDICT {name:13s} parent {mb:9.3f}  this {mn:9.3f}  ratio {mb / mn:5.3f}x  gain {mb - mn:8.3f}  3 x larger spread {3 * sp:7.3f}  -> "
          + ("gain" if mb - mn > 3 * sp else "NOT beyond three times the spread"))
verdict("f32 headline", "parent_f32", "this_f32", "headline")
verdict("f64 headline", "parent_f64", "this_f64", "headline")
verdict("f32 candidate", "parent_f32", "cand_f32", "headline")
verdict("f64 candidate", "parent_f64", "cand_f64", "headline")
# the switch: this build with DMX_LEAN_KERNEL=0 must read as the parent, within the parent's spread
for dt in ("f32", "f64"):
    b, n = runs.get(("parent_" + dt, "headline")), runs.get(("off_" + dt, "headline"))
    if b and n:
        mb, mn, sp = statistics.median(b), statistics.median(n), max(b) - min(b)
        print(f"SWITCH-OFF {dt} headline  parent {mb:9.3f} (spread {sp:7.3f})  DMX_LEAN_KERNEL=0 {mn:9.3f}  off - parent {mn - mb:+8.3f}  -> "
              + ("as the parent within its spread" if abs(mn - mb) <= sp else "NOT as the parent"))
# nothing else slower: this build against the parent's, within the parent's spread on that leg
for key in sorted(k for (label, k) in runs if label == "parent_full"):
    b, n = runs[("parent_full", key)], runs.get(("this_full", key))
    if not n:
        continue
    mb, mn, sp = statistics.median(b), statistics.median(n), max(b) - min(b)
    print(f"OTHERS {key:16s} parent {mb:9.3f} (spread {sp:7.3f})  this {mn:9.3f}  this - parent {mn - mb:+8.3f}  -> "
          + ("not slower beyond the spread" if mn - mb <= sp else "SLOWER than the parent by more than its spread"))
EOF
cat "$OUT" "$OUT.summary" > "$O/ab_lean_kernel.txt"; rm -f "$OUT.summary"
cat "$O/ab_lean_kernel.txt"
