#!/bin/bash
# A/B of what integrate_free leaves out (dmxBatchSetElision / DMX_ELIDE: bit 0 = store elision, bit 1 = uniform constants as
# kernel arguments) on bench.py's headline and its companions, in ONE visit to the GPU: every step under a time limit of its
# own, the script ends at the first step that fails.
#
#   [AB_OUT=dir] [AB_RUNS=5] scripts/ab_elision.sh [PARENT_TREE]
#
# PARENT_TREE: a built checkout of the parent commit (optional).  Its bench.py is run beside this tree's DMX_ELIDE=0 first,
# to confirm that mask 0 IS the parent (within the spread), so that the in-tree A/B stands for parent-versus-this.
# With PARENT_TREE it also takes the parent's `--full` legs and kernel traces, and compares `--dump-outputs` of the two builds (cmp).
# Writes $AB_OUT/ab_elision.txt (default: bench_out/ab_elision/; copied to profiles/ab_elision.txt by hand): every run's ms_per_step, the
# median per setting, the spread (max - min) of the DMX_ELIDE=0 runs, and integrate_free's rocprofv3 average per setting.
set -u
R=$(cd "$(dirname "$0")/.." && pwd)
PARENT=${1:-}
[ -n "$PARENT" ] && PARENT=$(cd "$PARENT" && pwd)
O=${AB_OUT:-$R/bench_out/ab_elision}; mkdir -p "$O"; O=$(cd "$O" && pwd)
OUT=$O/ab_elision.txt; : > "$OUT"
RUNS=${AB_RUNS:-5}
cd /tmp && export TMPDIR=/tmp

# one bench.py run: label, tree, DMX_ELIDE value ("" = the default), key path into the JSON line ..., -- bench arguments
bench() {
    local label=$1 tree=$2 mask=$3; shift 3
    local log=$O/run_$(date +%s%N).log
    if [ -n "$mask" ]; then
        timeout -k 10 420 env DMX_ELIDE="$mask" python3 "$tree/bench.py" "$@" > "$log" 2>&1 || { echo "FAILED: $label ($log)" | tee -a "$OUT"; tail -5 "$log"; return 1; }
    else
        timeout -k 10 420 env -u DMX_ELIDE python3 "$tree/bench.py" "$@" > "$log" 2>&1 || { echo "FAILED: $label ($log)" | tee -a "$OUT"; tail -5 "$log"; return 1; }
    fi
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
print(f"RUN {label:28s} " + "  ".join(parts))
EOF
    tail -1 "$OUT"
}

echo "# integrate_free: DMX_ELIDE A/B, bench.py ms_per_step as us per tick ($(date -u +%Y-%m-%d))" >> "$OUT"
if [ -n "$PARENT" ]; then
    echo "## parent commit's build beside DMX_ELIDE=0 (f32 headline)" >> "$OUT"
    for i in 1 2 3; do
        bench "parent_f32" "$PARENT" "" || exit 1
        bench "check_mask0_f32" "$R" 0 || exit 1
    done
fi
echo "## f32 headline, alternating" >> "$OUT"
for i in $(seq "$RUNS"); do
    bench "mask0_f32" "$R" 0 || exit 1
    bench "default_f32" "$R" "" || exit 1
done
echo "## f64 headline, alternating" >> "$OUT"
for i in $(seq "$RUNS"); do
    bench "mask0_f64" "$R" 0 --dtype f64 || exit 1
    bench "default_f64" "$R" "" --dtype f64 || exit 1
done
echo "## --full --no-cpu-baseline: headline, f64, hbm_resident (16 Mi bodies), fused (32 ticks per launch), and everything else that" >> "$OUT"
echo "## must not get slower: configs[0] (1 024 boxes, mostly exact ticks), configs[2] (step_plane), configs[4] (hulls), the reference's pen" >> "$OUT"
for i in 1 2 3; do
    if [ -n "$PARENT" ]; then bench "parent_full" "$PARENT" "" --full --no-cpu-baseline || exit 1; fi
    bench "mask0_full" "$R" 0 --full --no-cpu-baseline || exit 1
    bench "default_full" "$R" "" --full --no-cpu-baseline || exit 1
done
echo "## each removal alone (f32 headline): 1 = store elision, 2 = uniform constants" >> "$OUT"
bench "mask1_f32" "$R" 1 || exit 1
bench "mask2_f32" "$R" 2 || exit 1

echo "## rocprofv3 --kernel-trace --stats, one run per setting and scene (bench.py [--config 3] --steps 300 --warmup 40): the headline's" >> "$OUT"
echo "## integrate_free, and configs[2]'s step_plane, which this change does not touch (it shares StepParams)" >> "$OUT"
trace() {   # label, tree, DMX_ELIDE value ("" = default), -- bench arguments
    local label=$1 tree=$2 mask=$3; shift 3
    local d=$O/trace_$label; rm -rf "$d"
    if [ -n "$mask" ]; then export DMX_ELIDE=$mask; else unset DMX_ELIDE; fi
    timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d "$d" -- \
        python3 "$tree/bench.py" "$@" --steps 300 --warmup 40 > "$O/trace_$label.log" 2>&1 || { echo "FAILED: trace $label" | tee -a "$OUT"; return 1; }
    unset DMX_ELIDE
    python3 - "$label" "$d" >> "$OUT" <<'EOF' || return 1
import csv, glob, sys
label, d = sys.argv[1:3]
f = glob.glob(d + "/**/*kernel_stats.csv", recursive=True)[0]
rows = [r for r in csv.DictReader(open(f)) if "integrate_free" in r["Name"] or "step_plane" in r["Name"]]
for r in sorted(rows, key=lambda r: -int(r["Calls"])):
    print(f"TRACE {label:22s} {float(r['AverageNs']) / 1e3:8.3f} us average over {int(r['Calls']):5d} calls  {r['Name'][:80]}")
EOF
}
if [ -n "$PARENT" ]; then trace "parent_headline" "$PARENT" "" || exit 1; fi
trace "mask0_headline" "$R" 0 || exit 1
trace "default_headline" "$R" "" || exit 1
if [ -n "$PARENT" ]; then trace "parent_configs2" "$PARENT" "" --config 3 || exit 1; fi
trace "mask0_configs2" "$R" 0 --config 3 || exit 1
trace "default_configs2" "$R" "" --config 3 || exit 1

if [ -n "$PARENT" ]; then
    echo "## bench.py --steps 200 --warmup 20 --dump-outputs on the parent's build and on this one: cmp of the four arrays" >> "$OUT"
    for dt in f32 f64; do
        rm -rf "$O/dump_parent_$dt" "$O/dump_this_$dt"
        timeout -k 10 300 env -u DMX_ELIDE python3 "$PARENT/bench.py" --steps 200 --warmup 20 --dtype $dt --dump-outputs "$O/dump_parent_$dt" > "$O/dump_parent_$dt.log" 2>&1 || { echo "FAILED: parent dump $dt" | tee -a "$OUT"; exit 1; }
        timeout -k 10 300 env -u DMX_ELIDE python3 "$R/bench.py" --steps 200 --warmup 20 --dtype $dt --dump-outputs "$O/dump_this_$dt" > "$O/dump_this_$dt.log" 2>&1 || { echo "FAILED: dump $dt" | tee -a "$OUT"; exit 1; }
        for f in "$O/dump_parent_$dt"/*.npy; do
            cmp "$f" "$O/dump_this_$dt/$(basename "$f")"; rc=$?
            echo "CMP $dt $(basename "$f") ($(stat -c %s "$f") bytes): cmp exit status $rc" >> "$OUT"
            [ $rc -eq 0 ] || exit 1
        done
        rm -rf "$O/dump_parent_$dt" "$O/dump_this_$dt"
    done
fi

python3 - "$OUT" >> "$OUT.summary" <<'EOF' || exit 1
import re, statistics, sys
runs = {}
for l in open(sys.argv[1]):
    if l.startswith("RUN "):
        label = l.split()[1]
        for k, v in re.findall(r"(headline|f64|hbm_resident|fused|configs\[\d\]|pen_\w+)\s+([0-9.]+) us/tick", l):
            runs.setdefault((label, k), []).append(float(v))
print("## medians (us per tick), spread = max - min")
for (label, k), v in runs.items():
    print(f"MEDIAN {label:18s} {k:13s} n={len(v)}  median {statistics.median(v):9.3f}  min {min(v):9.3f}  max {max(v):9.3f}  spread {max(v) - min(v):7.3f}")
def verdict(name, base, new, key):
    b, n = runs.get((base, key)), runs.get((new, key))
    if not b or not n:
        return
    mb, mn, sp = statistics.median(b), statistics.median(n), max(b) - min(b)
    print(f"VERDICT {name:13s} mask 0 {mb:9.3f}  default {mn:9.3f}  ratio {mb / mn:5.3f}x  gain {mb - mn:8.3f}  3 x spread {3 * sp:7.3f}  -> "
          + ("gain" if mb - mn > 3 * sp else "NOT beyond three times the spread"))
verdict("f32 headline", "mask0_f32", "default_f32", "headline")
verdict("f64 headline", "mask0_f64", "default_f64", "headline")
verdict("hbm_resident", "mask0_full", "default_full", "hbm_resident")
verdict("fused", "mask0_full", "default_full", "fused")
verdict("f64 (full)", "mask0_full", "default_full", "f64")
# nothing else slower: the default against the parent's build (or DMX_ELIDE=0 without one), within the spread of that yardstick
base = "parent_full" if ("parent_full", "headline") in runs else "mask0_full"
for key in sorted(k for (label, k) in runs if label == base and (k.startswith("configs") or k.startswith("pen_") or k == "fused")):
    b, n = runs[(base, key)], runs.get(("default_full", key))
    if not n:
        continue
    mb, mn, sp = statistics.median(b), statistics.median(n), max(b) - min(b)
    print(f"OTHERS {key:16s} {base} {mb:9.3f} (spread {sp:7.3f})  default {mn:9.3f}  default - yardstick {mn - mb:+8.3f}  -> "
          + ("not slower beyond the spread" if mn - mb <= sp else "SLOWER than the yardstick by more than its spread"))
p, c = runs.get(("parent_f32", "headline")), runs.get(("check_mask0_f32", "headline"))
if p and c:
    print(f"PARENT vs MASK 0  parent median {statistics.median(p):9.3f} (spread {max(p) - min(p):6.3f})  DMX_ELIDE=0 median {statistics.median(c):9.3f} "
          f"(spread {max(c) - min(c):6.3f})")
EOF
cat "$OUT.summary" >> "$OUT"; rm -f "$OUT.summary"
cat "$OUT"
