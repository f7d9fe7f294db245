#!/bin/bash
# Re-measures the four profiles/hbm_pmc_*.json that bench.py reads for `roofline.traffic` (it refuses them once
# csrc/dmx_kernels.hip has changed): per case one `rocprofv3 --kernel-trace --stats` pass and two counter passes
# (FETCH_SIZE, WRITE_SIZE), each a run of its own, folded by scripts/pmc_traffic.py.  Every pass has its own time
# limit and the script ends at the first one that fails.  Results land in $PROFILE_OUT (default: bench_out/profile_traffic/); the JSONs and
# the kernel-stats tables worth keeping are copied to profiles/ afterwards.
set -u
R=$(cd "$(dirname "$0")/.." && pwd); O=${PROFILE_OUT:-$R/bench_out/profile_traffic}; mkdir -p "$O"; O=$(cd "$O" && pwd); cd /tmp && export TMPDIR=/tmp
prof() {   # name  kernel  kind dtype n  -- bench flags
    local name=$1 kernel=$2 kind=$3 dtype=$4 n=$5 pass; shift 5
    local bench=(python3 "$R/bench.py" --no-cpu-baseline --no-extras "$@")
    rm -rf "$O/${name}_stats" "$O/${name}_fetch" "$O/${name}_write"
    timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/${name}_stats" -- "${bench[@]}" --steps 300 --warmup 40 > "$O/${name}_stats.log" 2>&1 || return 1
    timeout -k 10 420 rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$O/${name}_fetch" -- "${bench[@]}" --steps 40 --warmup 8 > "$O/${name}_fetch.log" 2>&1 || return 1
    timeout -k 10 420 rocprofv3 --pmc WRITE_SIZE --output-format csv -d "$O/${name}_write" -- "${bench[@]}" --steps 40 --warmup 8 > "$O/${name}_write.log" 2>&1 || return 1
    (cd "$R" && python3 scripts/pmc_traffic.py "$kind" "$dtype" "$n" "$kernel" "$O/${name}_fetch" "$O/${name}_write" "$O/${name}_stats" "$O/hbm_pmc_${kind}_${dtype}_${n}.json") || return 1
    cp "$(ls "$O/${name}_stats"/*/*kernel_stats.csv | head -1)" "$O/${name}_kernel_stats.csv"
}
prof c2_f32 integrate_free free f32 1048576 || exit 1
prof c2_f64 integrate_free free f64 1048576 --dtype f64 || exit 1
prof c2_f32_16Mi integrate_free free f32 16777216 --side 4096 || exit 1
prof c3_f32 step_plane plane f32 262144 --config 3 || exit 1
ls "$O"/*.json "$O"/*.csv
