#!/bin/bash
# Round profile: bench JSON (with cpu baseline) + rocprofv3 kernel stats of the same command (without cpu leg).
#   bash tools/gpu_profile_round.sh [OUTDIR]      (default: profile_out/ in the repository root)
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:-$R/profile_out}
mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd) || exit 1
cd "$R"
timeout 1200 python bench.py --full > "$OUT/bench_full.log" 2>&1; tail -n 1 "$OUT/bench_full.log" > "$OUT/bench_line.json"; cut -c1-600 "$OUT/bench_line.json"
cd "$OUT" && timeout 1200 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof" -- python3 "$R/bench.py" --steps 10 --warmup 3 --full --no-cpu-baseline > "$OUT/prof.log" 2>&1
f=$(find "$OUT/prof" -name "*kernel_stats.csv" | head -1); cp "$f" "$OUT/kernel_stats.csv"
grep '"metric"' "$OUT/prof.log" | tail -1 > "$OUT/bench_under_rocprof.json"
find "$OUT/prof" -name "*kernel_trace.csv" -delete
head -12 "$OUT/kernel_stats.csv" | cut -c1-150
# the same steps with one launch at a time (what bench.py's `roofline.achieved` is measured on): per-kernel averages
# without the other model's workgroups inside them
export DEVIT_TEACHER_STREAM=0 DEVIT_WGRAD_STREAM=0 && timeout 1200 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_serial" -- python3 "$R/bench.py" --steps 10 --warmup 3 --full --no-cpu-baseline --teacher-lookahead 0 > "$OUT/prof_serial.log" 2>&1
unset DEVIT_TEACHER_STREAM DEVIT_WGRAD_STREAM
f=$(find "$OUT/prof_serial" -name "*kernel_stats.csv" | head -1); cp "$f" "$OUT/kernel_stats_serial.csv"
find "$OUT/prof_serial" -name "*kernel_trace.csv" -delete
grep '"metric"' "$OUT/prof_serial.log" | tail -1 | cut -c1-200
