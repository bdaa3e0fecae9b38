#!/bin/bash
# Round-end artifacts: the default bench line with every diagnostic and the
# CPU baseline (--full), and a rocprofv3 kernel-trace summary of a short
# bench run.  Outputs under $OUT (default: bench_out/ in the repository).
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$ROOT/bench_out}
PROF=$(mktemp -d)
mkdir -p "$OUT"
cd "$ROOT" || exit 1
timeout -k 10 400 python bench.py --full > "$OUT/bench_final.log" 2>&1 || { tail -20 "$OUT/bench_final.log"; exit 1; }
tail -1 "$OUT/bench_final.log"
cd "$PROF" && timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$PROF/pf" -o f -- python3 "$ROOT/bench.py" --steps 3 --warmup 1 --full --no-cpu-baseline > "$OUT/prof_final.log" 2>&1 || exit $?
cd "$ROOT" && python3 tools/rocpd_stats.py "$PROF/pf/f_results.db" > "$OUT/prof_final_stats.txt" || exit $?
head -5 "$OUT/prof_final_stats.txt"
