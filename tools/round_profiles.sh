# Round-end measurement set: the bench line with every diagnostic (--full),
# rocprof kernel stats of the bench, PMC HBM traffic (FETCH_SIZE, WRITE_SIZE
# in separate passes) of the Krum Gram kernel at the bench shape.  Outputs
# under $OUT (default: bench_out/ in the repository).
ROOT=$(cd "$(dirname "$0")/.." && pwd)
export OUT=${OUT:-$ROOT/bench_out}
PROF=$(mktemp -d)
mkdir -p "$OUT"
cd "$ROOT" || exit 1
timeout -k 10 300 python bench.py --full > "$OUT/bench_full.log" 2>&1 || { tail -20 "$OUT/bench_full.log"; exit 1; }
tail -1 "$OUT/bench_full.log"
cd "$PROF" || exit 1
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$PROF/pb" -o b -- python3 "$ROOT/bench.py" --steps 3 --warmup 1 --full --no-cpu-baseline > "$OUT/prof_bench.log" 2>&1 || exit $?
cd "$ROOT" && python3 tools/rocpd_stats.py "$PROF/pb/b_results.db" > "$OUT/prof_bench_stats.txt" || exit $?
ls "$PROF/pb" >> "$OUT/prof_bench.log"
cp "$PROF"/pb/*stats*.csv "$OUT/" 2>/dev/null
for C in FETCH_SIZE WRITE_SIZE; do
  K=128 P=11800394 timeout -k 10 -s KILL 120 rocprofv3 --kernel-trace --pmc $C -d "$PROF/pmc_$C" -o p -- python3 tools/pairwise_only.py > "$OUT/pmc_$C.log" 2>&1 || exit $?
  python3 tools/pmc_stats.py "$PROF/pmc_$C/p_results.db" > "$OUT/pmc_gram_$C.txt" 2>&1
  head -4 "$OUT/pmc_gram_$C.txt"
done
python3 - <<'PY'
import json, os
out = os.environ["OUT"]
def val(path):
    for line in open(path):
        if "gram_partials_kernel" in line:
            return float(line.split()[-2])
f = val(out + "/pmc_gram_FETCH_SIZE.txt"); w = val(out + "/pmc_gram_WRITE_SIZE.txt")
json.dump({"kernel": "gram_partials_kernel", "K": 128, "P": 11800394, "fetch_kib": f, "write_kib": w,
           "source": "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (separate passes), tools/pairwise_only.py K=128 P=11800394"},
          open(out + "/gram_traffic.json", "w"), indent=1)
print("traffic GB per launch:", (2 * f + w) * 1024 / 1e9)
PY
