# All bench workloads on one box, every measurement (--full): one JSON line each under $OUT.
set -o pipefail
cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
for m in newcrfs newcrfs_kitti adabins depthformer; do
  timeout -k 10 400 python -u bench.py --full --model $m > "$OUT"/bench_$m.log 2>&1 || { echo "BENCH $m FAILED"; tail -20 "$OUT"/bench_$m.log; exit 1; }
  grep '^{"metric' "$OUT"/bench_$m.log
done
