# North-star bench (--full: CPU baseline, cold layer, PMC traffic) + rocprofv3 kernel stats + PMC traffic passes.
# Writes under $OUT (default bench_out/).
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p $OUT/prof
export TMPDIR=/tmp
STEPS=${STEPS:-20}
timeout -k 10 900 python bench.py --full --steps $STEPS --warmup 3 > $OUT/bench_ns.json 2> $OUT/bench_ns.err || exit $?
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof/trace -o run \
  -- python3 bench.py --steps 10 --warmup 2 > $OUT/prof/trace.log 2>&1 || exit $?
timeout -k 10 600 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/prof/fetch -o run \
  --kernel-include-regex spmm -- python3 bench.py --steps 3 --warmup 1 > $OUT/prof/fetch.log 2>&1 || exit $?
timeout -k 10 600 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/prof/write -o run \
  --kernel-include-regex spmm -- python3 bench.py --steps 3 --warmup 1 > $OUT/prof/write.log 2>&1 || exit $?
F=$(find $OUT/prof/fetch -name '*counter_collection.csv' | head -n 1)
W=$(find $OUT/prof/write -name '*counter_collection.csv' | head -n 1)
python tools/pmc_summary.py "$F" "$W" $OUT/prof/pmc_ns.json --config ns
