# GPU: $TESTS first (if set), the whole -m gpu suite, then the headline + C5 legs (no CPU baseline).
# Output in $OUT (default bench_out/c5check).
set -o pipefail
OUT=${OUT:-bench_out/c5check}
mkdir -p $OUT
if [ -n "$TESTS" ]; then
  timeout -k 10 600 python -u -m pytest $TESTS -m gpu -x -v --timeout 120 --timeout-method thread \
    > $OUT/targeted.log 2>&1 || exit $?
fi
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread \
  > $OUT/gpu_tests.log 2>&1 || exit $?
timeout -k 10 600 python3 -u bench.py --full --legs C5 --no-cpu --latency 0 > $OUT/b.json 2> $OUT/b.err || exit $?
