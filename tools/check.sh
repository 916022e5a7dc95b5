# GPU check of a change (run from the repo root on the GPU box): the tests named in
# $TESTS first (default: none), then the whole -m gpu suite, then (BENCH=1) the
# full bench (headline, legs, CPU baseline).  Every step under its own time limit;
# stop at the first failure.  Output in $OUT (default bench_out/check).
set -o pipefail
OUT=${OUT:-bench_out/check}
mkdir -p $OUT
if [ -n "$TESTS" ]; then
  timeout -k 10 600 python -u -m pytest $TESTS -m gpu -x -v --timeout 120 --timeout-method thread \
    > $OUT/targeted.log 2>&1 || exit $?
fi
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread \
  > $OUT/gpu_tests.log 2>&1 || exit $?
if [ "$BENCH" = "1" ]; then
  timeout -k 10 1000 python3 -u bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/b.json 2> $OUT/b.err || exit $?
fi
