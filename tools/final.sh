# Round check at HEAD (run from the repo root on the GPU box): the whole GPU suite,
# then the full bench (headline, legs, CPU baseline).  Output in $OUT (default
# bench_out/final).
set -o pipefail
OUT=${OUT:-bench_out/final}
mkdir -p $OUT
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread \
  > $OUT/t.log 2>&1 || exit $?
timeout -k 10 1000 python3 -u bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/b.json 2> $OUT/b.err || exit $?
