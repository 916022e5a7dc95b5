# The full bench (headline, default legs, CPU baseline) under a time limit.  Output in
# $OUT (default bench_out/full).
set -o pipefail
OUT=${OUT:-bench_out/full}
mkdir -p $OUT
timeout -k 10 900 python3 bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/bench.json 2> $OUT/bench.err || exit $?
