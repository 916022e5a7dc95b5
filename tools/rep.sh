#!/bin/bash
# Repeat the headline bench (no legs, no CPU leg; --full for the isolated pass's
# host time) to see run-to-run spread.  Output in $OUT (default bench_out/rep).
#   bash tools/rep.sh <reps> [extra bench args]
set -e
N=$1; shift
OUT=${OUT:-bench_out/rep}
mkdir -p $OUT
for i in $(seq 1 $N); do
  timeout -k 10 200 python3 bench.py --steps 20 --warmup 6 --full --no-cpu --latency 0 --legs none "$@" > $OUT/$i.json 2> $OUT/$i.err
  python3 -c "import json; d=json.load(open('$OUT/$i.json')); print($i, round(d['ms_per_step'],4), d['phase_ms']['host_total'])"
done
