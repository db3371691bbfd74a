#!/bin/bash
# Benches of one build under several environment settings on one box (ENVS: space-separated
# NAME=VALUE words, "-" = none), twice each, after the GPU tests in $TESTS.
# Logs and lines go to $OUT (default build/ab).
set -o pipefail
O=${OUT:-build/ab}
mkdir -p $O
timeout -k 10 300 python -u -m pytest ${TESTS:-tests/test_gpu_engine.py} -x -q --timeout 120 --timeout-method thread -p no:cacheprovider > $O/abe_tests.log 2>&1 || { tail -30 $O/abe_tests.log; exit 1; }
tail -1 $O/abe_tests.log
for rep in 1 2; do
for E in $ENVS; do
  if [ "$E" = "-" ]; then ENV=""; else ENV="$E"; fi
  env $ENV timeout -k 10 200 python bench.py --steps ${STEPS:-300} --warmup 30 --full --no-cpu-baseline > $O/abe.json 2> $O/abe.err || { tail -20 $O/abe.err; exit 1; }
  python -c "import json;d=json.load(open('$O/abe.json'));print('$E',d['ms_per_step'],d['grid_bw_ms'])"
done
done
