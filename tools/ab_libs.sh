#!/bin/bash
# Benches of several library builds on one box (LIBS: space-separated paths, "-" = the default build), twice each.
# PRESET picks bench.py's preset (default: its own, lego).  Logs and lines go to $OUT (default build/ab).
set -o pipefail
O=${OUT:-build/ab}
mkdir -p $O
timeout -k 10 300 python -u -m pytest ${TESTS:-tests/test_gpu_engine.py} -x -q --timeout 120 --timeout-method thread -p no:cacheprovider > $O/abl_tests.log 2>&1 || { tail -30 $O/abl_tests.log; exit 1; }
tail -1 $O/abl_tests.log
for rep in 1 2; do
for L in $LIBS; do
  if [ "$L" = "-" ]; then unset MFNERF_LIB; else export MFNERF_LIB=$PWD/$L; fi
  timeout -k 10 200 python bench.py ${PRESET:+--preset $PRESET} --steps ${STEPS:-300} --warmup 30 --full --no-cpu-baseline > $O/abl.json 2> $O/abl.err || { tail -20 $O/abl.err; exit 1; }
  python -c "import json;d=json.load(open('$O/abl.json'));print('$L',d['ms_per_step'],d['grid_bw_ms'])"
done
done
