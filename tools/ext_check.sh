#!/bin/bash
# extraction/stereo GPU parity tests, then a short bench with its stage timers (no CPU baseline, no LocalBA)
#   usage: bash tools/ext_check.sh OUTDIR
O=${1:?usage: bash tools/ext_check.sh OUTDIR}
mkdir -p $O
timeout -k 10 400 python -u -m pytest tests/test_gpu_extract.py tests/test_gpu_stereo.py tests/test_golden.py tests/test_shim.py tests/test_tracking.py -m gpu -x -q --timeout 120 --timeout-method thread > $O/ext_tests.log 2>&1
rc=$?; echo "tests rc=$rc"; tail -3 $O/ext_tests.log
[ $rc -ne 0 ] && exit $rc
timeout -k 10 300 python bench.py --full --no-cpu-baseline --ba-calls 0 ${BENCH_EXTRA} > $O/bench_ext.log 2>&1
rc=$?; echo "bench rc=$rc"
[ $rc -ne 0 ] && exit $rc
python - $O/bench_ext.log <<'PY'
import json
import sys
j = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print("value", j["value"], "ms/step", j["ms_per_step"], "median", j["median_ms_per_step"])
print(json.dumps(j["stage_ms_per_step"]))
PY
