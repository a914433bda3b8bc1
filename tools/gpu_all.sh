#!/bin/bash
# smoke + GPU tests, then (only if both pass) a bench.py --full run.   usage: bash tools/gpu_all.sh OUTDIR
O=${1:?usage: bash tools/gpu_all.sh OUTDIR}
mkdir -p $O
bash tools/gpu_check.sh || exit $?
timeout -k 10 400 python bench.py --full ${BENCH_ARGS:---cpu-baseline-seconds 5} > $O/bench.log 2>&1
rc=$?
echo "bench rc=$rc"
tail -1 $O/bench.log
exit $rc
