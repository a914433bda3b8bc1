#!/bin/bash
# A/B of the extraction stages: bench.py stage timers for the default library and each
# build_ab/<variant>/liborbx.so (extraction + stereo only), one line per variant.
#   usage: bash tools/ab_fast.sh OUTDIR
O=${1:?usage: bash tools/ab_fast.sh OUTDIR}
mkdir -p $O
for v in base $(ls build_ab 2>/dev/null); do
  if [ "$v" = base ]; then lib=""; else lib=$PWD/build_ab/$v/liborbx.so; fi
  ORBX_LIB_OVERRIDE=$lib timeout -k 10 200 python bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --ba-calls 0 --pipeline-steps 0 --c3-steps 0 --c1-batch 0 --single-frames 0 --track-steps 0 > $O/ab_$v.log 2>&1 || exit 1
  echo "$v $(tail -1 $O/ab_$v.log | python3 -c 'import json,sys; d=json.loads(sys.stdin.read()); print(d["value"], d["stage_ms_per_step"])')"
done
