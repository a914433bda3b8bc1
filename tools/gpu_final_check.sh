#!/bin/bash
# smoke(), the full GPU suite and the bench.py --full line at the current tree (round-end rehearsal)
#   usage: bash tools/gpu_final_check.sh OUTDIR   (from the repository root)
O=${1:?usage: bash tools/gpu_final_check.sh OUTDIR}
mkdir -p $O
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $O/smoke.log 2>&1 || { tail -20 $O/smoke.log; exit 1; }
tail -1 $O/smoke.log
timeout -k 10 900 python -u -m pytest -x -q --timeout 120 --timeout-method thread -m gpu tests/ > $O/gputest.log 2>&1
rc=$?; echo rc=$rc >> $O/gputest.log; [ $rc -eq 0 ] || { tail -30 $O/gputest.log; exit $rc; }
tail -2 $O/gputest.log
timeout -k 10 600 python bench.py --full > $O/bench.json 2> $O/bench.err || exit 1
python3 -c "import json; d=json.loads(open('$O/bench.json').read().strip().splitlines()[-1]); print(d['value'], d['ms_per_step'], d['localba']['iters_per_s'], d['stage_ms_per_step'])"
