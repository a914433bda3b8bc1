#!/bin/bash
# Round close-out evidence on the GPU box: smoke, the full GPU suite, rocprofv3 passes of the bench
# and of LocalBA (kernel trace, FETCH_SIZE, WRITE_SIZE; prof_passes below), the SQ counter passes
# (tools/pmc_kernel.sh), then the bench.py --full line.  Every GPU step under its own time limit; the
# script stops at the first failure.  Post-processing on the CPU side:
#   tools/rocprof_stages.py  gpurun_out/close/prof/trace/.../run_kernel_stats.csv HEAD  > profiles/rNN_rocprof_stages.json
#   tools/traffic_json.py    gpurun_out/close/prof HEAD 256                              > profiles/traffic.json
#   tools/ba_traffic.py      gpurun_out/close/prof/ba 10 HEAD                          > profiles/rNN_localba_traffic.json
#   tools/sq_summary.py      gpurun_out/close/pmc                                      > profiles/rNN_sq_counters.json
cd /tmp && export TMPDIR=/tmp && cd - > /dev/null
O=${CLOSE_OUT:-gpurun_out/close}
mkdir -p $O

# rocprofv3 evidence for the bench line:
#   trace : --kernel-trace --stats of a short bench run      -> per-stage ms per step
#   fetch / write : --pmc FETCH_SIZE / WRITE_SIZE (own passes) -> HBM bytes per stage event
#   ba/* : the same three passes over tools/ba_time.py        -> LocalBA bytes per LM iteration
# Counters run in passes without trace domains; each pass under its own time limit.  A pass that
# fails, faults or runs into its limit ends the function with status 1 (each pass checks its own
# status: errexit does not apply to a function called on the left of ||), so nothing more starts.
prof_passes() {
  local OUT ARGS
  OUT=$1
  ARGS=${BENCH_ARGS:---steps 10 --warmup 2 --inflight 1 --profile-steps 5 --no-cpu-baseline --ba-calls 0 --pipeline-steps 0 --c3-steps 0 --c1-batch 0 --single-frames 0 --track-steps 0}
  mkdir -p $OUT $OUT/ba || return 1
  timeout -k 10 240 rocprofv3 --kernel-trace --stats -d $OUT/trace -o run --output-format csv -- python3 bench.py $ARGS > $OUT/trace.log 2>&1 || { echo "trace pass failed"; return 1; }
  echo "trace ok"
  timeout -k 10 240 rocprofv3 --pmc FETCH_SIZE -d $OUT/fetch -o run --output-format csv -- python3 bench.py $ARGS > $OUT/fetch.log 2>&1 || { echo "fetch pass failed"; return 1; }
  echo "fetch ok"
  timeout -k 10 240 rocprofv3 --pmc WRITE_SIZE -d $OUT/write -o run --output-format csv -- python3 bench.py $ARGS > $OUT/write.log 2>&1 || { echo "write pass failed"; return 1; }
  echo "write ok"
  timeout -k 10 240 rocprofv3 --kernel-trace --stats -d $OUT/ba/trace -o run --output-format csv -- python3 tools/ba_time.py 10 > $OUT/ba/trace.log 2>&1 || { echo "ba/trace pass failed"; return 1; }
  echo "ba trace ok"
  timeout -k 10 240 rocprofv3 --pmc FETCH_SIZE -d $OUT/ba/fetch -o run --output-format csv -- python3 tools/ba_time.py 10 > $OUT/ba/fetch.log 2>&1 || { echo "ba/fetch pass failed"; return 1; }
  timeout -k 10 240 rocprofv3 --pmc WRITE_SIZE -d $OUT/ba/write -o run --output-format csv -- python3 tools/ba_time.py 10 > $OUT/ba/write.log 2>&1 || { echo "ba/write pass failed"; return 1; }
  echo "ba pmc ok"
  find $OUT -name "*stats.csv" -o -name "*counter_collection.csv" | head -20
  return 0
}

timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1 || { echo "smoke failed"; tail -20 $O/smoke.log; exit 1; }
echo "smoke ok"
timeout -k 10 900 python -u -m pytest -x -q --timeout 200 --timeout-method thread -m gpu tests/ > $O/gputest.log 2>&1
rc=$?; echo rc=$rc >> $O/gputest.log; [ $rc -eq 0 ] || { tail -30 $O/gputest.log; exit $rc; }
tail -2 $O/gputest.log
prof_passes $O/prof > $O/prof.log 2>&1 || exit 1
OUT=$O/pmc bash tools/pmc_kernel.sh > $O/pmc.log 2>&1 || exit 1
timeout -k 10 600 python bench.py --full > $O/bench.json 2> $O/bench.err || exit 1
tail -c 400 $O/bench.json
