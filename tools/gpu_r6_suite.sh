#!/bin/bash
# GPU box (round 6): the whole -m gpu suite (tools/gpu_tests.sh); with BENCH=1 the driver's bench command after it.
cd "$GRAFT_REPO_ROOT"; export TMPDIR=/tmp
bash tools/gpu_tests.sh; rc=$?
[ $rc -gt 1 ] && exit $rc
if [ -n "$BENCH" ]; then
  bout=${OUT:-bench_outputs}/bench; mkdir -p "$bout"
  timeout -k 10 600 python -u bench.py --full --steps 20 --warmup 5 > "$bout/bench.json" 2> "$bout/bench.err" || exit $?
fi
exit $rc
