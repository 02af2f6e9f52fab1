#!/bin/bash
# GPU box: the HBM-traffic PMC passes of the bench workload (FETCH_SIZE, WRITE_SIZE; separate counter-only runs of the
# plain headline) -> tools/pmc_summary.py (stamped with acestep_mi355x.source_hash(); copied to
# profiles/pmc_traffic.json so the bench line below reports `traffic` -- commit that summary from $OUT/pmc/summary.json),
# then the driver's bench command with --full, then the rocprofv3 kernel-trace summary of a short plain run of the same
# workload.  Results under $OUT (default bench_outputs/).
cd "$(dirname "$0")/.." || exit 1
out=${OUT:-bench_outputs}; mkdir -p "$out/final" "$out/pmc"; export TMPDIR=/tmp
for ctr in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 300 rocprofv3 --pmc $ctr -d "$PWD/$out/pmc/$ctr" -o pmc --output-format csv -- python bench.py --steps 2 --warmup 1 > "$out/pmc/$ctr.log" 2>&1 || exit $?
done
python tools/pmc_summary.py "$out/pmc" "$out/pmc/FETCH_SIZE.log" > "$out/pmc/summary.json" || exit $?
cp "$out/pmc/summary.json" profiles/pmc_traffic.json
timeout -k 10 600 python -u bench.py --full --steps 20 --warmup 5 > "$out/final/bench.json" 2> "$out/final/bench.err" || exit $?
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$PWD/$out/final/prof" -o bench --output-format csv -- python bench.py --steps 10 --warmup 2 > "$out/final/bench_prof.log" 2>&1 || exit $?
