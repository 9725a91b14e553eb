#!/bin/bash
# Round measurement on the GPU box: PMC traffic passes (config 2
# and config 4, tagged with the library's build id), the bench line (reads the
# fresh traffic), and the kernel-trace profile of the bench.  Parity tests run
# after the counter passes (one of them checks the traffic of this build).
#   bash scripts/gpu_measure.sh
#     -> $OUT_DIR/{pytest_gpu.log, pmc_*, pmc_table*.txt, pmc_traffic.json, bench.log, prof/}
#        (default: out/ in the repository)
# The fresh pmc_traffic.json is copied to profiles/ as well.
set -e
R="${GRAFT_REPO_ROOT:-$PWD}"
cd "$R"
export OUT_DIR="${OUT_DIR:-out}"
O="$OUT_DIR"
mkdir -p "$O"
rm -rf "$O"/pmc_* "$O/pmc4"
bash scripts/gpu_check.sh pmc
python scripts/pmc_summary.py "$O" > "$O/pmc_table.txt"
python scripts/pmc_traffic.py "$O" "$O/pmc_traffic.json" --workload config2 > "$O/pmc_traffic.txt"
PMC_DIR="$O/pmc4" PMC_BENCH_ARGS="--config 4" bash scripts/gpu_check.sh pmc
python scripts/pmc_summary.py "$O/pmc4" > "$O/pmc_table_config4.txt"
python scripts/pmc_traffic.py "$O/pmc4" "$O/pmc_traffic.json" --workload config4 >> "$O/pmc_traffic.txt"
cp "$O/pmc_traffic.json" profiles/pmc_traffic.json
rm -rf "$O/pmc_FETCH_SIZE" "$O/pmc_WRITE_SIZE" "$O/pmc4/pmc_FETCH_SIZE" "$O/pmc4/pmc_WRITE_SIZE"
# the tests after the counters: the N = 2 line test expects this build's traffic
if [ -z "$SKIP_TESTS" ]; then
  timeout -k 10 1200 python -u -m pytest tests -x -q -m gpu --timeout 300 --timeout-method thread > "$O/pytest_gpu.log" 2>&1
  echo "tests ok"
fi
bash scripts/gpu_check.sh bench prof
echo "measure ok"
