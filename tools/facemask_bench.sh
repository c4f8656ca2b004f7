#!/bin/bash
# The face masks' measurements on one MI355X: whole calls per style beside the comparator, then the kernel times from a
# rocprofv3 run of its own.  Every GPU step has its own time limit and a failure ends the run.
#   tools/facemask_bench.sh [OUT_DIR]     writes OUT_DIR/facemask_bench.json (default profiles/) and the trace under OUT_DIR/facemask_trace/
set -eo pipefail
cd "$(dirname "$0")/.."
O=${1:-profiles}
T=$O/facemask_trace
mkdir -p "$T"
timeout -k 10 300 python3 tools/facemask_bench.py calls --calls 100 --out "$O/facemask_bench.json"
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$T" -o fm -- python3 tools/facemask_bench.py run --calls 20 > "$T/fm.log" 2> "$T/fm.err"
stats=$(find "$T" -name "fm_kernel_stats.csv" | head -1)
python3 tools/facemask_bench.py kernels --stats "$stats" --out "$O/facemask_bench.json"
