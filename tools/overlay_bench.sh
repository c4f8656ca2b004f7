#!/bin/bash
# The overlay renderer's measurements on one MI355X: whole draw calls and the MJPEG tick beside the comparator, then the
# kernel time from a rocprofv3 run of its own.  Every GPU step has its own time limit and a failure ends the run.
#   tools/overlay_bench.sh [OUT_DIR]     writes OUT_DIR/overlay_bench.json (default profiles/) and the trace under OUT_DIR/overlay_trace/
set -eo pipefail
cd "$(dirname "$0")/.."
O=${1:-profiles}
T=$O/overlay_trace
mkdir -p "$T"
timeout -k 10 300 python3 tools/overlay_bench.py calls --calls 100 --out "$O/overlay_bench.json"
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$T" -o ovl -- python3 tools/overlay_bench.py run --calls 20 > "$T/ovl.log" 2> "$T/ovl.err"
stats=$(find "$T" -name "ovl_kernel_stats.csv" | head -1)
python3 tools/overlay_bench.py kernels --stats "$stats" --out "$O/overlay_bench.json"
