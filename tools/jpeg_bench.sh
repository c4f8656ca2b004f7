#!/bin/bash
# The JPEG encoder's measurements on one MI355X: whole calls beside the reference's path, then kernel time per pass from
# rocprofv3 runs of their own.  Every GPU step has its own time limit and a failure ends the run.
#   tools/jpeg_bench.sh [OUT_DIR]     writes OUT_DIR/jpeg_bench.json (default profiles/) and the traces under OUT_DIR/jpeg_trace/
set -eo pipefail
cd "$(dirname "$0")/.."
O=${1:-profiles}
T=$O/jpeg_trace
mkdir -p "$T"
timeout -k 10 300 python3 tools/jpeg_bench.py calls --calls 100 --out "$O/jpeg_bench.json"
for n in 1 8; do
  timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$T" -o "n$n" -- python3 tools/jpeg_bench.py run --frames $n --calls 20 > "$T/n$n.log" 2> "$T/n$n.err"
  stats=$(find "$T" -name "n${n}_kernel_stats.csv" | head -1)
  python3 tools/jpeg_bench.py kernels --stats "$stats" --frames $n --out "$O/jpeg_bench.json"
done
