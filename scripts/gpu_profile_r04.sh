#!/bin/bash
# Round-4 profile set (one gpurun call): kernel trace of the bench command, counters of both emit kernels, the count kernel's
# counters, the index legs' trace.  Summaries: scripts/summarize_trace_r04.py, scripts/emit_pmc_json.py, scripts/trace_table.py.
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-profile_out}; export OUT  # where the logs and profiler output go
mkdir -p "$OUT"
export TMPDIR=/tmp
R=${1:-r04}
rm -rf "$OUT"/${R}_trace
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT"/${R}_trace -- python3 bench.py --full --steps 10 --warmup 2 --compare-pool 0 --no-cpu-baseline --no-index --no-config5 > "$OUT"/${R}_trace.log 2>&1
echo "trace rc=$?"
tail -c 600 "$OUT"/${R}_trace.log
