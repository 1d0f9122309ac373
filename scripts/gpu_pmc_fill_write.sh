#!/bin/bash
# The write-side counter pass of the fill kernel alone (the round profile's set 2 needs more than its 240 s under --pmc)
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-profile_out}; export OUT  # where the logs and profiler output go
export TMPDIR=/tmp
R=${1:-r03}
rm -rf "$OUT"/${R}_pmc_2
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE TCC_EA0_WRREQ_sum TCC_EA0_WRREQ_64B_sum --output-format csv -d "$OUT"/${R}_pmc_2 -- python3 bench.py --full --steps 1 --warmup 0 --placements 1 --no-cpu-baseline --no-index --no-config5 > "$OUT"/${R}_pmc_2.log 2>&1
echo "pmc write set rc=$?"
