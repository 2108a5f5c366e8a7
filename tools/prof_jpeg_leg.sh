#!/bin/bash
# tools/prof_jpeg_leg.sh OUT -- the `jpeg` workload of tools/run_profile.sh alone (GPU box): bench.py --full --only jpeg under rocprofv3 --kernel-trace --stats
# -> OUT/jpeg.json, OUT/jpeg/**/run_kernel_stats.csv
OUT=$(realpath -m "${1:?usage: tools/prof_jpeg_leg.sh OUT}")
cd /tmp && export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-/root/repo}
mkdir -p "$OUT" && rm -rf "$OUT/jpeg"
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/jpeg" -o run -- python3 $R/bench.py --full --no-cpu-baseline --no-reference-cases --only jpeg > "$OUT/jpeg.json" 2> "$OUT/jpeg.err"
python3 $R/tools/show_bench.py "$OUT/jpeg.json"
