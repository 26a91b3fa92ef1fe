#!/bin/bash
# Round-end evidence on the GPU box: bench line, rocprofv3 kernel stats of the same command, PMC traffic passes.
#   bash tools/round_profiles.sh <tag>      -> $OUT/<tag>_*, OUT: tool_out/   (copy what should be judged into profiles/)
# The bench line and its kernel stats are of `bench.py --full` (roofline, profile, CPU baselines, PCG beside the headline).
set -e
TAG=${1:-rXX}
R=${GRAFT_REPO_ROOT:-/root/repo}
export OUT=${OUT:-$R/tool_out}; mkdir -p "$OUT"
cd $R
python3 bench.py --full > "$OUT/${TAG}_bench_venice.json" 2> "$OUT/${TAG}_bench_venice.err"
tail -c 600 "$OUT/${TAG}_bench_venice.json"; echo
cd /tmp && export TMPDIR=/tmp
rm -rf "$OUT/${TAG}_prof"
rocprofv3 --kernel-trace --stats -d "$OUT/${TAG}_prof" -o run --output-format csv -- python3 $R/bench.py --full --cpu-seconds 0 \
  > "$OUT/${TAG}_prof.log" 2>&1
find "$OUT/${TAG}_prof" -name "*kernel_stats.csv" -exec cp {} "$OUT/${TAG}_kernel_stats_venice_bench.csv" \;
find "$OUT/${TAG}_prof" -name "*kernel_trace.csv" -delete   # large; the stats summary is what is kept
head -12 "$OUT/${TAG}_kernel_stats_venice_bench.csv"
cd $R && bash tools/collect_pmc.sh > "$OUT/${TAG}_pmc.log" 2>&1 && cp "$OUT/pmc_traffic.json" "$OUT/${TAG}_pmc_traffic.json"
rm -rf "$OUT/pmc_bench_FETCH_SIZE" "$OUT/pmc_bench_WRITE_SIZE"
echo "[round_profiles] done"
