#!/bin/bash
# HBM traffic of the bench workload's kernels from the PMC counters, one counter per pass (the MI355X guide's recipe:
# separate --pmc runs, no tracing domains beside them).  Run on the GPU box from the repo root:
#   bash tools/collect_pmc.sh [bench args]        -> $OUT/pmc_bench_<COUNTER>/ + $OUT/pmc_traffic.json  (OUT: tool_out/)
# The program itself follows `--` (python3 bench.py ...), never a wrapper.
set -e
cd /tmp && export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-/root/repo}
OUT=${OUT:-$R/tool_out}; mkdir -p "$OUT"
ARGS="${@:---steps 2 --warmup 1 --no-profile --cpu-seconds 0 --full}"
for C in FETCH_SIZE WRITE_SIZE; do
  rm -rf "$OUT/pmc_bench_$C"
  rocprofv3 --pmc $C -d "$OUT/pmc_bench_$C" -o run --output-format csv -- python3 $R/bench.py $ARGS \
    > "$OUT/pmc_bench_$C.log" 2>&1
  echo "[pmc] $C done"
done
python3 $R/tools/pmc_traffic.py "$OUT/pmc_bench_FETCH_SIZE" "$OUT/pmc_bench_WRITE_SIZE" > "$OUT/pmc_traffic.json"
cat "$OUT/pmc_traffic.json"
