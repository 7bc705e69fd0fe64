#!/bin/bash
# The other bench workloads (1B shapes on one GPU, Grouping), every figure (--full): one JSON line each under
# $BENCH_OUT (default bench_out/)
cd "$(dirname "$0")/.."
O=${BENCH_OUT:-bench_out}
mkdir -p "$O"
for w in ${PRESETS:-synthetic-1B-pq16-nc993127-nprobe32 synthetic-1B-pq16-nc993127-nprobe64 deep-1B-d96-opq-pq16-nc999973-nprobe128 grouping-1B-pq16-nc993127-nsubc64-opq-pruning}; do
  timeout -k 10 700 python3 bench.py --full --workload $w > "$O/b_$w.json" 2> "$O/b_$w.err" || exit 1
  echo "[presets] $w done"; tail -c 200 "$O/b_$w.json"
done
w=grouping-100M-pq16-nc131072-nsubc64-opq-pruning
timeout -k 10 500 python3 bench.py --full --workload $w > "$O/b_$w.json" 2> "$O/b_$w.err" || exit 1
echo "[presets] $w done"
