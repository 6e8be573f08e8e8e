#!/bin/bash
# `python bench.py --gpus N` (no launcher: it spawns its ranks) with 2 and 4 ranks on ONE GPU — the ranks share the
# device, host-staged transport: exercises bench.py's N > 1 path (BASELINE config 3 family) end to end, --full for the per-rank parity
# usage: bash tools/gpu_n2.sh <output dir>
OUT=${1:?usage: bash tools/gpu_n2.sh <output dir>}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
mkdir -p "$OUT"
for N in 2 4; do
timeout 900 python bench.py --full --gpus $N --steps 3 --warmup 1 > "$OUT/bench_n$N.json" 2> "$OUT/bench_n$N.err"
echo "N=$N rc=$?"; tail -3 "$OUT/bench_n$N.err"; cat "$OUT/bench_n$N.json"
done
