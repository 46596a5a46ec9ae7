#!/bin/bash
# round end: the whole GPU suite + smoke (scripts/gpu_full.sh), then the default bench with every sub-record (--full)
set -u
cd "$GRAFT_REPO_ROOT"; mkdir -p gpurun_out/final
export HSA_ENABLE_IPC_MODE_LEGACY=0 PYTHONUNBUFFERED=1
bash scripts/gpu_full.sh 1000 || exit $?
OUT=${OUT:-bench_out/final}; mkdir -p "$OUT"
timeout -k 10 600 python bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err" || { tail -30 "$OUT/bench.err"; exit 1; }
tail -1 "$OUT/bench.json"
