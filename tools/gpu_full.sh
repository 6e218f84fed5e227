#!/bin/bash
# the whole GPU suite and the full bench line (bench.py --full), on an MI355X
cd "$GRAFT_REPO_ROOT"; mkdir -p gpurun_out; export TMPDIR=/tmp
timeout 2400 python -m pytest tests -x -q -m gpu 2>&1 | tail -8
OUT=${BENCH_OUT:-bench_out}; mkdir -p "$OUT"
timeout 1500 python bench.py --full > "$OUT/bench_full.json" 2> "$OUT/bench_full.err"; echo "bench rc $?"; tail -3 "$OUT/bench_full.err"
