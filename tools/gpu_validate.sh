#!/bin/bash
# End-of-work validation on the GPU machine, from the repository root: the GPU tests, smoke() and the benchmark with every leg.
# Usage: bash tools/gpu_validate.sh [out_dir]      (the bench line and its stderr go to out_dir, default bench_outputs/)
python -m pytest tests -x -q -m gpu 2>&1 | grep -E "passed|failed|error" | tail -3
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -2
OUT=${1:-bench_outputs}
mkdir -p "$OUT"
python bench.py --full > "$OUT/bench_validate.json" 2> "$OUT/bench_validate.err"; tail -c 3500 "$OUT/bench_validate.json"
