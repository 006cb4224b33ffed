#!/bin/bash
# The GPU checks on one machine: the GPU test suite, smoke() and the full benchmark line (bench.py --full).
# usage: gpu_full.sh OUTPUT_DIR.  Exit status = the first failing step's.
set -u
R=${GRAFT_REPO_ROOT:-$(pwd)}; cd "$R"; export PYTHONPATH=$R
OUT=${1:?usage: gpu_full.sh OUTPUT_DIR}
mkdir -p "$OUT"
rc=0
python -m pytest tests -q -m gpu -x > "$OUT/gpu_full_tests.txt" 2>&1 < /dev/null || rc=$?
tail -4 "$OUT/gpu_full_tests.txt"
[ $rc -ne 0 ] && exit $rc
python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/gpu_full_smoke.txt" 2>&1 < /dev/null || rc=$?
tail -2 "$OUT/gpu_full_smoke.txt"
[ $rc -ne 0 ] && exit $rc
python bench.py --full --full-json "$OUT/gpu_full_bench_full.json" > "$OUT/gpu_full_bench.json" 2> "$OUT/gpu_full_bench.err" < /dev/null || rc=$?
python tools/benchline.py < "$OUT/gpu_full_bench.json"; tail -2 "$OUT/gpu_full_bench.err"
exit $rc
