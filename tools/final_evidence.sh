#!/bin/bash
# Round-end evidence on one box: full GPU parity suite, PMC + rocprofv3 summaries for the library
# as built (tools/round_profile.sh), then the default bench line. Each GPU step is time-limited and
# the first failure ends the script. Outputs go to OUT_DIR (default: bench_out/ in the repository).
set -o pipefail
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export OUT_DIR="${OUT_DIR:-$PWD/bench_out}"
O="$OUT_DIR"
mkdir -p "$O"
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > "$O"/pytest_gpu.log 2>&1 || { echo "pytest failed"; tail -30 "$O"/pytest_gpu.log; exit 1; }
tail -2 "$O"/pytest_gpu.log
export ROUND_DIR=${ROUND_DIR:-r06}
bash tools/round_profile.sh || exit 1
timeout -k 10 400 python bench.py --full > "$O"/bench_default.json 2> "$O"/bench_default.err || { echo "bench failed"; tail -20 "$O"/bench_default.err; exit 1; }
cp "$O"/bench_default.json "$O"/profile_$ROUND_DIR/bench_default.json
cp "$O"/pytest_gpu.log "$O"/profile_$ROUND_DIR/gpu_tests.txt
echo "final_evidence done"
