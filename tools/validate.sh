#!/bin/bash
# Round validation on the GPU box: GPU tests, smoke, the full bench, then the rocprofv3 passes.
#   bash tools/validate.sh <tag>        (logs under $OUT, default validate_out/)
set -euo pipefail
TAG=${1:-r01}
cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-validate_out}
mkdir -p "$OUT"
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > "$OUT/gputests_$TAG.log" 2>&1
tail -3 "$OUT/gputests_$TAG.log"
timeout -k 10 180 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke_$TAG.log" 2>&1
tail -1 "$OUT/smoke_$TAG.log"
timeout -k 10 600 python -u bench.py --full > "$OUT/bench_$TAG.json" 2> "$OUT/bench_$TAG.err"
cat "$OUT/bench_$TAG.json"
bash profiles/profile.sh "$TAG"
