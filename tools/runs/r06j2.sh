set -e
export TMPDIR=/tmp
O=gpurun_out/r06j; mkdir -p $O
timeout -k 10 600 python -u bench.py --full > $O/bench.json 2> $O/bench.err
timeout -k 10 1000 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > $O/gputests.txt 2>&1
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.txt 2>&1
