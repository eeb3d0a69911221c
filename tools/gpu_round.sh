#!/bin/bash
# One GPU-box pass: parity tests, smoke, the bench line with every measurement
# (--full; + the dense-occupancy, Config-5 truck and Config-3 fox workloads),
# rocprof stats + PMC. Logs and JSON lines go to $NGP_OUT_DIR/TAG (default
# build/runs/TAG).
# usage (on the box): bash tools/gpu_round.sh TAG [noprof]
set -eo pipefail
TAG=${1:-r01}
R=${GRAFT_REPO_ROOT:-$(pwd)}
cd "$R"
O=${NGP_OUT_DIR:-build/runs}/$TAG
mkdir -p $O
export TMPDIR=/tmp
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread \
    > $O/pytest_gpu.log 2>&1
timeout -k 10 180 python -u -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" \
    > $O/smoke.log 2>&1
timeout -k 10 400 python -u bench.py --full > $O/bench.json 2> $O/bench.err
timeout -k 10 200 python -u bench.py --full --no-cpu --workload lego_dense > $O/bench_dense.json 2> $O/bench_dense.err
timeout -k 10 200 python -u bench.py --full --no-cpu --workload truck > $O/bench_truck.json 2> $O/bench_truck.err
timeout -k 10 200 python -u bench.py --full --no-cpu --workload fox > $O/bench_fox.json 2> $O/bench_fox.err
if [ "$2" != "noprof" ]; then bash tools/prof.sh $TAG/prof; fi
