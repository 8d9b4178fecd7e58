#!/bin/bash
# the stress record of profiles/<tag>_stress.txt (one box): usage tools/stress.sh [tag=r5]
R=${GRAFT_REPO_ROOT:-$(cd $(dirname $0)/.. && pwd)}
TAG=${1:-r6}
cd $R
run() { echo "== $*"; "$@" 2>/dev/null | tail -6; }
{
run python tools/fp6v2_stress.py 200 32
run python tools/vae_fp6_stress.py 100 8
run python tools/modes_stress.py 30 256
run python tools/r6_stress.py 120
run python tools/backward_stress.py 90 7
run python tools/tinv_stress.py 400 1
} > gpurun_out/${TAG}_stress_final.txt 2>&1
cat gpurun_out/${TAG}_stress_final.txt
