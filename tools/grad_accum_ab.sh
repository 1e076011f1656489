#!/bin/bash
set -o pipefail
# Same-box comparison for gradient accumulation, alternating fresh processes as tools/step_ab.sh does:
#   tools/grad_accum_ab.sh PARENT_ROOT [batch=64] [rounds=3] [n=4] [steps=48]
# PARENT_ROOT: a built checkout of the parent commit (its plain step is the yardstick).  Per round: the parent's plain step, this
# checkout's plain step (accumulation off: expected equal), this checkout's groups of n micro-steps.  One JSON line each.
PARENT=$1; BATCH=${2:-64}; R=${3:-3}; N=${4:-4}; STEPS=${5:-48}
HERE=$(cd "$(dirname "$0")/.." && pwd)
for i in $(seq 1 $R); do
  for RUN in "--root $PARENT --mode plain" "--root $HERE --mode plain" "--root $HERE --mode accum --n $N"; do
    printf "round %s: " "$i"
    timeout -k 10 300 python "$HERE/tools/grad_accum_time.py" $RUN --batch $BATCH --steps $STEPS --warmup 12 2>/dev/null | tail -1 || exit 1
  done
done
