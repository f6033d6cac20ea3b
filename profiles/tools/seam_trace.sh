#!/bin/bash
# rocprofv3 --kernel-trace --stats (no counters) of `bench.py` at the headline size and at the c4 shard, for a built checkout of the PARENT
# commit (directory $1) and for this tree, each in a run of its own; the per-kernel summaries land in OUT_DIR as
# <build>_<workload>_kernel_stats.csv.  The seam launch (xde_seam_kernel) of this tree stands against the parent's
# xde_errnorm_pre_kernel + xde_control_kernel + one of its six xde_combine launches per attempt.
#   profiles/tools/seam_trace.sh PARENT_DIR OUT_DIR
set -o pipefail
PARENT=$(cd "$1" && pwd) || exit 2
mkdir -p "$2" || exit 2
OUT=$(cd "$2" && pwd)
HERE=$(cd "$(dirname "$0")/../.." && pwd)
TMP=$(mktemp -d)
for w in c2 c4-shard; do
  for build in parent this; do
    dir=$PARENT; [ $build = this ] && dir=$HERE
    (cd "$dir" && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$TMP/${build}_$w" -- python3 bench.py --gpus 1 \
       --steps 200 --warmup 20 --workload $w --no-cpu-baseline --no-kernel-events --no-odeint > "$OUT/${build}_${w}_rocprof.json" 2> "$OUT/${build}_${w}_rocprof.err") || exit 1
    stats=$(find "$TMP/${build}_$w" -name '*kernel_stats.csv' | head -1)
    [ -n "$stats" ] || exit 1
    cp "$stats" "$OUT/${build}_${w}_kernel_stats.csv"
    echo "$build $w done"
  done
done
