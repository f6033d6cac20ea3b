#!/bin/bash
# A/B of two builds of this repository on one GPU, alternating: `bench.py --steps 200 --warmup 20 --repeat-blocks 4` of a checkout of
# the PARENT commit (built, in directory $1) against this tree, PAIRS times per workload, and the output dump of both builds.
#   profiles/tools/seam_ab.sh PARENT_DIR OUT_DIR [WORKLOAD ...]      (default workloads: c2 c4-shard; PAIRS=5; DUMP=1;
#   DUMP_DIR=OUT_DIR: where the two dumps go, 4 x 32 MiB each)
# Every run has a time limit of its own and the script stops at the first run that fails.  profiles/tools/seam_ab_collect.py OUT_DIR
# then prints every block, the medians, the within-build spreads and the verdict (every block of this tree faster than every block of
# the parent, and the medians further apart than three times the larger spread).
set -o pipefail
PARENT=$(cd "$1" && pwd) || exit 2
mkdir -p "$2" || exit 2
OUT=$(cd "$2" && pwd)
shift 2
WORKLOADS=${*:-c2 c4-shard}
PAIRS=${PAIRS:-5}
HERE=$(cd "$(dirname "$0")/../.." && pwd)
ARGS="--gpus 1 --steps 200 --warmup 20"
DUMP_DIR=${DUMP_DIR:-$OUT}
mkdir -p "$DUMP_DIR" || exit 2
if [ "${DUMP:-1}" = 1 ]; then
  (cd "$PARENT" && timeout -k 10 300 python bench.py $ARGS --dump-outputs "$DUMP_DIR/dump_parent" > "$OUT/dump_parent.json") || exit 1
  (cd "$HERE" && timeout -k 10 300 python bench.py $ARGS --dump-outputs "$DUMP_DIR/dump_this" > "$OUT/dump_this.json") || exit 1
fi
for w in $WORKLOADS; do
  for i in $(seq 1 "$PAIRS"); do
    (cd "$PARENT" && timeout -k 10 300 python bench.py $ARGS --repeat-blocks 4 --workload "$w" > "$OUT/${w}_parent_$i.json") || exit 1
    (cd "$HERE" && timeout -k 10 300 python bench.py $ARGS --repeat-blocks 4 --workload "$w" > "$OUT/${w}_this_$i.json") || exit 1
    echo "$w pair $i done"
  done
done
