#!/bin/bash
# HBM traffic per kernel launch from two rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE: they cannot share a pass on gfx950),
# summarised on the GPU box (the counter databases are too large to travel):
#   $OUT/rNN_pmc_<config>.txt, $OUT/rNN_pmc_summary.json  -> copy into profiles/
# Only --kernel-trace next to --pmc (other trace domains do not share a pass with counters).
set -u
R=${1:-r01}; CFG=${2:-sq}
ROOT=$(pwd); export TMPDIR=/tmp
OUT=$(realpath -m "${OUT:-out}")
mkdir -p "$OUT"
for c in FETCH_SIZE WRITE_SIZE; do
  rm -rf $OUT/pmc_$c
  ( cd "$TMPDIR" && rocprofv3 --kernel-trace --pmc $c -d $OUT/pmc_$c -o pmc -- python $ROOT/bench.py --full --config $CFG --steps 8 --warmup 2 --no-cpu-baseline --no-fp16-ref --no-prefill --no-parity --no-batch-sweep --no-tp-prediction ) > $OUT/pmc_$c.log 2>&1
done
F=$(find $OUT/pmc_FETCH_SIZE -name "*_results.db" | head -1); W=$(find $OUT/pmc_WRITE_SIZE -name "*_results.db" | head -1)
cp profiles/${R}_pmc_summary.json $OUT/${R}_pmc_summary.json 2>/dev/null
python tools/pmc_summary.py "$F" "$W" $CFG $OUT/${R}_pmc_summary.json > $OUT/${R}_pmc_$CFG.txt
rm -rf $OUT/pmc_FETCH_SIZE $OUT/pmc_WRITE_SIZE
cat $OUT/${R}_pmc_$CFG.txt | cut -c1-170
