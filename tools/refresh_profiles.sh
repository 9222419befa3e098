#!/bin/bash
# Re-create the round's profile artefacts on a GPU box (run from the repo root; OUT = output directory, default out/):
#   $OUT/rNN_bench_default.log        bench.py --full run (every side report), JSON line included
#   $OUT/rNN_bench_kernel_stats.txt   rocprofv3 --kernel-trace --stats of the same command (fewer steps), per kernel
#   $OUT/rNN_prefill_kernel_stats.txt the same for the 1024-token context phase
# then copy them into profiles/ (tracked).  PMC passes: tools/pmc_summary.py.
set -u
R=${1:-r01}
ROOT=$(pwd)
export TMPDIR=/tmp
OUT=$(realpath -m "${OUT:-out}")
mkdir -p "$OUT"
( time python bench.py --full ) > $OUT/${R}_bench_default.log 2>&1
rm -rf $OUT/prof_bench $OUT/prof_prefill
( cd "$TMPDIR" && rocprofv3 --kernel-trace --stats -d $OUT/prof_bench -- python $ROOT/bench.py --full --steps 64 --no-cpu-baseline --no-fp16-ref --no-parity --no-prefill --no-batch-sweep --no-tp-prediction ) > $OUT/prof_bench.log 2>&1
DB=$(find $OUT/prof_bench -name "*_results.db" | head -1)
python tools/rocpd_summary.py "$DB" > $OUT/${R}_bench_kernel_stats.txt
( cd "$TMPDIR" && rocprofv3 --kernel-trace --stats -d $OUT/prof_prefill -- python $ROOT/tools/prefill_probe.py ) > $OUT/prof_prefill.log 2>&1
DB=$(find $OUT/prof_prefill -name "*_results.db" | head -1)
python tools/rocpd_summary.py "$DB" > $OUT/${R}_prefill_kernel_stats.txt
rm -rf $OUT/prof_bench $OUT/prof_prefill   # the databases are large; the summaries are what is kept
tail -3 $OUT/${R}_bench_default.log | cut -c1-600
head -14 $OUT/${R}_bench_kernel_stats.txt
