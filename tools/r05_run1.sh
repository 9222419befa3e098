set -x
cd $GRAFT_REPO_ROOT
OUT=${OUT:-out}; mkdir -p "$OUT"
for i in 1 2; do
timeout 300 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-prefill --no-fp16-ref --no-batch-sweep --no-parity > $OUT/r05_ab_fused_$i.json 2> $OUT/r05_ab_fused_$i.err
timeout 300 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-prefill --no-fp16-ref --no-batch-sweep --no-parity --two-launch-attention > $OUT/r05_ab_two_$i.json 2> $OUT/r05_ab_two_$i.err
done
grep -o '"value": [0-9.]*\|"layer_kernel_us": {[^}]*}' $OUT/r05_ab_*.json
timeout 1500 python -m pytest tests/test_gpu_full_size.py tests/test_gpu_bench_geometry.py -x -q 2>&1 | tail -30 > $OUT/r05_fullsize.log
tail -30 $OUT/r05_fullsize.log
