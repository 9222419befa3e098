"""What the fp8 (OCP E4M3) KV cache costs and saves in the generation step: the benchmark's 7B SmoothQuant int8 configuration,
batch 1, contexts 128 / 1024 / 2047, in the SEPARATE-launch form (QKV GEMV, attention with its in-launch merge, O GEMV) for the
three cache types - fp16, int8, fp8 - on the same weights: the attention launch alone (tllm_session_time_kernel, kernel 2) and
tokens/s of the step from its graph.  The yardstick of the fp8 attention launch is the int8 instance of the same kernel in the
same run (same bytes, same loads): the ratio is stated.  One more line per context: the default int8 one-launch form, which an
fp8 session gives up today.  GPU only; writes profiles/kv_fp8_cache.txt (or --out).
    python tools/kv_fp8_timing.py"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'trtllm-llama_amd'))
import torch, numpy as np
import bench
from tensorrt_llm.runtime.native import NativeSession
ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kv_fp8_cache.txt'))
ap.add_argument('--steps', type=int, default=40)
args = ap.parse_args()
assert torch.cuda.is_available(), 'kv_fp8_timing.py needs a GPU'
cfg = dict(bench.LLAMA_7B, num_layers=32)
dev = torch.device('cuda', 0)
torch.cuda.set_stream(torch.cuda.Stream(device=dev))
stream = torch.cuda.current_stream().cuda_stream
FP8_KV = 64
# the scales of bench.py's int8 cache (127 / 6) serve the fp8 cache too: 6 sigma at 127 lies inside +-448
w = bench.synth_weights(torch, cfg, 'sq', True, 1, 0, dev)
KV = {'fp16': 0, 'int8': bench.INT8_KV, 'fp8': FP8_KV}
K, W = args.steps, 5
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def measure(kv, ctx, fused):
    s = NativeSession(dict(cfg, quant_mode=bench.QM['sq'] | KV[kv], tp_size=1, tp_rank=0, fuse_qkv_attention=-1 if fused else 0))
    for k, t in w.items():
        s.set_tensor(k, t)
    s.finalize()
    s.setup(1, ctx, 3 * K + W + 4)
    s.fake_context(ctx, seed=1, stream=stream)
    s.step(2, use_graph=False, stream=stream)
    s.step(W, use_graph=True, stream=stream)
    torch.cuda.synchronize()
    tps = []
    for _ in range(2):
        t0 = time.perf_counter()
        s.step(K, use_graph=True, stream=stream)
        torch.cuda.synchronize()
        tps.append(K / (time.perf_counter() - t0))
    form = s.decode_form()
    att = None
    if not fused:
        att = min(s.time_kernel('attention', 8, stream=stream)[0] for _ in range(5))
    logits = s.logits(stream=stream)
    assert np.isfinite(logits).all()
    nbytes = s.step_bytes(ctx)
    s.close()
    return att, max(tps), form, nbytes


say('7B SmoothQuant int8 (per channel, static), batch 1; attention = microseconds per launch of the split-KV attention (kernel 2:')
say('RoPE + cache append + attention + in-launch merge), min of 5 x 8 sweeps over 32 layers; tokens/s = best of 2 x %d steps from the' % K)
say('step graph, wall clock.  "separate" = QKV GEMV | attention | O GEMV launches (fuse_qkv_attention = 0; the only form of an fp8')
say('session); "one-launch" = the default form of the int8 session (decode form bit 0).')
for ctx in (128, 1024, 2047):
    row = {}
    for kv in ('fp16', 'int8', 'fp8'):
        row[kv] = measure(kv, ctx, False)
        att, tps, form, nbytes = row[kv]
        say(f'context {ctx:4d} separate   {kv:4s} KV: attention {att:7.2f} us | {tps:7.1f} tokens/s | decode form {form} | '
            f'{nbytes / 1e9:.3f} GB per step')
    _, tps1, form1, _ = measure('int8', ctx, True)
    say(f'context {ctx:4d} one-launch int8 KV: {"":20s} | {tps1:7.1f} tokens/s | decode form {form1}')
    a8, af = row['int8'][0], row['fp8'][0]
    say(f'context {ctx:4d} fp8 / int8 attention launch: {af / a8:.4f} ({af - a8:+.2f} us); fp8 / fp16: {af / row["fp16"][0]:.4f}; '
        f'tokens/s fp8 separate vs int8 separate {row["fp8"][1] / row["int8"][1]:.4f}, vs int8 one-launch {row["fp8"][1] / tps1:.4f}')
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, 'w') as f:
    f.write('\n'.join(lines) + '\n')
