"""What a different number of tokens per sequence costs in an append (tllm_session_append_ragged), on the benchmark's 7B SmoothQuant
int8 + int8 KV configuration with the settings of tools/append_timing.py - device events, median (min) of 7 runs, one warm-up
run dropped, the context pass that restores the cache untimed ahead of every run:
    batch 1, the uniform entry            append of 128 onto 896 past; append of n = 8 onto 1024 past
    batch 2, ragged against uniform       lengths (128, 16) against the uniform pass of 128; (16, 4) against the uniform pass of 16
--uniform-only stops behind the first block: it uses nothing a build without the ragged entries lacks, so that the same file times
the uniform entry of an older build (run the two alternately, a process each).
GPU only.    python tools/append_ragged_timing.py [--uniform-only]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'trtllm-llama_amd'))
import torch, numpy as np
import bench
from tensorrt_llm.runtime.native import NativeSession
assert torch.cuda.is_available(), 'append_ragged_timing.py needs a GPU'
cfg = dict(bench.LLAMA_7B, num_layers=32)
V = cfg['vocab_size']
dev = torch.device('cuda', 0)
torch.cuda.set_stream(torch.cuda.Stream(device=dev))
stream = torch.cuda.current_stream().cuda_stream
mode, int8_kv = 'sq', True
qm = bench.QM[mode] | bench.INT8_KV
w = bench.synth_weights(torch, cfg, mode, int8_kv, 1, 0, dev)
RUNS = 7


def session():
    s = NativeSession(dict(cfg, quant_mode=qm, tp_size=1, tp_rank=0))
    for k, t in w.items():
        s.set_tensor(k, t)
    s.finalize()
    return s


def timed(fn, before, n=RUNS):
    ts = []
    for _ in range(n + 1):  # the first run warms (lazy kernel loading, the GEMM profile of a new M)
        before()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts = ts[1:]
    return f'{float(np.median(ts)):.3f} ({min(ts):.3f})'


ids = np.random.default_rng(1).integers(3, V, (2, 1024)).astype(np.int32)
L = lambda B, n: np.full(B, n, np.int32)
print(f'7B SmoothQuant int8 + int8 KV; ms, median (min) of {RUNS} runs between device events, one warm-up run dropped')

s = session()
s.setup(1, 896, 256)
t128 = timed(lambda: s.append(ids[:1, 896:], stream=stream), lambda: s.context(ids[:1, :896], L(1, 896), stream=stream))
s.close()
s = session()
s.setup(1, 1024, 72)
t8 = timed(lambda: s.append(ids[:1, :8], stream=stream), lambda: s.context(ids[:1], L(1, 1024), stream=stream))
print(f'batch 1, uniform entry: append of 128 onto 896: {t128} | append of n = 8 onto 1024: {t8}', flush=True)
s.close()
if '--uniform-only' in sys.argv:
    sys.exit(0)

s = session()
s.setup(2, 896, 256)
restore = lambda: s.context(ids[:, :896], L(2, 896), stream=stream)
for N, lengths in ((128, (128, 16)), (16, (16, 4))):
    tok = ids[:, 896:896 + N]
    lens = np.array(lengths, np.int32)
    tu = timed(lambda: s.append(tok, stream=stream), restore)
    tr = timed(lambda: s.append(tok, lengths=lens, stream=stream), restore)
    tf = timed(lambda: s.append(tok, lengths=L(2, N), stream=stream), restore)
    print(f'batch 2 onto 896 past: uniform pass of {N}: {tu} | lengths {lengths}: {tr} | lengths ({N}, {N}) through the ragged entry: {tf}',
          flush=True)
print(f'attention launches (wave, MFMA): {s.append_launches()}')
s.close()
print('not measured: batch > 2, the fp16 / fp8 cache, grouped heads, other weight modes, a packed row layout')
