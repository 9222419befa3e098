"""What the paged KV cache costs in an append pass (session key paged_append; the paged instances of kernels/append_attn.hip), on the
benchmark's 7B SmoothQuant int8 + int8 KV configuration, batch 1, blocks of 64 tokens, with the settings of tools/append_timing.py -
device events, median (min) of 7 runs, one warm-up run dropped, the context pass that restores the cache untimed ahead of every run:
    the linear session                    append of 128 onto 896 past; verify of 8 ids onto 1024 past
    the paged session, same process       the same two
    the attention launches alone          (n, past) = (128, 896) and (8, 1024), linear against paged at T = 16 / 64 / 128
--linear-only stops behind the first block: it uses nothing a build without the paged entries lacks, so that the same file times the
linear session of an older build (run the two alternately, a process each).
GPU only.    python tools/append_paged_timing.py [--linear-only]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'trtllm-llama_amd'))
import torch, numpy as np
import bench
from tensorrt_llm.plugin import capi
from tensorrt_llm.runtime.native import NativeSession
assert torch.cuda.is_available(), 'append_paged_timing.py needs a GPU'
cfg = dict(bench.LLAMA_7B, num_layers=32)
V = cfg['vocab_size']
dev = torch.device('cuda', 0)
torch.cuda.set_stream(torch.cuda.Stream(device=dev))
stream = torch.cuda.current_stream().cuda_stream
mode, int8_kv = 'sq', True
qm = bench.QM[mode] | bench.INT8_KV
w = bench.synth_weights(torch, cfg, mode, int8_kv, 1, 0, dev)
RUNS, T = 7, 64


def session(**keys):
    s = NativeSession(dict(cfg, quant_mode=qm, tp_size=1, tp_rank=0, **keys))
    for k, t in w.items():
        s.set_tensor(k, t)
    s.finalize()
    return s


def timed(fn, before=None, n=RUNS):
    ts = []
    for _ in range(n + 1):  # the first run warms (lazy kernel loading, the GEMM profile of a new M)
        if before:
            before()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts = ts[1:]
    return float(np.median(ts)), min(ts)


ids = np.random.default_rng(1).integers(3, V, (1, 1024)).astype(np.int32)
L = lambda n: np.array([n], np.int32)
fmt = lambda t: f'{t[0]:.3f} ({t[1]:.3f})'
print(f'7B SmoothQuant int8 + int8 KV, batch 1; ms, median (min) of {RUNS} runs between device events, one warm-up run dropped')


def both(keys):
    s = session(**keys)
    s.setup(1, 896, 256)
    t128 = timed(lambda: s.append(ids[:, 896:], stream=stream), lambda: s.context(ids[:, :896], L(896), stream=stream))
    s.close()
    s = session(**keys)
    s.setup(1, 1024, 72)
    s.context(ids, L(1024), stream=stream)
    tok = np.concatenate([s.output_ids()[:, 1024:1025], ids[:, :7]], axis=1).astype(np.int32)  # the pending token and 7 drafts
    t8 = timed(lambda: s.verify(tok, stream=stream), lambda: s.context(ids, L(1024), stream=stream))
    s.close()
    return t128, t8


lin = both({})
print(f'linear session: append of 128 onto 896: {fmt(lin[0])} | verify of 8 ids onto 1024: {fmt(lin[1])}', flush=True)
if '--linear-only' in sys.argv:
    sys.exit(0)
pg = both(dict(paged_kv_cache=1, tokens_per_block=T, paged_append=1))
print(f'paged session (T = {T}): append of 128 onto 896: {fmt(pg[0])} | verify of 8 ids onto 1024: {fmt(pg[1])}')
print(f'paged / linear: append {pg[0][0] / lin[0][0]:.4f}, verify {pg[1][0] / lin[1][0]:.4f}', flush=True)

# ---- the attention launches alone (RoPE + cache write launch included), 7B heads: 32 x 128, int8 cache
from tensorrt_llm.runtime.native import attention_append, attention_append_paged
H, Dh, S = 32, 128, 1152
sc = torch.tensor([16.0], device=dev), torch.tensor([1 / 16.0], device=dev)
reps = 20
for n, past in ((128, 896), (8, 1024)):
    qkv = (torch.randn((1, n, 3 * H * Dh), device=dev) * 0.5).half()
    out = torch.empty((1, n, H * Dh), device=dev, dtype=torch.float16)
    seq = torch.tensor([past], device=dev, dtype=torch.int32)
    args = dict(num_heads=H, head_size=Dh, max_input_len=past, max_past=past, kv_cache_type=capi.INT8, kv_scale_orig_quant=sc[0],
                kv_scale_quant_orig=sc[1], stream=stream)
    cache = torch.randint(-127, 128, (1, 2, H, S, Dh), device=dev, dtype=torch.int8)

    def run_linear():
        for _ in range(reps):
            attention_append(qkv, cache, out, seq, seq, **args)
    t = timed(run_linear)
    line = f'attention launches alone at (n, past) = ({n}, {past}), us per layer: linear {t[0] / reps * 1e3:.1f} ({t[1] / reps * 1e3:.1f})'
    for tpb in (16, 64, 128):
        M = S // tpb
        pool = torch.randint(-127, 128, (2 * M, H, tpb, Dh), device=dev, dtype=torch.int8)
        nbytes = H * tpb * Dh
        order = torch.randperm(M)  # the blocks of the sequence scattered over the pool
        table = torch.stack([pool.data_ptr() + order * nbytes, pool.data_ptr() + (M + order) * nbytes]).view(1, 2, M).to(dev)

        def run_paged():
            for _ in range(reps):
                attention_append_paged(qkv, pool, table, out, seq, seq, tokens_per_block=tpb, max_seq_len=S, **args)
        t = timed(run_paged)
        line += f' | paged T = {tpb}: {t[0] / reps * 1e3:.1f} ({t[1] / reps * 1e3:.1f})'
    print(line, flush=True)
print('not measured: batch > 1, the fp16 / fp8 cache, grouped heads, other weight modes, tables grown on demand')
