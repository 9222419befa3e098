"""What appending tokens to a live KV cache costs (tllm_session_append) against the routes it replaces, on the benchmark's 7B
SmoothQuant int8 + int8 KV configuration, batch 1 - device events, medians of >= 5 runs, every route in this process on this build:
    append of 128 tokens onto 896 past     | the one-shot context of 1024; 128 x (force_tokens + step from the graph)
    append of n = 1, 4, 8 onto 1024 past   | n steps replayed from the graph
    8 x 128 chunked prefill                | the one-shot context of 1024
    the append attention launches alone at (n, past) = (128, 896), both kernels | the prefill attention launches at S = 1024
GPU only.    python tools/append_timing.py"""
import ctypes, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'trtllm-llama_amd'))
import torch, numpy as np
import bench
from tensorrt_llm.plugin import capi
from tensorrt_llm.runtime.native import APPEND_ATTN_MFMA, APPEND_ATTN_WAVE, NativeSession, attention_append
assert torch.cuda.is_available(), 'append_timing.py needs a GPU'
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


def timed(fn, before=None, n=RUNS):
    """(median, min) ms of n runs of fn between device events; `before` runs untimed ahead of each (it restores the state)"""
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
print(f'7B SmoothQuant int8 + int8 KV, batch 1; ms, median (min) of {RUNS} runs between device events, one warm-up run dropped')

# ---- 1. 128 onto 896
one = session()
one.setup(1, 1024, 72)
t_one = timed(lambda: one.context(ids, L(1024), stream=stream))
a = session()
a.setup(1, 896, 256)
t_ctx896 = timed(lambda: a.context(ids[:, :896], L(896), stream=stream))
t_app = timed(lambda: a.append(ids[:, 896:], stream=stream), before=lambda: a.context(ids[:, :896], L(896), stream=stream))
wave, mfma = a.append_launches()


def forced():
    for t in range(896, 1024):
        a.force_tokens(ids[:, t], stream=stream)
        a.step(1, use_graph=True, stream=stream)


a.context(ids[:, :896], L(896), stream=stream)
forced()
ts = []
for _ in range(3):
    a.context(ids[:, :896], L(896), stream=stream)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    forced()
    torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
print(f'one-shot context of 1024: {t_one[0]:.3f} ({t_one[1]:.3f}) | context of 896: {t_ctx896[0]:.3f} ({t_ctx896[1]:.3f})')
print(f'append of 128 onto 896: {t_app[0]:.3f} ({t_app[1]:.3f})  [{"MFMA" if mfma else "wave"} attention kernel] | '
      f'128 x (force_tokens + step from the graph), host clock: {np.median(ts):.1f} ({min(ts):.1f})')
print(f'CONDITION append(128 onto 896) < one-shot context(1024): {t_app[0]:.3f} < {t_one[0]:.3f}: {"holds" if t_app[0] < t_one[0] else "FAILS"}',
      flush=True)
a.close()

# ---- 2. n = 1, 4, 8 onto 1024 past against n graph steps
restore = lambda: one.context(ids, L(1024), stream=stream)
one.context(ids, L(1024), stream=stream)
one.step(2, use_graph=True, stream=stream)  # captures the step graph
for n in (1, 4, 8):
    tok = ids[:, :n]
    ta = timed(lambda: one.append(tok, stream=stream), before=restore)
    tg = timed(lambda: one.step(n, use_graph=True, stream=stream), before=restore)
    print(f'append of n = {n} onto 1024 past: {ta[0]:.3f} ({ta[1]:.3f}) | {n} step(s) from the graph: {tg[0]:.3f} ({tg[1]:.3f})', flush=True)
one.close()

# ---- 3. 8 x 128 chunked prefill
c = session()
c.setup(1, 128, 1024)


def chunked():
    c.context(ids[:, :128], L(128), stream=stream)
    for k in range(1, 8):
        c.append(ids[:, 128 * k:128 * (k + 1)], stream=stream)


tc = timed(chunked)
print(f'8 x 128 chunked prefill (context of 128 + 7 appends): {tc[0]:.3f} ({tc[1]:.3f}) | one-shot context of 1024: {t_one[0]:.3f} ({t_one[1]:.3f})',
      flush=True)
c.close()

# ---- 4. the attention launches alone (RoPE + cache write launch included on both sides), 7B heads: 32 x 128, int8 cache
H, Dh, n, past, S = 32, 128, 128, 896, 1024
lib = capi.load_library()
qkv = (torch.randn((1, S, 3 * H * Dh), device=dev) * 0.5).half()
cache = torch.randint(-127, 128, (1, 2, H, S + 8, Dh), device=dev, dtype=torch.int8)
out = torch.empty((1, S, H * Dh), device=dev, dtype=torch.float16)
sc = torch.tensor([16.0], device=dev), torch.tensor([1 / 16.0], device=dev)
seq, lens = torch.tensor([past], device=dev, dtype=torch.int32), torch.tensor([past], device=dev, dtype=torch.int32)
reps = 20
for kind, name in ((APPEND_ATTN_MFMA, 'MFMA'), (APPEND_ATTN_WAVE, 'wave')):
    qkv_n, out_n = qkv[:, :n].contiguous(), out[:, :n].contiguous()

    def run():
        for _ in range(reps):
            attention_append(qkv_n, cache, out_n, seq, lens, num_heads=H, head_size=Dh, max_input_len=past, max_past=past,
                             kv_cache_type=capi.INT8, kv_scale_orig_quant=sc[0], kv_scale_quant_orig=sc[1], append_kernel=kind,
                             stream=stream)
    t = timed(run)
    print(f'append attention ({name}) at (n, past) = ({n}, {past}), RoPE + cache write + attention: {t[0] / reps * 1e3:.1f} us '
          f'({t[1] / reps * 1e3:.1f}) per layer')
p = capi.AttentionParams(batch=1, seq=S, num_heads=H, num_kv_heads=H, head_size=Dh, rotary_dim=Dh, neox=1, kv_cache_type=capi.INT8,
                         max_seq_len=S + 8)
lens_s = torch.tensor([S], device=dev, dtype=torch.int32)
p.qkv, p.kv_cache, p.out, p.input_lengths, p.kv_scale_orig_quant = qkv.data_ptr(), cache.data_ptr(), out.data_ptr(), lens_s.data_ptr(), sc[0].data_ptr()
ws = torch.empty(lib.tllm_attention_workspace_size(ctypes.byref(p), 1), device=dev, dtype=torch.uint8)
p.workspace = ws.data_ptr()


def prefill():
    for _ in range(reps):
        assert lib.tllm_attention_context(ctypes.byref(p), stream) == 0, capi.last_error()


t = timed(prefill)
print(f'prefill attention at S = {S}, RoPE + cache write + attention: {t[0] / reps * 1e3:.1f} us ({t[1] / reps * 1e3:.1f}) per layer')
print('not measured: batch > 1, the fp16 / fp8 cache, grouped heads, other weight modes, n between 8 and 128, pasts beyond 1024')
