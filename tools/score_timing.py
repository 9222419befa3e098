"""What scoring a prompt costs: tllm_session_score against tllm_session_context on the benchmark's 7B SmoothQuant int8
configuration, batch 1, S = 128 and 1024 - device events, warmed, alternating - for score_chunk_rows 128 / 256 / 512 / 1024 and the
default (64 MiB of fp32 logits); the streaming kernel alone with its bytes / time; and, for scale, the only route to the same
numbers without it: context on the first token, then force_tokens + step for each of the S - 1 others.  GPU only.
    python tools/score_timing.py"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'trtllm-llama_amd'))
import torch, numpy as np
import bench
from tensorrt_llm.runtime.native import NativeSession, token_logprobs
assert torch.cuda.is_available(), 'score_timing.py needs a GPU'
cfg = dict(bench.LLAMA_7B, num_layers=32)
V = cfg['vocab_size']
dev = torch.device('cuda', 0)
torch.cuda.set_stream(torch.cuda.Stream(device=dev))
stream = torch.cuda.current_stream().cuda_stream
mode, int8_kv = 'sq', True
qm = bench.QM[mode] | bench.INT8_KV
w = bench.synth_weights(torch, cfg, mode, int8_kv, 1, 0, dev)


def session(**keys):
    s = NativeSession(dict(cfg, quant_mode=qm, tp_size=1, tp_rank=0, **keys))
    for k, t in w.items():
        s.set_tensor(k, t)
    s.finalize()
    return s


def timed(fn, n=5):
    """min and median of n runs between device events (the calls synchronise themselves; the events bound the device work)"""
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return min(ts), float(np.median(ts))


print(f'7B SmoothQuant int8 (+ int8 KV), batch 1, vocab {V}; times in ms: min / median of 5, context and score alternating')
for S in (128, 1024):
    ids = np.random.default_rng(1).integers(3, V, (1, S)).astype(np.int32)
    lens = np.array([S], np.int32)
    base = None
    for chunk in (0, 128, 256, 512, 1024):
        if chunk > S:
            continue
        s = session(**({'score_chunk_rows': chunk} if chunk else {}))
        s.setup(1, S, 8)
        s.context(ids, lens, stream=stream)  # profiles the prefill GEMM shapes of this M
        lp, _ = s.score(ids, lens, stream=stream)
        if base is None:
            base = lp
        assert np.array_equal(np.isfinite(lp), np.isfinite(base)) and np.abs(lp - base).max() < 1e-3
        ctx, sco = [], []
        for _ in range(3):
            ctx.append(timed(lambda: (s.context(ids, lens, stream=stream), torch.cuda.synchronize())))
            sco.append(timed(lambda: s.score(ids, lens, stream=stream)))
        c, m = min(x[0] for x in ctx), min(x[0] for x in sco)
        print(f'S={S} chunk rows {chunk or "default (64 MiB)"}: context {c:.3f} (median {np.median([x[1] for x in ctx]):.3f}) | '
              f'score {m:.3f} (median {np.median([x[1] for x in sco]):.3f}) | score - context {m - c:.3f}', flush=True)
        s.close()
    # the streaming kernel alone (partial + the one-thread-per-row merge launch) on [S - 1, V] fp32 logits
    x = torch.randn((S - 1, V), device=dev) * 4
    tg = torch.randint(0, V, (S - 1, ), device=dev, dtype=torch.int32)
    rec = torch.empty((1, S - 1, 8), device=dev)
    token_logprobs(x, tg, partials=rec, stream=stream)
    k = timed(lambda: token_logprobs(x, tg, partials=rec, stream=stream), n=20)
    print(f'S={S} token_logprob kernels on [{S - 1}, {V}] fp32: {k[0] * 1e3:.1f} us (median {k[1] * 1e3:.1f}), '
          f'{(S - 1) * V * 4 / (k[0] * 1e-3) / 1e12:.2f} TB/s of logits read', flush=True)
    # the route without score: one decode step per token
    s = session()
    s.setup(1, 1, S)
    t0 = None
    for rnd in range(2):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        s.context(ids[:, :1], np.array([1], np.int32), stream=stream)
        for t in range(1, S):
            s.force_tokens(ids[:, t], stream=stream)
            s.step(1, use_graph=True, stream=stream)
        s.logits(stream=stream)
        torch.cuda.synchronize(); dt = (time.perf_counter() - t0) * 1e3
    print(f'S={S} context(1 token) + {S - 1} x (force_tokens + step from the graph), logits left on the device: {dt:.1f} ms '
          f'(second run; reading each step\'s logits back, as a log-probability needs, comes on top)', flush=True)
    s.close()
