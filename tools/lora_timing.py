"""What a LoRA adapter costs at the 7B extents on one GPU: weight-only int4 (+ int8 KV) and fp16, batch 1 and
4, context 1024 - every session in this process on this build, device events, medians of >= 5 runs, one warm-up run dropped:
    ms per generation step (from the graph)   the default session | lora keys, every sequence on -1 | r = 16 on q,k,v,o |
                                              r = 16 on all seven modules
    a 1024-token prefill (batch 1)            the default session | r = 16 on q,k,v,o, with and without the adapter selected
    us of each LoRA launch alone (batch 1 and 4 rows) against its A / B bytes at 8 TB/s
--default-only times the default session's step and prefill alone and needs none of the LoRA entry points: copied into a tree of the
parent commit it gives the parent's figures for the same table.
GPU only.    python tools/lora_timing.py [--configs woq4,fp16] [--batches 1,4] [--default-only]"""
import argparse, ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'trtllm-llama_amd'))
import torch, numpy as np
import bench
from tensorrt_llm.plugin import capi
from tensorrt_llm.runtime.native import NativeSession
ap = argparse.ArgumentParser()
ap.add_argument('--configs', default='woq4,fp16')
ap.add_argument('--batches', default='1,4')
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--default-only', action='store_true')
args = ap.parse_args()
if not args.default_only:
    from tensorrt_llm.runtime import lora_ref as LR
assert torch.cuda.is_available(), 'lora_timing.py needs a GPU'
cfg = dict(bench.LLAMA_7B, num_layers=32)
V, CTX, RANK, RUNS = cfg['vocab_size'], 1024, 16, 5
ALL = 'q,k,v,o,gate,up,down'
dev = torch.device('cuda', 0)
torch.cuda.set_stream(torch.cuda.Stream(device=dev))
stream = torch.cuda.current_stream().cuda_stream


def timed(fn, before=None, n=RUNS):
    ts = []
    for _ in range(n + 1):
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


def session(w, qm, **keys):
    s = NativeSession(dict(cfg, quant_mode=qm, tp_size=1, tp_rank=0, **keys))
    for k, t in w.items():
        s.set_tensor(k, t)
    s.finalize()
    return s


def step_ms(s, B, slots):
    s.setup(B, CTX, args.steps + 8)
    if slots is not None:
        s.lora_select(slots)
    s.fake_context(CTX, seed=1, stream=stream)
    s.step(2, use_graph=True, stream=stream)  # captures
    med, lo = timed(lambda: s.step(args.steps, use_graph=True, stream=stream))
    return med / args.steps, lo / args.steps


print(f'7B extents, context {CTX}; r = {RANK}; ms, median (min) of {RUNS} runs between device events', flush=True)
for mode in args.configs.split(','):
    int8_kv = mode != 'fp16'
    qm = bench.QM[mode] | (bench.INT8_KV if int8_kv else 0)
    w = bench.synth_weights(torch, cfg, mode, int8_kv, 1, 0, dev)
    for mods in ('q,k,v,o', ) if args.default_only else ('q,k,v,o', ALL):
        adapter = None if args.default_only else LR.random_adapter(cfg, 7, RANK, modules=tuple(mods.split(',')))
        keys = dict(lora_max_rank=RANK, lora_max_adapters=1, lora_target_modules=mods)
        for B in [int(b) for b in args.batches.split(',')]:
            if mods == 'q,k,v,o':
                s = session(w, qm)
                t = step_ms(s, B, None)
                print(f'[{mode} batch {B}] step, the default session (form {s.decode_form()}): {t[0]:.4f} ({t[1]:.4f})', flush=True)
                s.close()
            if args.default_only:
                continue
            s = session(w, qm, **keys)
            s.lora_load(0, adapter, 32.0)
            t0 = step_ms(s, B, [-1] * B)
            t1 = step_ms(s, B, [0] * B)
            print(f'[{mode} batch {B}] step, lora keys on {mods}: every sequence on -1 {t0[0]:.4f} ({t0[1]:.4f}) | on the adapter '
                  f'{t1[0]:.4f} ({t1[1]:.4f})', flush=True)
            s.close()
    # ---- prefill of 1024 tokens, batch 1
    ids = np.random.default_rng(1).integers(3, V, (1, CTX)).astype(np.int32)
    lens = np.array([CTX], np.int32)
    s = session(w, qm)
    s.setup(1, CTX, 8)
    t = timed(lambda: s.context(ids, lens, stream=stream))
    print(f'[{mode}] prefill of {CTX}, the default session: {t[0]:.3f} ({t[1]:.3f})', flush=True)
    s.close()
    if args.default_only:
        del w
        torch.cuda.empty_cache()
        continue
    s = session(w, qm, lora_max_rank=RANK, lora_max_adapters=1, lora_target_modules='q,k,v,o')
    s.lora_load(0, LR.random_adapter(cfg, 7, RANK, modules=('q', 'k', 'v', 'o')), 32.0)
    s.setup(1, CTX, 8)
    t0 = timed(lambda: s.context(ids, lens, stream=stream))
    s.lora_select([0])
    t1 = timed(lambda: s.context(ids, lens, stream=stream))
    print(f'[{mode}] prefill of {CTX}, lora keys on q,k,v,o: on -1 {t0[0]:.3f} ({t0[1]:.3f}) | on the adapter {t1[0]:.3f} ({t1[1]:.3f})',
          flush=True)
    s.close()
    del w
    torch.cuda.empty_cache()

if args.default_only:
    sys.exit(0)
# ---- the launches alone
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from test_gpu_lora_kernels import ExpandParams, ShrinkParams, table  # noqa: E402
lib = capi.load_library()
lib.tllm_lora_shrink.argtypes = [ctypes.POINTER(ShrinkParams), ctypes.c_void_p]
lib.tllm_lora_expand.argtypes = [ctypes.POINTER(ExpandParams), ctypes.c_void_p]
D, I = cfg['hidden_size'], cfg['inter_size']
SITES = (('qkv', D, (D, D, D), 1), ('dense', D, (D, ), 0), ('fc|gate', D, (I, I), 1), ('proj', I, (D, ), 0))
reps = 50
for M in (1, 4, 1024):
    for name, K, segs, pro in SITES:
        nseg, N, R = len(segs), sum(segs), len(segs) * RANK
        x = (torch.randn((M, K), device=dev)).half()
        gamma = torch.ones(K, device=dev).half()
        A = (torch.randn((R, K), device=dev) / K ** 0.5).half()
        Bm = (torch.randn((N, RANK), device=dev) * 0.05).half()
        y = torch.zeros((M, N), device=dev).half()
        t = torch.zeros((M, R), device=dev)
        rows = torch.zeros(M, device=dev, dtype=torch.int32)
        tab = table([A], [Bm], [1e-3])
        sp = ShrinkParams(M=M, K=K, R=R, pro=pro, x=x.data_ptr(), ldx=K, gamma=gamma.data_ptr(), eps=1e-6, row_adapter=rows.data_ptr(),
                          table=tab.data_ptr(), num_adapters=1, t=t.data_ptr())
        ep = ExpandParams(M=M, r=RANK, nseg=nseg, t=t.data_ptr(), row_adapter=rows.data_ptr(), table=tab.data_ptr(), num_adapters=1)
        off = 0
        for g, n in enumerate(segs):
            ep.seg_n[g], ep.seg_y[g], ep.seg_ldy[g] = n, y.data_ptr() + 2 * off, N
            off += n

        def run(fn, p):
            def f():
                for _ in range(reps):
                    assert fn(ctypes.byref(p), stream) == 0, capi.last_error()
            return f
        ts, te = timed(run(lib.tllm_lora_shrink, sp)), timed(run(lib.tllm_lora_expand, ep))
        ab, bb = R * K * 2, N * RANK * 2
        print(f'[{M} rows] {name}: shrink {ts[0] / reps * 1e3:.2f} us (A {ab / 1e3:.0f} KB = {ab / 8e6:.3f} us at 8 TB/s) | expand '
              f'{te[0] / reps * 1e3:.2f} us (B {bb / 1e3:.0f} KB = {bb / 8e6:.3f} us at 8 TB/s)', flush=True)
print('back-to-back launches on one stream: the figures include each launch\'s boundary; the operands stay in the L2 / Infinity Cache')
