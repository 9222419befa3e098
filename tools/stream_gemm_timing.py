"""What the weight-streaming GEMM (tllm_gemm_stream, 9 <= M <= 64 rows; --wtype 3 SmoothQuant, 1 / 2 weight-only int8 / int4: fp16
activations and scales, results compared within 2 fp16 ulp of the row's largest output and not bit for bit, part 2 on the
weight-only session; --wtype 0 fp16 weights: tllm_gemm_stream_f16, every route held to a float64 product on the device) costs against the dispatch of tllm_gemm on the
same operands, and what the session key stream_gemm does to the verify pass - device events, medians with the spread, the two routes
alternating in this process on this build.
  1. the four 7B shapes (N x K: 12288 x 4096, 4096 x 4096, 11008 x 4096, 4096 x 11008), per-channel x per-token scales where the type
     has them, fp16 output, M = 9, 16, 24, 32, 48, 64 (16, 32, 48, 64 but for SmoothQuant): microseconds per call and weight bytes /
     time as a share of 8 TB/s.  Successive calls rotate over 8 copies of the weights (400 MB and more: no copy is in a cache when
     its turn comes, as in a pass over 32 layers).  --wtype 0 adds the lm_head (32000 x 4096, fp32 logits, 4 copies) with a third
     route: the slabs of 8 rows through tllm_gemv (plain prologue) that run_head launches for more than 8 rows;
  2. the verify pass of n = 16 / 32 ids with and without the key (7B SmoothQuant int8 + int8 KV, batch 1, 1024-token cache,
     append_split = 1 on both), beside one step from the graph, with the break-even acceptance.  --wtype 0: the fp16 engine (fp16
     KV) keyless against stream_gemm = 2, then the SmoothQuant engine under stream_gemm = 1 against 2 (the head alone differs).
GPU only.    python tools/stream_gemm_timing.py [--wtype 3] [--out profiles/stream_gemm.txt] [--no_pass]"""
import argparse, ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'trtllm-llama_amd'))
import torch, numpy as np
import bench
from tensorrt_llm.plugin import capi
from tensorrt_llm.runtime.native import NativeSession
ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'stream_gemm.txt'))
ap.add_argument('--wtype', type=int, default=3, choices=[0, 1, 2, 3], help='0 fp16, 1 / 2 weight-only int8 / int4, 3 SmoothQuant')
ap.add_argument('--no_pass', action='store_true', help='part 1 alone')
args = ap.parse_args()
assert torch.cuda.is_available(), 'stream_gemm_timing.py needs a GPU'
dev = torch.device('cuda', 0)
CUS = torch.cuda.get_device_properties(dev).multi_processor_count
RUNS, REPS, COPIES = 9, 16, 8
lib = capi.load_library()
lib.tllm_gemm.argtypes = [ctypes.POINTER(capi.GemmParams), ctypes.c_void_p]
lib.tllm_gemm.restype = ctypes.c_int32
WT = args.wtype
F16 = WT == 0
WOQ, WBYTES = WT != 3, {0: 2.0, 1: 1.0, 2: 0.5, 3: 1.0}[WT]  # not SmoothQuant: fp16 A (and scales); bytes per weight
MS = (9, 16, 24, 32, 48, 64) if WT == 3 else (16, 32, 48, 64)
HEAD = (32000, 4096)
lines = []


class GemvParams(ctypes.Structure):
    """tllm_gemv_params_t (include/tllm_runtime_api.h)"""
    _fields_ = [(n, ctypes.c_int32) for n in ('wtype', 'pro', 'epi', 'out_dtype', 'M', 'N', 'K')] + [
        ('x', ctypes.c_void_p), ('ldx', ctypes.c_int64), ('w', ctypes.c_void_p), ('ldw', ctypes.c_int64), ('scale_col', ctypes.c_void_p),
        ('scale_row', ctypes.c_void_p), ('per_channel', ctypes.c_int32), ('per_token', ctypes.c_int32), ('gamma', ctypes.c_void_p),
        ('eps', ctypes.c_float), ('act_scale', ctypes.c_void_p), ('dyn_scale_out', ctypes.c_void_p), ('x_pro_out', ctypes.c_void_p),
        ('residual', ctypes.c_void_p), ('epi_scale', ctypes.c_void_p), ('y', ctypes.c_void_p), ('ldy', ctypes.c_int64)]


lib.tllm_gemv.argtypes = [ctypes.POINTER(GemvParams), ctypes.c_void_p]
lib.tllm_gemv.restype = ctypes.c_int32


def say(text):
    print(text, flush=True)
    lines.append(text)


def event_us(fn, reps=REPS):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def gemm_case(M, N, K, head=False):
    g = torch.Generator(device=dev).manual_seed(N + K + M)
    copies = 4 if head else COPIES
    ldw = int(K * WBYTES)  # bytes; any byte is a valid s8 / u8 / pair of nibbles
    a = torch.randn((64, K), generator=g, device=dev).half() if WOQ else torch.randint(-127, 128, (64, K), generator=g, device=dev, dtype=torch.int8)
    if F16:
        ws_ = [(torch.randn((N, K), generator=g, device=dev) * K ** -0.5).half() for _ in range(copies)]
    else:
        ws_ = [torch.randint(-127, 128, (N, ldw), generator=g, device=dev, dtype=torch.int8) for _ in range(copies)]
    sc = torch.rand((N, ), generator=g, device=dev) * 1e-5
    sc = (sc * 1e3).half() if WOQ else sc
    sr = torch.rand((64, ), generator=g, device=dev)
    odt = torch.float32 if head else torch.float16
    c0, c1, c2 = (torch.zeros((64, N), device=dev, dtype=odt) for _ in range(3))
    scales = {} if F16 else dict(scale_col=sc.data_ptr(), scale_row=sr.data_ptr(), per_channel=1, per_token=1)
    q = lambda w, c: capi.GemmParams(wtype=WT, out_dtype=0 if head else 1, M=M, N=N, K=K, a=a.data_ptr(), lda=K, w=w.data_ptr(), ldw=ldw,
                                     c=c.data_ptr(), ldc=N, **scales)
    nbytes, slices = ctypes.c_int64(), ctypes.c_int32()
    layout = lib.tllm_gemm_stream_f16_layout if F16 else lib.tllm_gemm_stream_layout
    assert layout(ctypes.byref(q(ws_[0], c0)), CUS, ctypes.byref(nbytes), ctypes.byref(slices), *[None] * 5) == 0
    work = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    turn = [0]

    def base():
        turn[0] += 1
        assert lib.tllm_gemm(ctypes.byref(q(ws_[turn[0] % copies], c0)), stream) == 0, capi.last_error()

    def new():
        turn[0] += 1
        p = ctypes.byref(q(ws_[turn[0] % copies], c1))
        rc = lib.tllm_gemm_stream_f16(p, None, None, work.data_ptr(), work.numel(), stream) if F16 else \
            lib.tllm_gemm_stream(p, None, work.data_ptr(), work.numel(), stream)
        assert rc == 0, capi.last_error()

    def slabs():  # run_head's route for more than 8 rows: the whole head once per slab of 8
        turn[0] += 1
        w = ws_[turn[0] % copies]
        for m0 in range(0, M, 8):
            p = GemvParams(wtype=0, pro=0, epi=0, out_dtype=0, M=min(8, M - m0), N=N, K=K, x=a.data_ptr() + m0 * K * 2, ldx=K,
                           w=w.data_ptr(), ldw=ldw, eps=1e-6, y=c2.data_ptr() + m0 * N * 4, ldy=N)
            assert lib.tllm_gemv(ctypes.byref(p), stream) == 0, capi.last_error()
    routes = dict(base=base, new=new, **(dict(slabs=slabs) if head else {}))
    t = {k: [] for k in routes}
    for i in range(RUNS + 1):
        for k, fn in routes.items():
            t[k].append(event_us(fn))
    # the same weights last: the routes agree (SmoothQuant: bit for bit)
    for fn in routes.values():
        turn[0] = -1
        fn()
    torch.cuda.synchronize()
    note = ''
    if F16:
        # fp16 weights: every route against a float64 product on the device, in fp16 ulp of the row's largest |v| (the bound of
        # tests/test_gpu_gemm_instances.py: 1.0 for fp16 output, 0.5 for fp32)
        v = a[:M].double() @ ws_[0].double().T
        ulp = torch.exp2(torch.floor(torch.log2(v.abs().amax(1, keepdim=True))) - 10)
        err = {k: float(((c[:M].double() - v).abs() / ulp).max()) for k, c in zip(routes, (c0, c1, c2))}
        note = ' | worst error in fp16 ulp of the row: ' + ', '.join(f'{k} {e:.3f}' for k, e in err.items())
        assert err['new'] <= (0.5 if head else 1.0), 'the stream misses the bound of the fp16 GEMMs'
    elif WOQ:
        for other in [c1] + ([c2] if head else []):
            d, top = (c0[:M].float() - other[:M].float()).abs().amax(1), c0[:M].float().abs().amax(1)
            assert bool((d <= top * 2.0 ** -9).all()), 'the routes differ by more than 2 fp16 ulp of the row'
    else:
        assert torch.equal(c0[:M], c1[:M]), 'tllm_gemm_stream differs from tllm_gemm'
    return {k: v[1:] for k, v in t.items()}, slices.value, note


NAME = {0: 'fp16', 1: 'weight-only int8', 2: 'weight-only int4', 3: 'SmoothQuant'}[WT]
say(f'Part 1: {NAME} GEMM, {"no" if F16 else "per-channel" if WOQ else "per-channel x per-token"} scales, fp16 output, {CUS} CUs; microseconds per call, median (min - max) of '
    f'{RUNS} runs of {REPS} calls between device events, tllm_gemm and the stream alternating, one warm-up run of each dropped; '
    f'calls rotate over {COPIES} copies of the weights; share = weight bytes / median time / 8 TB/s; spread = max - min of tllm_gemm')
for N, K in ((12288, 4096), (4096, 4096), (11008, 4096), (4096, 11008)) + ((HEAD, ) if F16 else ()):
    head = (N, K) == HEAD
    if head:
        say(f'the lm_head, fp32 logits, 4 copies; third route: ceil(M / 8) tllm_gemv slabs')
    for M in MS:
        t, slices, note = gemm_case(M, N, K, head)
        b, n = np.median(t['base']), np.median(t['new'])
        spread = max(t['base']) - min(t['base'])
        share = lambda us: N * K * WBYTES / (us * 1e-6) / 8e12
        text = (f'{N:5d} x {K:5d} M {M:2d}: tllm_gemm {b:7.1f} ({min(t["base"]):.1f} - {max(t["base"]):.1f}) {100 * share(b):4.1f} % | '
                f'stream ({slices} K-slices) {n:7.1f} ({min(t["new"]):.1f} - {max(t["new"]):.1f}) {100 * share(n):4.1f} % | {b / n:.2f} x, '
                f'gain {b - n:+.1f} us = {(b - n) / max(spread, 1e-9):+.1f} spreads')
        if head:
            sl = t['slabs']
            text += f' | GEMV slabs {np.median(sl):7.1f} ({min(sl):.1f} - {max(sl):.1f})'
        say(text + note)


def verify_passes(mode, int8_kv, base_keys, new_keys, base_name, new_name):
    cfg = dict(bench.LLAMA_7B, num_layers=32)
    V = cfg['vocab_size']
    stream = torch.cuda.current_stream().cuda_stream
    w = bench.synth_weights(torch, cfg, mode, int8_kv, 1, 0, dev)
    PAST, STEPS, PRUNS = 1024, 8, 7

    def event_ms(fn):
        return event_us(fn, 1) * 1e-3

    sess = {}
    for name, keys in (('base', dict(append_split=1, **base_keys)), ('stream', dict(append_split=1, **new_keys))):
        s = NativeSession(dict(cfg, quant_mode=bench.QM[mode] | (bench.INT8_KV if int8_kv else 0), tp_size=1, tp_rank=0, **keys))
        for k, t in w.items():
            s.set_tensor(k, t)
        s.finalize()
        s.setup(1, PAST, 512)
        sess[name] = s
    say(f'Part 2: the verify pass, 7B {mode} + {"int8" if int8_kv else "fp16"} KV, batch 1, synthetic weights, {PAST}-token cache, append_split = 1; ms, '
        f'median (min - max) of {PRUNS} runs between device events; the session {base_name} and {new_name} and graph steps alternating')
    r = np.random.default_rng(1)
    for n in (16, 32):
        for s in sess.values():
            s.fake_context(PAST, seed=3, stream=stream)
            s.step(2, use_graph=True, stream=stream)
        tv = dict(base=[], stream=[])
        ts = []
        for i in range(PRUNS + 1):
            ids = r.integers(3, V, (1, n)).astype(np.int32)
            for name, s in sess.items():
                tv[name].append(event_ms(lambda: s.verify(ids, stream=stream)))
            ts.append(event_ms(lambda: sess['base'].step(STEPS, use_graph=True, stream=stream)) / STEPS)
        a, b, st = np.median(tv['base'][1:]), np.median(tv['stream'][1:]), np.median(ts[1:])
        say(f'verify pass of n = {n:2d}: {base_name} {a:.3f} ({min(tv["base"][1:]):.3f} - {max(tv["base"][1:]):.3f}) | {new_name} {b:.3f} '
            f'({min(tv["stream"][1:]):.3f} - {max(tv["stream"][1:]):.3f}) | one step from the graph {st:.3f} | break-even acceptance '
            f'{a / st - 1:.2f} -> {b / st - 1:.2f} drafts kept per round')
    say(f'stream GEMM launches of the session {new_name} {sess["stream"].stream_gemm_launches()}, of the one {base_name} '
        f'{sess["base"].stream_gemm_launches()}')
    for s in sess.values():
        s.close()
    del w, sess
    torch.cuda.empty_cache()


if not args.no_pass:
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    if F16:
        verify_passes('fp16', False, {}, dict(stream_gemm=2), 'without the key', 'with stream_gemm = 2')
        verify_passes('sq', True, dict(stream_gemm=1), dict(stream_gemm=2), 'with stream_gemm = 1', 'with stream_gemm = 2')
    else:
        verify_passes({1: 'woq8', 2: 'woq4', 3: 'sq'}[WT], True, {}, dict(stream_gemm=1), 'without the key', 'with stream_gemm = 1')
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, 'w') as f:
    f.write('\n'.join(lines) + '\n')
