"""What the weight-streaming GEMM (tllm_gemm_stream, 9 <= M <= 64 rows; --wtype 3 SmoothQuant, 1 / 2 weight-only int8 / int4: fp16
activations and scales, results compared within 2 fp16 ulp of the row's largest output and not bit for bit, part 2 on the
weight-only session) costs against the dispatch of tllm_gemm on the same operands, and what the session key stream_gemm does to the verify pass - device events, medians with the spread, the two routes
alternating in this process on this build.
  1. the four 7B SmoothQuant shapes (N x K: 12288 x 4096, 4096 x 4096, 11008 x 4096, 4096 x 11008), per-channel x per-token scales,
     fp16 output, M = 9, 16, 24, 32, 48, 64: microseconds per call and weight bytes / time as a share of 8 TB/s.  Successive calls
     rotate over 8 copies of the weights (400 MB and more: no copy is in a cache when its turn comes, as in a pass over 32 layers);
  2. the verify pass of n = 16 / 32 ids with and without the key (7B SmoothQuant int8 + int8 KV, batch 1, 1024-token cache,
     append_split = 1 on both), beside one step from the graph, with the break-even acceptance.
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
ap.add_argument('--wtype', type=int, default=3, choices=[1, 2, 3], help='1 / 2 weight-only int8 / int4, 3 SmoothQuant')
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
WOQ, WBYTES = WT != 3, 0.5 if WT == 2 else 1.0  # weight-only: fp16 A and scales; bytes per weight
MS = (9, 16, 24, 32, 48, 64) if WT == 3 else (16, 32, 48, 64)
lines = []


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


def gemm_case(M, N, K):
    g = torch.Generator(device=dev).manual_seed(N + K + M)
    ldw = int(K * WBYTES)  # any byte is a valid u8 / pair of nibbles
    a = torch.randn((64, K), generator=g, device=dev).half() if WOQ else torch.randint(-127, 128, (64, K), generator=g, device=dev, dtype=torch.int8)
    ws_ = [torch.randint(-127, 128, (N, ldw), generator=g, device=dev, dtype=torch.int8) for _ in range(COPIES)]
    sc = torch.rand((N, ), generator=g, device=dev) * 1e-5
    sc = (sc * 1e3).half() if WOQ else sc
    sr = torch.rand((64, ), generator=g, device=dev)
    c0, c1 = torch.zeros((64, N), device=dev, dtype=torch.float16), torch.zeros((64, N), device=dev, dtype=torch.float16)
    q = lambda w, c: capi.GemmParams(wtype=WT, out_dtype=1, M=M, N=N, K=K, a=a.data_ptr(), lda=K, w=w.data_ptr(), ldw=ldw,
                                     scale_col=sc.data_ptr(), scale_row=sr.data_ptr(), per_channel=1, per_token=1, c=c.data_ptr(), ldc=N)
    nbytes, slices = ctypes.c_int64(), ctypes.c_int32()
    assert lib.tllm_gemm_stream_layout(ctypes.byref(q(ws_[0], c0)), CUS, ctypes.byref(nbytes), ctypes.byref(slices), *[None] * 5) == 0
    work = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    turn = [0]

    def base():
        turn[0] += 1
        assert lib.tllm_gemm(ctypes.byref(q(ws_[turn[0] % COPIES], c0)), stream) == 0, capi.last_error()

    def new():
        turn[0] += 1
        assert lib.tllm_gemm_stream(ctypes.byref(q(ws_[turn[0] % COPIES], c1)), None, work.data_ptr(), work.numel(), stream) == 0, \
            capi.last_error()
    t = dict(base=[], new=[])
    for i in range(RUNS + 1):
        t['base'].append(event_us(base))
        t['new'].append(event_us(new))
    # the same weights last: the two routes agree bit for bit
    turn[0] = -1
    base()
    turn[0] = -1
    new()
    torch.cuda.synchronize()
    if WOQ:
        d, top = (c0[:M].float() - c1[:M].float()).abs().amax(1), c0[:M].float().abs().amax(1)
        assert bool((d <= top * 2.0 ** -9).all()), 'tllm_gemm_stream differs from tllm_gemm by more than 2 fp16 ulp of the row'
    else:
        assert torch.equal(c0[:M], c1[:M]), 'tllm_gemm_stream differs from tllm_gemm'
    return {k: v[1:] for k, v in t.items()}, slices.value


say(f'Part 1: {({1: "weight-only int8", 2: "weight-only int4", 3: "SmoothQuant"})[WT]} GEMM, per-channel{"" if WOQ else " x per-token"} scales, fp16 output, {CUS} CUs; microseconds per call, median (min - max) of '
    f'{RUNS} runs of {REPS} calls between device events, tllm_gemm and tllm_gemm_stream alternating, one warm-up run of each dropped; '
    f'calls rotate over {COPIES} copies of the weights; share = weight bytes / median time / 8 TB/s; spread = max - min of tllm_gemm')
for N, K in ((12288, 4096), (4096, 4096), (11008, 4096), (4096, 11008)):
    for M in MS:
        t, slices = gemm_case(M, N, K)
        b, n = np.median(t['base']), np.median(t['new'])
        spread = max(t['base']) - min(t['base'])
        share = lambda us: N * K * WBYTES / (us * 1e-6) / 8e12
        say(f'{N:5d} x {K:5d} M {M:2d}: tllm_gemm {b:7.1f} ({min(t["base"]):.1f} - {max(t["base"]):.1f}) {100 * share(b):4.1f} % | '
            f'stream ({slices} K-slices) {n:7.1f} ({min(t["new"]):.1f} - {max(t["new"]):.1f}) {100 * share(n):4.1f} % | {b / n:.2f} x, '
            f'gain {b - n:+.1f} us = {(b - n) / max(spread, 1e-9):+.1f} spreads')

if not args.no_pass:
    cfg = dict(bench.LLAMA_7B, num_layers=32)
    V = cfg['vocab_size']
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    stream = torch.cuda.current_stream().cuda_stream
    MODE = {1: 'woq8', 2: 'woq4', 3: 'sq'}[WT]
    w = bench.synth_weights(torch, cfg, MODE, True, 1, 0, dev)
    PAST, STEPS, PRUNS = 1024, 8, 7

    def event_ms(fn):
        return event_us(fn, 1) * 1e-3

    sess = {}
    for name, keys in (('base', dict(append_split=1)), ('stream', dict(append_split=1, stream_gemm=1))):
        s = NativeSession(dict(cfg, quant_mode=bench.QM[MODE] | bench.INT8_KV, tp_size=1, tp_rank=0, **keys))
        for k, t in w.items():
            s.set_tensor(k, t)
        s.finalize()
        s.setup(1, PAST, 512)
        sess[name] = s
    say(f'Part 2: the verify pass, 7B {MODE} + int8 KV, batch 1, synthetic weights, {PAST}-token cache, append_split = 1; ms, '
        f'median (min - max) of {PRUNS} runs between device events; the session without and with stream_gemm = 1 and graph steps alternating')
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
        say(f'verify pass of n = {n:2d}: without {a:.3f} ({min(tv["base"][1:]):.3f} - {max(tv["base"][1:]):.3f}) | stream_gemm {b:.3f} '
            f'({min(tv["stream"][1:]):.3f} - {max(tv["stream"][1:]):.3f}) | one step from the graph {st:.3f} | break-even acceptance '
            f'{a / st - 1:.2f} -> {b / st - 1:.2f} drafts kept per round')
    say(f'stream GEMM launches of the keyed session {sess["stream"].stream_gemm_launches()}, of the keyless one '
        f'{sess["base"].stream_gemm_launches()}')
    for s in sess.values():
        s.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, 'w') as f:
    f.write('\n'.join(lines) + '\n')
