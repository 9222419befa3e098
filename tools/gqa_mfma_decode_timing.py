"""What the grouped MFMA decode attention (tllm_attention_decode_grouped, csrc/kernels/mmha_gqa_mfma.hip: the query heads of a K/V
head as MFMA columns, every cache row requested once per K/V head) buys against the head-mapped launch: tllm_attention_decode at
query tile 1 - the default - and at tile 2, the best grouped tile of profiles/gqa_attention.txt, timed in the same run.  The method
is tools/gqa_timing.py's: per cell a graph of LAUNCHES back-to-back launches (ticket reset + attention, + combine where the plan
has one) replayed between two device events, ROUNDS rounds, the kernels in rotating order inside a round; median and min - max.
Cells: (H, Hkv) in (32, 8), (64, 8), (32, 1) at head size 128; fp16 and int8 cache; contexts 128 / 1024 / 4000; batch 1 and 8.
Verdict per cell: a win or a loss only where the medians differ by more than 3 spreads (max - min) of the tile-1 range, else a tie.
GPU only; writes profiles/gqa_mfma_decode.txt (or --out) - the bench.py ranges at its end are appended by hand from
`python bench.py` runs of the parent and of this tree, alternating.
    python tools/gqa_mfma_decode_timing.py"""
import argparse, ctypes, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'trtllm-llama_amd'))
import torch
from tensorrt_llm.plugin import capi
ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gqa_mfma_decode.txt'))
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--launches', type=int, default=200)
args = ap.parse_args()
assert torch.cuda.is_available(), 'gqa_mfma_decode_timing.py needs a GPU'
lib = capi.load_library()
side = torch.cuda.Stream(device=torch.device('cuda', 0))
torch.cuda.set_stream(side)
stream = side.cuda_stream
lines = []
KERNELS = ('tile 1', 'tile 2', 'mfma')


def say(s):
    print(s, flush=True)
    lines.append(s)


def make_call(B, H, Hkv, Dh, L, kind, tile):
    smax = 2048 if L < 2048 else 4096
    g = torch.Generator(device='cuda').manual_seed(1)
    keep = {}
    p = capi.AttentionParams(batch=B, num_heads=H, num_kv_heads=Hkv, head_size=Dh, rotary_dim=Dh, neox=1, q_scaling=1.0,
                             kv_cache_type=capi.HALF if kind == 'fp16' else capi.INT8, max_seq_len=smax, max_input_len=L, timestep=L,
                             q_heads_per_workgroup=tile)
    if kind == 'fp16':
        keep['kv_cache'] = torch.randn((B, 2, Hkv, smax, Dh), generator=g, device='cuda', dtype=torch.float16)
    else:
        keep['kv_cache'] = torch.randint(-127, 128, (B, 2, Hkv, smax, Dh), generator=g, device='cuda', dtype=torch.int8)
        keep['kv_scale_orig_quant'] = torch.tensor([20.0], device='cuda')
        keep['kv_scale_quant_orig'] = torch.tensor([0.05], device='cuda')
    keep['qkv'] = torch.randn((B, (H + 2 * Hkv) * Dh), generator=g, device='cuda', dtype=torch.float16)
    keep['sequence_length'] = torch.full((B, ), L, dtype=torch.int32, device='cuda')
    keep['input_lengths'] = torch.full((B, ), L, dtype=torch.int32, device='cuda')
    keep['out'] = torch.zeros((B, H * Dh), device='cuda', dtype=torch.float16)
    keep['workspace'] = torch.zeros(lib.tllm_attention_workspace_size(ctypes.byref(p), 0), dtype=torch.uint8, device='cuda')
    for k, t in keep.items():
        setattr(p, k, t.data_ptr())
    lay = [ctypes.c_int32() for _ in range(4)]
    assert lib.tllm_attention_decode_layout(ctypes.byref(p), *[ctypes.byref(x) for x in lay]) == 0, capi.last_error()
    return p, keep, [x.value for x in lay]


def launch(name, p, n):
    fn = lib.tllm_attention_decode_grouped if name == 'mfma' else lib.tllm_attention_decode
    for _ in range(n):
        assert fn(ctypes.byref(p), stream) == 0, capi.last_error()


def capture(name, p, n):
    """n launches as one graph: the replay has no host enqueue between the kernels"""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        launch(name, p, n)
    return g


def timed(g, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / n


say('decode attention launch, microseconds per launch: two device events around the replay of a graph of %d back-to-back launches' % args.launches)
say('(ticket reset + attention, + combine where stated); median [min - max] of %d rounds, kernels in rotating order inside a round.' % args.rounds)
say('tile 1 = tllm_attention_decode, head-mapped (the default); tile 2 = the same with 2 query heads per workgroup in turn; mfma =')
say('tllm_attention_decode_grouped.  "rows" = cache bytes the launch requests per sequence.  Verdict: mfma against tile 1, a win or a')
say('loss only beyond 3 x (max - min) of the tile-1 range.')
verdicts = []
for B in (1, 8):
    for kind in ('fp16', 'int8'):
        for (H, Hkv, Dh) in ((32, 8, 128), (64, 8, 128), (32, 1, 128)):
            G = H // Hkv
            for L in (128, 1024, 4000):
                calls = {k: make_call(B, H, Hkv, Dh, L, kind, 2 if k == 'tile 2' else 1) for k in KERNELS}
                outs = {}
                for k in KERNELS:  # warm-up: code objects, RoPE table, clocks
                    launch(k, calls[k][0], 20)
                    torch.cuda.synchronize()
                    outs[k] = calls[k][1]['out'].clone()
                graphs = {k: capture(k, calls[k][0], args.launches) for k in KERNELS}
                for k in KERNELS:
                    graphs[k].replay()
                torch.cuda.synchronize()
                # faster and different is not faster: every kernel computes what tile 1 computes (fp32 sums in another order at most)
                worst = max(float((outs[k].float() - outs['tile 1'].float()).abs().max()) for k in KERNELS)
                us = {k: [] for k in KERNELS}
                for r in range(args.rounds):
                    order = KERNELS[r % 3:] + KERNELS[:r % 3]
                    for k in order:
                        us[k].append(timed(graphs[k], args.launches))
                esz = 2 if kind == 'fp16' else 1
                base = statistics.median(us['tile 1'])
                spread = max(us['tile 1']) - min(us['tile 1'])
                once = 2 * Hkv * L * Dh * esz
                cell = f'B {B} {kind:4s} H {H:2d} Hkv {Hkv:2d} G {G:2d} ctx {L:4d}'
                for k in KERNELS:
                    tc, ns, _, merged = calls[k][2]
                    med = statistics.median(us[k])
                    rows = once * {'tile 1': G, 'tile 2': G // 2, 'mfma': (G + 15) // 16}[k]
                    say(f'{cell} {k:6s}: {med:7.2f} us [{min(us[k]):7.2f} - {max(us[k]):7.2f}] x{base / med:5.2f} vs tile 1 | rows '
                        f'{rows / 1e6:7.3f} MB (once {once / 1e6:6.3f} MB) | split {tc} x {min(L // tc + 1, ns)} of {ns}, '
                        f'{"in-launch" if merged else "combine"} | max |out - out(tile 1)| {worst:.1e}')
                d = base - statistics.median(us['mfma'])
                verdicts.append(f'{cell}: {"win" if d > 3 * spread else ("loss" if -d > 3 * spread else "tie")} '
                                f'({d:+.2f} us against 3 x {spread:.2f} us)')
say('')
say('verdict per cell, mfma against tile 1:')
for v in verdicts:
    say(v)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, 'w') as f:
    f.write('\n'.join(lines) + '\n')
