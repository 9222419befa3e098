"""What the query tile of the grouped-query decode attention buys: the decode attention launch (tllm_attention_decode: RoPE +
cache append + split-KV attention + merge), batch 1, timed in the same run for tile 1 - the head-mapped form, every query head
its own workgroup and its own load of the cache rows, the baseline - against each grouped tile (2, 4, 8 query heads of a K/V head
per workgroup, the rows loaded once per tile).  Shapes (H, Hkv, Dh): (32, 8, 128), (64, 8, 128), (32, 1, 128) and the multi-head
instance (32, 32, 128); contexts 128 / 1024 / 4000; fp16 and int8 cache.  Per cell: ROUNDS rounds, the tiles in rotating order
inside every round, a graph of LAUNCHES launches replayed between two device events per round; median and min - max over the rounds (the spread).
Bytes: the cache rows the launch requests (K and V rows of the context, once per tile: 2 * Hkv * (G / tile) * L * Dh * element
size) next to the 1 / G stream (tile = G).  GPU only; writes profiles/gqa_attention.txt (or --out).
    python tools/gqa_timing.py"""
import argparse, ctypes, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'trtllm-llama_amd'))
import torch
from tensorrt_llm.plugin import capi
ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gqa_attention.txt'))
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--launches', type=int, default=300)
args = ap.parse_args()
assert torch.cuda.is_available(), 'gqa_timing.py needs a GPU'
lib = capi.load_library()
dev = torch.device('cuda', 0)
side = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(side)
stream = side.cuda_stream
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def make_call(H, Hkv, Dh, L, kind, tile):
    smax = 2048 if L < 2048 else 4096
    g = torch.Generator(device='cuda').manual_seed(1)
    keep = {}
    p = capi.AttentionParams(batch=1, num_heads=H, num_kv_heads=Hkv, head_size=Dh, rotary_dim=Dh, neox=1, q_scaling=1.0,
                             kv_cache_type=capi.HALF if kind == 'fp16' else capi.INT8, max_seq_len=smax, max_input_len=L, timestep=L,
                             q_heads_per_workgroup=tile)
    if kind == 'fp16':
        keep['kv_cache'] = torch.randn((1, 2, Hkv, smax, Dh), generator=g, device='cuda', dtype=torch.float16)
    else:
        keep['kv_cache'] = torch.randint(-127, 128, (1, 2, Hkv, smax, Dh), generator=g, device='cuda', dtype=torch.int8)
        keep['kv_scale_orig_quant'] = torch.tensor([20.0], device='cuda')
        keep['kv_scale_quant_orig'] = torch.tensor([0.05], device='cuda')
    keep['qkv'] = torch.randn((1, (H + 2 * Hkv) * Dh), generator=g, device='cuda', dtype=torch.float16)
    keep['sequence_length'] = torch.tensor([L], dtype=torch.int32, device='cuda')
    keep['input_lengths'] = torch.tensor([L], dtype=torch.int32, device='cuda')
    keep['out'] = torch.zeros((1, H * Dh), device='cuda', dtype=torch.float16)
    keep['workspace'] = torch.zeros(lib.tllm_attention_workspace_size(ctypes.byref(p), 0), dtype=torch.uint8, device='cuda')
    for k, t in keep.items():
        setattr(p, k, t.data_ptr())
    lay = [ctypes.c_int32() for _ in range(4)]
    assert lib.tllm_attention_decode_layout(ctypes.byref(p), *[ctypes.byref(x) for x in lay]) == 0, capi.last_error()
    return p, keep, [x.value for x in lay]


def launch(p, n):
    for _ in range(n):
        assert lib.tllm_attention_decode(ctypes.byref(p), stream) == 0, capi.last_error()


def capture(p, n):
    """n launches as one graph: the replay has no host enqueue between the kernels"""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        launch(p, n)
    return g


def timed(g, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / n


say('decode attention launch, batch 1, microseconds per launch: two device events around the replay of a graph of %d back-to-back' % args.launches)
say('launches (ticket reset + attention, + combine where stated; no host enqueue in the window); median [min - max] of %d rounds,' % args.rounds)
say('tiles in rotating order inside a round.  tile 1 = head-mapped baseline.  "rows" = cache bytes the launch requests, "1/G" = the')
say('stream if every cache row were loaded once.  merge: in-launch = last-arriver merge inside the launch, combine = second launch.')
for kind in ('fp16', 'int8'):
    for (H, Hkv, Dh) in ((32, 8, 128), (64, 8, 128), (32, 1, 128), (32, 32, 128)):
        G = H // Hkv
        tiles = [t for t in (1, 2, 4, 8) if G % t == 0]
        for L in (128, 1024, 4000):
            calls = {t: make_call(H, Hkv, Dh, L, kind, t) for t in tiles}
            outs = {}
            for t in tiles:  # warm-up: code objects, RoPE table, clocks
                launch(calls[t][0], 30)
                torch.cuda.synchronize()
                outs[t] = calls[t][1]['out'].clone()
            graphs = {t: capture(calls[t][0], args.launches) for t in tiles}
            for t in tiles:
                graphs[t].replay()
            torch.cuda.synchronize()
            # faster and different is not faster: every tile computes what tile 1 computes (fp32 sums in another order at most)
            worst = max(float((outs[t].float() - outs[1].float()).abs().max()) for t in tiles)
            us = {t: [] for t in tiles}
            for r in range(args.rounds):
                order = tiles[r % len(tiles):] + tiles[:r % len(tiles)]
                for t in order:
                    us[t].append(timed(graphs[t], args.launches))
            esz = 2 if kind == 'fp16' else 1
            base = statistics.median(us[1])
            for t in tiles:
                tc, ns, qt, merged = calls[t][2]
                med = statistics.median(us[t])
                rows = 2 * Hkv * (G // t) * L * Dh * esz
                say(f'{kind:4s} H {H:2d} Hkv {Hkv:2d} G {G:2d} ctx {L:4d} tile {t}: {med:7.2f} us [{min(us[t]):7.2f} - {max(us[t]):7.2f}] '
                    f'x{base / med:5.2f} vs tile 1 | rows {rows / 1e6:7.3f} MB (1/G {2 * Hkv * L * Dh * esz / 1e6:6.3f} MB) '
                    f'{rows / med / 1e3:7.1f} GB/s | split {tc} x {min(L // tc + 1, ns)} of {ns}, {"in-launch" if merged else "combine"} '
                    f'| max |out - out(tile 1)| {worst:.1e}')
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, 'w') as f:
    f.write('\n'.join(lines) + '\n')
