"""What the split-KV append attention (tllm_attention_append_split) costs against the kernel the rule picks, and what it does to the
verify pass - device events, medians with the spread, the two routes alternating in this process on this build.
  1. the attention call alone (RoPE + cache write, attention, and for SPLIT the merge), 7B extents: H 32, Dh 128, batch 1, int8 and
     fp16 cache, past 1024 and 4000; SPLIT against WAVE at n = 1, 2, 4, 8, 15 and against MFMA at n = 16, 32; one grouped shape
     (Hkv 8); a sweep over split_chunk behind the plan's constants;
  2. the verify pass of n = 2 / 4 / 8 / 16 ids with and without the session key append_split, in the format of
     profiles/prompt_lookup.txt (7B SmoothQuant int8 + int8 KV, batch 1, 1024-token cache), with the break-even acceptance.
Part 1 calls each entry 20 times on ONE cache, which then sits in the chip's caches; a pass walks 32 layers, each with a cache of its
own.  Part 1b repeats four rows with the calls rotating over 32 caches, as the layers of a pass do.
GPU only.    python tools/append_split_timing.py [--out profiles/append_split.txt] [--no_pass]
--paged [--tokens_per_block T]: the same three things on the paged cache (paged_report below) -> profiles/append_split_paged.txt
--trace_pass: nothing is timed - 8 verify passes of n = 2 on the keyless session, then 8 on the keyed one, for a kernel trace:
             rocprofv3 --kernel-trace --stats -d <dir> -- python tools/append_split_timing.py --trace_pass"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'trtllm-llama_amd'))
import torch, numpy as np
import bench
from tensorrt_llm.plugin import capi
from tensorrt_llm.runtime.native import (APPEND_ATTN_MFMA, APPEND_ATTN_WAVE, NativeSession, attention_append, attention_append_paged,
                                         attention_append_split, attention_append_split_layout, attention_append_split_paged)
ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None, help='profiles/append_split.txt, with --paged profiles/append_split_paged.txt')
ap.add_argument('--no_pass', action='store_true', help='part 1 alone')
ap.add_argument('--paged', action='store_true', help='the paged cache: attention call and verify pass of the paged session without '
                'the key, the paged session with append_split = 2 and the linear session with append_split = 1')
ap.add_argument('--tokens_per_block', type=int, default=64, help='with --paged: tokens per page')
ap.add_argument('--trace_pass', action='store_true', help='run verify passes for a kernel trace, time nothing')
args = ap.parse_args()
assert torch.cuda.is_available(), 'append_split_timing.py needs a GPU'
dev = torch.device('cuda', 0)
CUS = torch.cuda.get_device_properties(dev).multi_processor_count
RUNS, REPS = 9, 20
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def event_us(fn):
    """one run: REPS calls between two device events, microseconds per call"""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / REPS


def med(v):
    return f'{np.median(v):7.1f} ({min(v):.1f} - {max(v):.1f})'


def attention_case(kv, past, n, H=32, Hkv=32, Dh=128, chunks=(0, ), layers=1):
    """the two entries on the same buffers (sequence_length is not advanced by the launch: every call sees the same past); layers > 1:
    successive calls rotate over that many caches of the same content"""
    g = torch.Generator(device=dev).manual_seed(past + n)
    smax = past + 64
    qkv = torch.randn((1, n, (H + 2 * Hkv) * Dh), generator=g, device=dev, dtype=torch.float16)
    if kv == 'fp16':
        cache, code, sc = torch.randn((1, 2, Hkv, smax, Dh), generator=g, device=dev, dtype=torch.float16), 0, None
    else:
        cache = torch.randint(-127, 128, (1, 2, Hkv, smax, Dh), generator=g, device=dev, dtype=torch.int8)
        code, sc = capi.INT8, (torch.tensor([32.0], device=dev), torch.tensor([1 / 32.0], device=dev))
    caches, turn = [cache] + [cache.clone() for _ in range(layers - 1)], [0]

    def next_cache():
        turn[0] += 1
        return caches[turn[0] % layers]
    out = torch.empty((1, n, H * Dh), device=dev, dtype=torch.float16)
    seq = torch.tensor([past], dtype=torch.int32, device=dev)
    kw = dict(num_heads=H, num_kv_heads=Hkv, head_size=Dh, max_input_len=past, max_past=past, kv_cache_type=code,
              kv_scale_orig_quant=sc and sc[0], kv_scale_quant_orig=sc and sc[1])
    rule = APPEND_ATTN_MFMA if n >= 16 else APPEND_ATTN_WAVE
    ws = torch.empty(attention_append_split_layout(n, Dh, batch=1, num_heads=H, num_kv_heads=Hkv, max_keys=past, split_chunk=64)[2],
                     dtype=torch.uint8, device=dev)  # (chunk 64: the most ranges any chunk of the sweep needs)
    base = lambda: attention_append(qkv, next_cache(), out, seq, seq, append_kernel=rule, **kw)
    t = {c: [] for c in ('rule', ) + tuple(chunks)}
    for i in range(RUNS + 1):
        t['rule'].append(event_us(base))
        for c in chunks:
            t[c].append(event_us(lambda: attention_append_split(qkv, next_cache(), out, seq, seq, split_chunk=c, workspace=ws, **kw)))
    return {k: v[1:] for k, v in t.items()}, ('MFMA' if n >= 16 else 'WAVE')


def paged_report(T):
    """--paged: the attention call and the verify pass on the paged cache, three routes alternating in one run - the paged session
    without append_split (what a paged session ran before the paged split instance: the WAVE kernel at n < 16), the paged session
    with append_split = 2, the linear session with append_split = 1 - at pasts 1024 and 4000, n = 2 / 4 / 8"""
    H, Dh, NS = 32, 128, (2, 4, 8)
    sc = torch.tensor([32.0], device=dev), torch.tensor([1 / 32.0], device=dev)
    say(f'Part 1: the attention call alone (RoPE + cache write launch, attention launch, SPLIT: + merge launch), int8 cache, batch 1, '
        f'H {H}, Dh {Dh}, T = {T}, {CUS} CUs; microseconds per call, median (min - max) of {RUNS} runs of {REPS} calls between device '
        'events, the routes alternating, one warm-up run of each dropped; the pages of the sequence scattered over the pool, and the same '
        'pool with its pages in ascending order')
    for past in (1024, 4000):
        smax = (past + 64 + T - 1) // T * T
        M = smax // T
        cache = torch.randint(-127, 128, (1, 2, H, smax, Dh), device=dev, dtype=torch.int8)
        pool = torch.randint(-127, 128, (2 * M, H, T, Dh), device=dev, dtype=torch.int8)
        order, nbytes = torch.randperm(M), H * T * Dh
        table = torch.stack([pool.data_ptr() + order * nbytes, pool.data_ptr() + (M + order) * nbytes]).view(1, 2, M).to(dev)
        order = torch.arange(M)  # the same pool with its pages in ascending order: what the scatter costs, apart from the table
        table_asc = torch.stack([pool.data_ptr() + order * nbytes, pool.data_ptr() + (M + order) * nbytes]).view(1, 2, M).to(dev)
        seq = torch.tensor([past], dtype=torch.int32, device=dev)
        for n in NS:
            qkv = (torch.randn((1, n, 3 * H * Dh), device=dev) * 0.5).half()
            out = torch.empty((1, n, H * Dh), device=dev, dtype=torch.float16)
            kw = dict(num_heads=H, head_size=Dh, max_input_len=past, max_past=past, kv_cache_type=capi.INT8, kv_scale_orig_quant=sc[0],
                      kv_scale_quant_orig=sc[1])
            ws = torch.empty(attention_append_split_layout(n, Dh, batch=1, num_heads=H, max_keys=past, cus=CUS)[2], dtype=torch.uint8,
                             device=dev)
            pg = dict(tokens_per_block=T, max_seq_len=smax, **kw)
            routes = dict(wave=lambda: attention_append_paged(qkv, pool, table, out, seq, seq, append_kernel=APPEND_ATTN_WAVE, **pg),
                          split=lambda: attention_append_split_paged(qkv, pool, table, out, seq, seq, workspace=ws, **pg),
                          asc=lambda: attention_append_split_paged(qkv, pool, table_asc, out, seq, seq, workspace=ws, **pg),
                          linear=lambda: attention_append_split(qkv, cache, out, seq, seq, workspace=ws, **kw))
            t = {k: [] for k in routes}
            for i in range(RUNS + 1):
                for k, fn in routes.items():
                    t[k].append(event_us(fn))
            t = {k: v[1:] for k, v in t.items()}
            say(f'int8 past {past:4d} n {n}: paged WAVE {med(t["wave"])} | paged SPLIT {med(t["split"])} | pages in order '
                f'{med(t["asc"])} | linear SPLIT {med(t["linear"])} | '
                f'WAVE / paged SPLIT {np.median(t["wave"]) / np.median(t["split"]):.2f} x, paged / linear SPLIT '
                f'{np.median(t["split"]) / np.median(t["linear"]):.3f}')
    if args.no_pass:
        return
    cfg = dict(bench.LLAMA_7B, num_layers=32)
    V = cfg['vocab_size']
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    stream = torch.cuda.current_stream().cuda_stream
    w = bench.synth_weights(torch, cfg, 'sq', True, 1, 0, dev)
    STEPS, PRUNS = 8, 7
    paged = dict(paged_kv_cache=1, tokens_per_block=T, paged_append=1)
    sess = {}
    for name, keys in (('paged', paged), ('paged2', dict(paged, append_split=2)), ('linear1', dict(append_split=1))):
        s = NativeSession(dict(cfg, quant_mode=bench.QM['sq'] | bench.INT8_KV, tp_size=1, tp_rank=0, **keys))
        for k, t in w.items():
            s.set_tensor(k, t)
        s.finalize()
        sess[name] = s

    def event_ms(fn):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    say(f'Part 2: the verify pass, 7B SmoothQuant int8 + int8 KV, batch 1, synthetic weights, T = {T}; ms, median (min - max) of {PRUNS} '
        'runs between device events, one warm-up run dropped; the paged session without append_split, the paged session with '
        'append_split = 2, the linear session with append_split = 1 and graph steps of the paged session alternating')
    r = np.random.default_rng(1)
    fm = lambda v: f'{np.median(v):.3f} ({min(v):.3f} - {max(v):.3f})'
    for past in (1024, 4000):
        for s in sess.values():
            s.setup(1, past, 512)
        for n in NS:
            for s in sess.values():
                s.fake_context(past, seed=3, stream=stream)
                s.step(2, use_graph=True, stream=stream)
            tv, ts = {k: [] for k in sess}, []
            for i in range(PRUNS + 1):
                ids = r.integers(3, V, (1, n)).astype(np.int32)
                for name, s in sess.items():
                    tv[name].append(event_ms(lambda: s.verify(ids, stream=stream)))
                ts.append(event_ms(lambda: sess['paged'].step(STEPS, use_graph=True, stream=stream)) / STEPS)
            tv, st = {k: v[1:] for k, v in tv.items()}, np.median(ts[1:])
            say(f'past {past:4d} verify pass of n = {n}: paged {fm(tv["paged"])} | paged append_split = 2 {fm(tv["paged2"])} | linear '
                f'append_split = 1 {fm(tv["linear1"])} | one paged step from the graph {st:.3f} | break-even '
                + ' -> '.join(f'{np.median(tv[k]) / st - 1:.2f}' for k in ('paged', 'paged2')) + ' drafts kept per round')
    say('split launches: ' + ', '.join(f'{k} {s.append_split_launches()}' for k, s in sess.items())
        + '; append launches (wave, mfma): ' + ', '.join(f'{k} {s.append_launches()}' for k, s in sess.items()))
    for s in sess.values():
        s.close()


if args.paged:
    paged_report(args.tokens_per_block)
    with open(args.out or os.path.join(ROOT, 'profiles', 'append_split_paged.txt'), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    sys.exit(0)
args.out = args.out or os.path.join(ROOT, 'profiles', 'append_split.txt')

if not args.trace_pass:
    say(f'Part 1: the attention call alone (RoPE + cache write launch, attention launch, SPLIT: + merge launch), batch 1, H 32, Dh 128, '
        f'{CUS} CUs; microseconds per call, median (min - max) of {RUNS} runs of {REPS} calls between device events, the rule\'s kernel '
        'and SPLIT alternating, one warm-up run of each dropped')
    for kv in ('int8', 'fp16'):
        for past in (1024, 4000):
            for n in (1, 2, 4, 8, 15, 16, 32):
                t, name = attention_case(kv, past, n)
                chunk, ranges, _ = attention_append_split_layout(n, 128, batch=1, num_heads=32, max_keys=past, cus=CUS)
                say(f'{kv:4s} past {past:4d} n {n:2d}: {name} {med(t["rule"])} | SPLIT (plan: chunk {chunk}, {ranges} ranges) {med(t[0])} | '
                    f'{np.median(t["rule"]) / np.median(t[0]):.2f} x')
    say('Part 1b: the same call rotating over 32 caches (int8, past 1024), as the 32 layers of a pass do:')
    for n in (2, 8, 16, 32):
        t, name = attention_case('int8', 1024, n, layers=32)
        say(f'int8 past 1024 n {n:2d}, 32 caches: {name} {med(t["rule"])} | SPLIT {med(t[0])} | {np.median(t["rule"]) / np.median(t[0]):.2f} x')
    say('grouped heads, H 32 on Hkv 8 (G = 4: n * 4 columns to a K/V head), int8 cache, past 1024:')
    for n in (2, 8, 16):
        t, name = attention_case('int8', 1024, n, Hkv=8)
        say(f'int8 past 1024 n {n:2d} Hkv 8: {name} {med(t["rule"])} | SPLIT {med(t[0])} | {np.median(t["rule"]) / np.median(t[0]):.2f} x')
    say('split_chunk sweep (int8 cache; 0 = the plan):')
    for past in (1024, 4000):
        for n in (2, 8):
            chunks = (0, 64, 128, 256, 512, 1024)
            t, _ = attention_case('int8', past, n, chunks=chunks)
            say(f'int8 past {past:4d} n {n}: ' + ' | '.join(f'chunk {c}: {np.median(t[c]):.1f}' for c in chunks))

if args.trace_pass or not args.no_pass:
    cfg = dict(bench.LLAMA_7B, num_layers=32)
    V = cfg['vocab_size']
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    stream = torch.cuda.current_stream().cuda_stream
    w = bench.synth_weights(torch, cfg, 'sq', True, 1, 0, dev)
    PAST, STEPS, PRUNS = 1024, 8, 7

    def event_ms(fn):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    sess = {}
    for name, keys in (('rule', {}), ('split', dict(append_split=1))):
        s = NativeSession(dict(cfg, quant_mode=bench.QM['sq'] | bench.INT8_KV, tp_size=1, tp_rank=0, **keys))
        for k, t in w.items():
            s.set_tensor(k, t)
        s.finalize()
        s.setup(1, PAST, 512)
        sess[name] = s
    if args.trace_pass:
        r = np.random.default_rng(1)
        for s in sess.values():  # keyless first, then keyed: the trace's attention kernels tell them apart
            s.fake_context(PAST, seed=3, stream=stream)
            for i in range(8):
                s.verify(r.integers(3, V, (1, 2)).astype(np.int32), stream=stream)
            s.close()
        sys.exit(0)
    say(f'Part 2: the verify pass, 7B SmoothQuant int8 + int8 KV, batch 1, synthetic weights, {PAST}-token cache; ms, median (min) of '
        f'{PRUNS} runs between device events; the keyless session, the session with append_split = 1 and graph steps alternating')
    r = np.random.default_rng(1)
    for n in (2, 4, 8, 16):
        for s in sess.values():
            s.fake_context(PAST, seed=3, stream=stream)
            s.step(2, use_graph=True, stream=stream)
        tv = dict(rule=[], split=[])
        ts = []
        for i in range(PRUNS + 1):
            ids = r.integers(3, V, (1, n)).astype(np.int32)
            for name, s in sess.items():
                tv[name].append(event_ms(lambda: s.verify(ids, stream=stream)))
            ts.append(event_ms(lambda: sess['rule'].step(STEPS, use_graph=True, stream=stream)) / STEPS)
        a, b, st = np.median(tv['rule'][1:]), np.median(tv['split'][1:]), np.median(ts[1:])
        say(f'verify pass of n = {n:2d}: rule {a:.3f} ({min(tv["rule"][1:]):.3f}) | append_split {b:.3f} ({min(tv["split"][1:]):.3f}) | '
            f'one step from the graph {st:.3f} | break-even acceptance {a / st - 1:.2f} -> {b / st - 1:.2f} drafts kept per round')
    say(f'split launches of the keyed session {sess["split"].append_split_launches()}, of the keyless one '
        f'{sess["rule"].append_split_launches()}')
    for s in sess.values():
        s.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, 'w') as f:
    f.write('\n'.join(lines) + '\n')
