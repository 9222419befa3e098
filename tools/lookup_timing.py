"""What one verify pass of speculative greedy decoding costs (tllm_session_verify) against the generation step it competes with, on
the benchmark's 7B SmoothQuant int8 + int8 KV configuration, batch 1, synthetic weights, behind a 1024-token cache - device events,
medians of 7 runs, the two routes alternating in this process on this build:
    verify pass of n = 2, 4, 8, 16 ids   | one generation step replayed from the graph (the mean of 8)
and from the two the break-even acceptance  t_verify(n) / t_step - 1: the drafts a verify round must keep, on average, to beat
plain steps (a round that keeps m drafts yields m + 1 tokens for t_verify; m + 1 steps cost (m + 1) t_step).
The verify pass is timed as the caller sees it: the copy of the ids, the read of sequence_length ahead of the pass, the pass, the
accept step and the read-back of its result.
GPU only.    python tools/lookup_timing.py [--out profiles/prompt_lookup.txt]

--sampled: speculative sampling by exact match instead -> profiles/spec_sampling.txt:
  * the sample-rows launch at n = 2 / 8 / 32, vocab 32000, batch 1, beside the token_logprob and accept launches it joins;
  * a sampled verify pass against a greedy one on the 7B configuration above (n = 8);
  * the path difference on the deterministic trained parent (fp16): the largest distance, as a share of S, between the prefix sums
    from the verify rows (the append pass's GEMMs) and from the step logits (the GEMVs) on the same forced tokens - what the margin of
    the seed of tests/test_gpu_session_verify_sampled.py is held against - and the same on the tiny fixture of its front-end test;
  * drafts offered and kept by generate_lookup(sampled=True) on the parent's evaluation prompts at temperature 0.7 and 1.0.
             python tools/lookup_timing.py --sampled [--seed N] [--out profiles/spec_sampling.txt]"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'trtllm-llama_amd'))
import torch, numpy as np
import bench
from tensorrt_llm.runtime.native import NativeSession
ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None)
ap.add_argument('--sampled', action='store_true')
ap.add_argument('--seed', type=int, default=125, help='--sampled: the seed whose sampled continuation is one of the forced paths')
ap.add_argument('--tiny_seed', type=int, default=112, help='--sampled: the same for the tiny fixture')
args = ap.parse_args()
args.out = args.out or os.path.join(ROOT, 'profiles', 'spec_sampling.txt' if args.sampled else 'prompt_lookup.txt')
assert torch.cuda.is_available(), 'lookup_timing.py needs a GPU'
cfg = dict(bench.LLAMA_7B, num_layers=32)
V = cfg['vocab_size']
dev = torch.device('cuda', 0)
torch.cuda.set_stream(torch.cuda.Stream(device=dev))
stream = torch.cuda.current_stream().cuda_stream
mode, int8_kv = 'sq', True
w = bench.synth_weights(torch, cfg, mode, int8_kv, 1, 0, dev)
RUNS, STEPS, PAST = 7, 8, 1024
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def event_ms(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


s = NativeSession(dict(cfg, quant_mode=bench.QM[mode] | bench.INT8_KV, tp_size=1, tp_rank=0))
for k, t in w.items():
    s.set_tensor(k, t)
s.finalize()
s.setup(1, PAST, 512)
r = np.random.default_rng(1)
if args.sampled:
    import lookup_timing_sampled
    lookup_timing_sampled.run(s, cfg, stream, say, event_ms, args.seed, args.tiny_seed)
    s.close()
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    sys.exit(0)
say(f'7B SmoothQuant int8 + int8 KV, batch 1, synthetic weights, {PAST}-token cache (tllm_session_fake_context); ms, median (min) of '
    f'{RUNS} runs between device events, verify pass and graph steps alternating, one warm-up run of each dropped')
say(f'decode form {s.decode_form()} (bit 0: projection + attention in one launch, bit 1: + the O-projection); the verify pass runs the '
    'separate-launch prefill schedule with the wave-per-query append attention (n < 16) or the MFMA one (n = 16)')
rows = []
for n in (2, 4, 8, 16):
    s.fake_context(PAST, seed=3, stream=stream)  # every n starts behind the same cache length
    s.step(2, use_graph=True, stream=stream)     # captures the step graph
    tv, ts, kept = [], [], []
    for i in range(RUNS + 1):
        ids = r.integers(3, V, (1, n)).astype(np.int32)
        box = {}
        tv.append(event_ms(lambda: box.update(acc=s.verify(ids, stream=stream)[0])))
        kept.append(int(box['acc'][0]))
        ts.append(event_ms(lambda: s.step(STEPS, use_graph=True, stream=stream)) / STEPS)
    tv, ts = tv[1:], ts[1:]
    wave, mfma = s.append_launches()
    length = int(s.step_state()['sequence_length'][0])
    mv, ms = float(np.median(tv)), float(np.median(ts))
    rows.append((n, mv, ms))
    say(f'verify pass of n = {n:2d}: {mv:.3f} ({min(tv):.3f}) | one step from the graph: {ms:.3f} ({min(ts):.3f}) | '
        f't_verify / t_step = {mv / ms:.2f}, break-even acceptance {mv / ms - 1:.2f} drafts kept per round (of {n - 1} offered) | '
        f'cache length at the end {length}, drafts kept in these runs (random ids) {sorted(set(kept))}')
say('reading: a verify round keeps m drafts and yields m + 1 tokens; it beats m + 1 plain steps when m > t_verify / t_step - 1.')
worst = max(rows, key=lambda q: q[1] / q[2])
say(f'the pass costs {min(q[1] / q[2] for q in rows):.2f} to {worst[1] / worst[2]:.2f} steps: '
    + ('more than the weights alone would explain (a step streams them once, and so does a pass of n <= 8 rows through the skinny '
       'GEMV) - the separate launches of the prefill schedule and the wave-per-query append attention are what is left'
       if worst[1] / worst[2] > 1.5 else 'close to one weight stream, as a pass of n <= 8 rows through the skinny GEMV should'))
say('not measured: batch > 1, other weight modes and cache types, cache lengths other than 1024, n = 32, real text (acceptance '
    'rates of prompt lookup on a trained model), the whole generate_lookup loop')
s.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, 'w') as f:
    f.write('\n'.join(lines) + '\n')
