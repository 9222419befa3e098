"""The --sampled mode of tools/lookup_timing.py (its docstring says what is measured).  Not run on its own."""
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'tests'), ):
    sys.path.insert(0, p)

from tensorrt_llm.runtime import sampling_ref as SR  # noqa: E402
from tensorrt_llm.runtime.native import NativeSession, spec_accept, spec_sample_rows, token_logprobs  # noqa: E402

SAMPLING = dict(top_k=40, top_p=0.9, temperature=0.8, repetition_penalty=1.1)
# the configurations of tests/test_gpu_session_verify_sampled.py: generate_lookup on the trained parent, decode_lookup on the tiny fixture
LOOKUP_CFG = dict(top_k=40, temperature=0.8, repetition_penalty=1.1)
TINY_CFG = dict(top_k=2, temperature=0.8, repetition_penalty=1.1)
TINY_MODEL = dict(num_layers=2, num_heads=2, hidden_size=64, inter_size=24, vocab_size=128, max_position_embeddings=64,
                  rms_norm_eps=1e-6, quant_mode=0)
NEW, CHUNK = 48, 8


def median_us(fn, runs=21):
    t = []
    for _ in range(runs + 2):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b) * 1e3)
    t = t[2:]
    return float(np.median(t)), float(min(t))


def kernel_launches(say):
    V, S, smax = 32000, 64, 256
    r = np.random.default_rng(0)
    say(f'launches behind the head of a verify pass, batch 1, vocab {V}, us between device events, median (min) of 21, 2 warm-up runs '
        f'dropped; sampling {SAMPLING} (history bitmap + y staged in LDS), 100 tokens in the record')
    for n in (2, 8, 32):
        x = torch.from_numpy((r.standard_normal((n, V)) * 3).astype(np.float32)).cuda()
        ids = torch.from_numpy(r.integers(3, V, (1, n)).astype(np.int32)).cuda()
        rec = torch.from_numpy(r.integers(3, V, (1, smax)).astype(np.int32)).cuda()
        i32 = lambda v: torch.full((1, ), v, dtype=torch.int32, device='cuda')
        seq_len, fin, cur, lens = i32(S + 100), i32(0), i32(5), i32(S)
        draws = torch.zeros((1, n), dtype=torch.int32, device='cuda')
        targets = torch.cat([ids[0, 1:], i32(-1)]).contiguous()
        part = torch.empty((1, n, 8), dtype=torch.float32, device='cuda')
        t_rows = median_us(lambda: spec_sample_rows(x, ids, seq_len, draws, max_input_len=S, out_ids=rec, input_lengths=lens,
                                                    finished=fin, random_seed=1, **SAMPLING))
        t_lp = median_us(lambda: token_logprobs(x, targets, partials=part))
        top1 = token_logprobs(x, targets, partials=part)[2].reshape(1, n).contiguous()
        out = torch.zeros((1, V), dtype=torch.float32, device='cuda')

        def accept():
            seq_len.fill_(S + 100)
            spec_accept(ids, top1, logits=x, seq_len=seq_len, finished=fin, cur_ids=cur, out_ids=rec, logits_out=out, max_input_len=S)
        t_acc = median_us(accept)
        say(f'n = {n:2d}: sample rows {t_rows[0]:.1f} ({t_rows[1]:.1f}) | token_logprob partial + merge (with their output allocations) '
            f'{t_lp[0]:.1f} ({t_lp[1]:.1f}) | accept (with the reset of seq_len) {t_acc[0]:.1f} ({t_acc[1]:.1f})')


def verify_passes(s, cfg, stream, say, event_ms):
    V, n, past = cfg['vocab_size'], 8, 1024
    r = np.random.default_rng(2)
    res = {}
    for name, scfg in (('greedy', None), ('sampled', dict(SAMPLING, random_seed=3))):
        s.set_sampling(scfg)
        s.fake_context(past, seed=3, stream=stream)
        s.step(2, use_graph=False, stream=stream)
        t = []
        for _ in range(8):
            ids = r.integers(3, V, (1, n)).astype(np.int32)
            t.append(event_ms(lambda: s.verify(ids, sampled=scfg is not None, stream=stream)))
        res[name] = (float(np.median(t[1:])), min(t[1:]))
    s.set_sampling(None)
    say(f'7B SmoothQuant int8 + int8 KV, batch 1, {past}-token cache, verify pass of n = {n} as the caller sees it, ms, median (min) of 7: '
        f'greedy {res["greedy"][0]:.3f} ({res["greedy"][1]:.3f}) | sampled {res["sampled"][0]:.3f} ({res["sampled"][1]:.3f}) | '
        f'difference {1e3 * (res["sampled"][0] - res["greedy"][0]):.0f} us')


@functools.lru_cache(maxsize=None)
def parent_model():
    import trained_parents as TP
    return TP.quantised('deterministic', 'fp16')


def parent_session(batch, S, new):
    cfg, q = parent_model()
    s = NativeSession(dict(cfg, quant_mode=q['quant_mode']))
    for k, v in q['engine_tensors'].items():
        s.set_tensor(k, v)
    s.finalize()
    s.setup(batch, S, new)
    return s


def normalised_prefix(y, cand):
    yc = y[cand].astype(np.float64)
    w = np.exp(yc - yc.max())
    c = np.cumsum(w)
    return c / c[-1]


def tiny_session(batch, S, new):
    t = dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'hf_tiny_llama.npz')))
    s = NativeSession(TINY_MODEL)
    for k in t:
        if k.startswith('layers.') or k in ('vocab_embedding.weight', 'ln_f.weight', 'lm_head.weight'):
            s.set_tensor(k, t[k])
    s.finalize()
    s.setup(batch, S, new)
    return s


def path_difference(say, seed, tiny=False):
    """the largest distance, as a share of S, between the normalised prefix sums of the candidates' weights from a verify pass's
    rows and from the step logits, both on the same forced tokens: a sampled continuation (the engine's own, for `seed`) and the
    greedy one"""
    if tiny:
        t = np.load(os.path.join(ROOT, 'tests', 'golden', 'hf_tiny_llama.npz'))
        prompts, lengths, rows_of, scfg, new, open_session, what = t['ids'], t['input_lengths'], range(t['ids'].shape[0]), TINY_CFG, 16, \
            tiny_session, 'tiny HF fixture, fp16'
    else:
        import trained_parents as TP
        e = TP.load_eval('deterministic')
        prompts, lengths, rows_of, scfg, new, open_session, what = e['prompts'], e['lengths'], (0, 1, 6), LOOKUP_CFG, NEW, parent_session, \
            'deterministic trained parent, fp16'
    worst, count, worst_logit = 0.0, 0, 0.0
    for row in rows_of:
        L = int(lengths[row])
        ids, lens = prompts[row:row + 1, :L].astype(np.int32), np.array([L], np.int32)
        s = open_session(1, L, new + CHUNK)
        paths = {}
        s.set_sampling(dict(scfg, random_seed=seed))
        paths[f'seed {seed}'] = s.generate(ids, lens, new)[:, L:L + new]
        s.set_sampling(None)
        paths['greedy'] = s.generate(ids, lens, new)[:, L:L + new]
        for name, tok in paths.items():
            z_step, z_ver = [None] * (new + 1), [None] * (new + 1)  # z[g]: the distribution of token g (1-based)
            s.context(ids, lens)
            for g in range(1, new + 1):
                z_step[g] = s.logits()[0]
                if g < new:
                    s.force_tokens(tok[:, g - 1])
                    s.step(1, use_graph=False)
            s.context(ids, lens)
            pos = 0  # tok[pos] stands in the pending token's place; row i of the pass is the distribution of token pos + i + 2
            while pos + 1 < new:
                n = min(CHUNK, new - pos, L)
                acc, _ = s.verify(tok[:, pos:pos + n])
                rows = s.verify_logits(n)[0]
                for i in range(n):
                    if pos + i + 2 <= new:
                        z_ver[pos + i + 2] = rows[i]
                pos += int(acc[0]) + 1
            rc = SR.Config(**scfg)
            rec = np.concatenate([ids[0], tok[0]])
            for g in range(2, new + 1):
                h = SR.history_ids(rec, L, L, g)
                ys, yv = SR.transform(z_step[g], rc, g, -1, h), SR.transform(z_ver[g], rc, g, -1, h)
                cand = SR.order(ys)[:rc.effective(len(ys))[0]]
                d = float(np.abs(normalised_prefix(ys, cand) - normalised_prefix(yv, cand)).max())
                worst, count = max(worst, d), count + 1
                worst_logit = max(worst_logit, float(np.abs(z_ver[g] - z_step[g]).max()))
        s.close()
    say(f'path difference, {what}, {scfg}: {worst:.3e} of S over {count} rows (prompts {list(rows_of)} one at a time, forced along the '
        f'engine\'s sampled continuation for seed {seed} and along the greedy one, {new} tokens each; verify passes of up to {CHUNK} ids '
        f'against forced single steps; the candidates in the step logits\' order); largest |logit(verify row) - logit(step)| '
        f'{worst_logit:.4f}')
    return worst


def acceptance(say):
    import trained_parents as TP
    e = TP.load_eval('deterministic')
    rows = list(range(min(8, e['hf_logits'].shape[0])))
    for temp in (0.7, 1.0):
        tot = dict(rounds=0, verify_rounds=0, step_rounds=0, drafted=0, accepted=0)
        for row in rows:
            L = int(e['lengths'][row])
            ids, lens = e['prompts'][row:row + 1, :L].astype(np.int32), np.array([L], np.int32)
            s = parent_session(1, L, NEW + CHUNK)
            s.set_sampling(top_k=40, temperature=temp, random_seed=row)
            _, st = s.generate_lookup(ids, lens, NEW, num_draft_tokens=CHUNK, max_ngram=3, sampled=True)
            s.close()
            for k in tot:
                tot[k] += st[k]
        say(f'generate_lookup(sampled) on evaluation prompts {rows[0]}..{rows[-1]} of the deterministic parent, one at a time, {NEW} new '
            f'tokens, num_draft_tokens {CHUNK}, max_ngram 3, top_k 40, temperature {temp}, random_seed = prompt number: {tot["drafted"]} '
            f'drafts offered, {tot["accepted"]} kept ({100.0 * tot["accepted"] / max(tot["drafted"], 1):.0f} %), '
            f'{tot["rounds"]} passes ({tot["verify_rounds"]} verify + {tot["step_rounds"]} steps) for {NEW * len(rows)} tokens')


def run(s, cfg, stream, say, event_ms, seed, tiny_seed):
    say('speculative sampling by exact match (DESIGN.md section 7e); python tools/lookup_timing.py --sampled')
    kernel_launches(say)
    verify_passes(s, cfg, stream, say, event_ms)
    path_difference(say, seed)
    path_difference(say, tiny_seed, tiny=True)
    acceptance(say)
    say('not measured: batch > 1 in the timings, vocabularies that do not fit the LDS (the recomputing form), a stochastic parent, '
        'the whole generate_lookup loop against generate in wall time')
