"""Choose the random seed of tests/test_gpu_session_verify_sampled.py on the CPU (no GPU needed).

generate_lookup(sampled=True) yields generate()'s tokens exactly in the rule but not in the arithmetic: a verify row's logits come
from the append pass's GEMMs and attention, a step's from the GEMVs, so a draw whose target lies within that difference of a
prefix-sum boundary may legitimately differ.  The test therefore uses a seed whose every draw keeps a distance from both ends of
its interval, and the distance is measured here, not on the code under test: oracle/llama_oracle.py runs the deterministic trained
parent (tests/golden/trained_llama, fp16 weights) step by step, sampling_ref.draw draws every token from the oracle's own logits
(teacher-forced along its own draws), and the margin of a draw is
    min(target - prefix[i - 1], prefix[i] - target) / S
(infinite where the configuration leaves one possible id; the lower end of the first candidate and the upper end of the last do
not count: a target cannot leave the candidates).  The margin of a seed is the smallest over the LOOKUP_NEW tokens of every sequence
of tests/test_spec_ref.py::LOOKUP_BATCHES.

    python tools/spec_sampling_seed_scan.py --seeds 300 [--temperature 0.8] [--top_k 40]

prints one line per seed (margin, and how many of its tokens differ from greedy, per batch) and the best seeds last.
--tiny --new 16: the same for the front-end test's tiny HF fixture (its two prompts as one batch)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'trtllm-llama_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

from oracle import llama_oracle as O  # noqa: E402
from tensorrt_llm.runtime import sampling_ref as SR  # noqa: E402
import trained_parents as TP  # noqa: E402
from test_spec_ref import LOOKUP_BATCHES, LOOKUP_NEW  # noqa: E402


def draw_margin(d: SR.Draw) -> float:
    if d.unique() or d.total <= 0:
        return float('inf')
    i, lo, hi = d.interval(d.token)
    m = float('inf')
    if i > 0:
        m = min(m, (d.target - lo) / d.total)
    if i < len(d.cand) - 1:
        m = min(m, (hi - d.target) / d.total)
    return m


TINY_CFG = dict(num_layers=2, num_heads=2, hidden_size=64, inter_size=24, vocab_size=128, rms_norm_eps=1e-6)


class Parent:
    def __init__(self, tiny=False):
        if tiny:  # the 2-layer HF fixture the front-end tests build their engine from (tests/golden/hf_tiny_llama.npz)
            t = dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'hf_tiny_llama.npz')))
            cfg, w = TINY_CFG, t
            self.prompts, self.lengths = t['ids'], t['input_lengths']
        else:
            cfg, w = TP.oracle_weights('deterministic')
            e = TP.load_eval('deterministic')
            self.prompts, self.lengths = e['prompts'], e['lengths']
        self.cfg, self.H = cfg, cfg['num_heads']
        f = lambda k: w[k].astype(np.float32)
        self.w = {k: f(k) for k in ('vocab_embedding.weight', 'ln_f.weight', 'lm_head.weight')}
        self.w['layers'] = [{k[len(f'layers.{i}.'):]: f(k) for k in w if k.startswith(f'layers.{i}.')} for i in range(cfg['num_layers'])]
        self.eps = cfg['rms_norm_eps']
        self.ctx = {}

    def batch(self, rows):
        lens = self.lengths[list(rows)].astype(np.int32)
        S = int(lens.max())
        ids = np.zeros((len(rows), S), np.int32)
        for i, b in enumerate(rows):
            ids[i, :lens[i]] = self.prompts[b, :lens[i]]
        return ids, lens

    def context(self, rows, new):
        """(logits of token 1, caches after the prompt): computed once per batch, copied per seed"""
        if rows not in self.ctx:
            ids, lens = self.batch(rows)
            B, S = ids.shape
            Dh = self.cfg['hidden_size'] // self.H
            caches = [np.zeros((B, 2, self.H, S + new, Dh), np.float16) for _ in range(self.cfg['num_layers'])]
            self.ctx[rows] = (O.llama_logits_context(ids, self.w, caches, lens, self.H, self.eps), caches)
        z, caches = self.ctx[rows]
        return z, [c.copy() for c in caches]

    def sampled_path(self, rows, cfg: SR.Config, new):
        """tokens [B, new] drawn from the oracle's own logits, and the smallest margin of any of the draws"""
        ids, lens = self.batch(rows)
        B, S = ids.shape
        z, caches = self.context(rows, new)
        masked = np.zeros((B, S + new), np.int32)
        for b in range(B):
            masked[b, lens[b]:S] = 1
        rec = np.zeros((B, S + new), np.int64)
        rec[:, :S] = ids
        worst = float('inf')
        for g in range(1, new + 1):
            for b in range(B):
                d = SR.draw(z[b], cfg, b, g, -1, SR.history_ids(rec[b], int(lens[b]), S, g))
                rec[b, S + g - 1] = d.token
                worst = min(worst, draw_margin(d))
            if g < new:
                t = S + g - 1
                z = O.llama_logits_decode(rec[:, t], self.w, caches, [t] * B, lens, S, t, self.H, masked, self.eps)
        return rec[:, S:].astype(np.int32), worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seeds', type=int, default=300)
    ap.add_argument('--first', type=int, default=0)
    ap.add_argument('--top_k', type=int, default=40)
    ap.add_argument('--top_p', type=float, default=0.9)
    ap.add_argument('--temperature', type=float, default=0.8)
    ap.add_argument('--repetition_penalty', type=float, default=1.1)
    ap.add_argument('--new', type=int, default=LOOKUP_NEW)
    ap.add_argument('--tiny', action='store_true', help='the tiny HF fixture and its own two prompts as one batch (the front-end test)')
    a = ap.parse_args()
    P = Parent(a.tiny)
    batches = ((0, 1), ) if a.tiny else LOOKUP_BATCHES
    greedy = {rows: P.sampled_path(rows, SR.Config(), a.new)[0] for rows in batches}
    res = []
    for seed in range(a.first, a.first + a.seeds):
        cfg = SR.Config(top_k=a.top_k, top_p=a.top_p, temperature=a.temperature, repetition_penalty=a.repetition_penalty, random_seed=seed)
        margin, off = float('inf'), []
        for rows in batches:
            tok, m = P.sampled_path(rows, cfg, a.new)
            margin = min(margin, m)
            off.append(int((tok != greedy[rows]).sum()))
        res.append((margin, seed, off))
        print(f'seed {seed}: smallest margin {margin:.3e} of S, {off} tokens differ from greedy (per batch)', flush=True)
    res.sort()
    print('best:')
    for margin, seed, off in res[-10:]:
        print(f'  seed {seed}: margin {margin:.3e}, {off} tokens differ from greedy')


if __name__ == '__main__':
    main()
