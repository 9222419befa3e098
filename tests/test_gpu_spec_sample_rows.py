"""GPU tests of the sampler on all rows of a verify pass (csrc/kernels/sampling.hip spec_sample_rows_kernel, through
tllm_spec_sample_rows; the rule: kernels.h SpecSampleParams).

(a) every draw and every u is BIT-EQUAL to what tllm_sample_tokens - the step kernel - returns for the same logits row, the
    history with t[0..i] written into it and the same g: the two kernels share the row draw and its integer weight sums;
(b) every draw lies in the interval of spec_ref.sample_rows (check_draw and TOL of tests/test_gpu_sampling.py: the derivation of
    TOL there is per row and does not depend on which kernel ran it);
(c) the logits are bitwise untouched; (d) the rows of frozen sequences hold end_id; (e) guard words behind draws and u_out are
    intact.

Shapes: vocab 32000 (y staged in LDS beside the bitmap), 40000 (does not fit: recomputed in every pass), 1003 (a bitmap tail word,
rows that are no multiple of 16 bytes).  Batch 3, ragged prompts under max_input_len 10, another seq_len per sequence, in every case
one sequence live, one finished and one at its limit - the roles rotate over the cases - and n in {1, 2, 5, 32}."""
import numpy as np
import pytest

from tensorrt_llm.runtime import sampling_ref as SR
from tensorrt_llm.runtime import spec_ref as R
from tensorrt_llm.runtime.native import sample_tokens, spec_sample_rows
from test_gpu_sampling import check_draw

pytestmark = pytest.mark.gpu

B, S, SMAX, END = 3, 10, 72, 2
IN_LEN = np.array([10, 6, 8], np.int32)
SEQ_LEN = np.array([14, 11, 19], np.int32)
GUARD_I, GUARD_F = -77, -3.5
NS = (1, 2, 5, 32)
# min_length None: set per case so that the mask ends inside the rows of the live sequence
CONFIGS = [dict(top_k=40, top_p=0.9, temperature=0.8, repetition_penalty=1.1), dict(top_k=0, top_p=0.7),
           dict(top_k=1, presence_penalty=1.5), dict(top_k=8, min_length=None), dict(top_k=0, top_p=0.9, repetition_penalty=1.3,
                                                                                   min_length=None)]


def case(V, n, ci):
    r = np.random.default_rng(V * 131 + n * 7 + ci)
    x = (r.standard_normal((B * n, V)) * 3.0).astype(np.float32)
    x[:, END] += 9.0  # end_id among the likely ids: min_length has something to mask, a draw can be end_id
    likely = np.argsort(-x, axis=1)[:, :16]
    rec = r.integers(0, min(V, 300), (B, SMAX)).astype(np.int32)
    ids = np.zeros((B, n), np.int32)
    for b in range(B):
        p = int(SEQ_LEN[b])
        rec[b, S:p] = likely[b * n, :p - S]  # likely ids in the record: the penalties move the draw
        rec[b, IN_LEN[b]:S] = likely[b * n, 0]  # ... and in the padding slots, where they must not count
        rec[b, p:] = likely[b * n, 1]          # slots the pass has not committed: never read
        ids[b] = [likely[b * n + min(i + 1, n - 1), i % 4] for i in range(n)]
    rec[0, 1], rec[1, S], rec[2, 0] = -5, V + 3, 0x7fffffff  # ids outside [0, vocab) are skipped
    live = (ci + n) % 3
    fin = np.zeros(B, np.int32)
    fin[(live + 1) % 3] = 1
    limit = SEQ_LEN + 100
    limit[(live + 2) % 3] = SEQ_LEN[(live + 2) % 3]
    return x, ids, rec, fin, limit.astype(np.int32), live


def run_rows(x, ids, rec, fin, limit, cfg, n, vocab=None, **kw):
    import torch
    dev = torch.from_numpy(x).cuda()
    before = dev.clone()
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()
    draws = torch.full((B * n + 8, ), GUARD_I, dtype=torch.int32, device='cuda')
    u = torch.full((B * n + 8, ), GUARD_F, dtype=torch.float32, device='cuda')
    spec_sample_rows(dev, t32(ids), t32(SEQ_LEN), draws, max_input_len=S, vocab=vocab, end_id=END, out_ids=t32(rec),
                     input_lengths=t32(IN_LEN), finished=t32(fin), limit=t32(limit), u_out=u, **kw, **cfg)
    torch.cuda.synchronize()
    assert torch.equal(before.view(torch.int32), dev.view(torch.int32)), 'the logits must not be written'  # (c)
    draws, u = draws.cpu().numpy(), u.cpu().numpy()
    assert (draws[B * n:] == GUARD_I).all() and (u[B * n:] == np.float32(GUARD_F)).all()  # (e)
    return draws[:B * n].reshape(B, n), u[:B * n].reshape(B, n)


def step_kernel_rows(x, ids, rec, cfg, n):
    """the existing step kernel on the same rows: for every i one call on the B rows (b, i), the history = the record with t[0..i]
    written into slots p .. p + i, g = p + i + 2 - S (row index = b, so the variate is the sequence's)"""
    import torch
    tok, uu = np.zeros((B, n), np.int32), np.zeros((B, n), np.float32)
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()
    in_len = t32(IN_LEN)
    for i in range(n):
        h = np.array(rec)
        for b in range(B):
            h[b, SEQ_LEN[b]:SEQ_LEN[b] + i + 1] = ids[b, :i + 1]
        rows = torch.from_numpy(np.ascontiguousarray(x.reshape(B, n, -1)[:, i])).cuda()
        out = torch.zeros(B, dtype=torch.int32, device='cuda')
        u = torch.zeros(B, dtype=torch.float32, device='cuda')
        sample_tokens(rows, t32(SEQ_LEN + i + 2 - S), out, end_id=END, history=t32(h), input_lengths=in_len, max_input_len=S, u_out=u,
                      **cfg)
        tok[:, i], uu[:, i] = out.cpu().numpy(), u.cpu().numpy()
    return tok, uu


@pytest.mark.parametrize('V', [32000, 40000, 1003])
def test_rows_equal_the_step_kernel_bit_for_bit_and_follow_the_rule(V):
    worst = 0.0
    for n in NS:
        for ci, cfg in enumerate(CONFIGS):
            x, ids, rec, fin, limit, live = case(V, n, ci)
            cfg = dict(cfg, random_seed=500 + ci)
            if 'min_length' in cfg:  # the live sequence draws g = g0 .. g0 + n - 1: end_id is masked for its first rows only
                cfg['min_length'] = int(SEQ_LEN[live]) + 2 - S + min(2, n - 1)
            draws, u = run_rows(x, ids, rec, fin, limit, cfg, n)
            frozen = [b for b in range(B) if b != live]
            assert (draws[frozen] == END).all(), f'V={V} n={n} {cfg}: frozen rows hold end_id'  # (d)
            # (a) the step kernel on the live sequence's rows, history with t[0..i], same g
            tok, us = step_kernel_rows(x, ids, rec, cfg, n)
            np.testing.assert_array_equal(draws[live], tok[live], err_msg=f'V={V} n={n} {cfg}')
            np.testing.assert_array_equal(u[live].view(np.uint32), us[live].view(np.uint32))
            # (b) the rule
            rc = SR.Config(**cfg)
            p = int(SEQ_LEN[live])
            want = R.sample_rows(x.reshape(B, n, V)[live], rc, live, p, ids[live], rec[live], int(IN_LEN[live]), S, END)
            for i, d in enumerate(want):
                assert np.float32(d.u).tobytes() == u[live, i].tobytes()
                worst = max(worst, check_draw(d, int(draws[live, i]), f'V={V} n={n} {cfg} row ({live}, {i})'))
            for b in frozen:
                assert R.sample_rows(x.reshape(B, n, V)[b], rc, b, int(SEQ_LEN[b]), ids[b], rec[b], int(IN_LEN[b]), S, END,
                                     finished=int(fin[b]), limit=int(limit[b])) == [None] * n
            if 'min_length' in cfg and n >= 5:  # the mask held for the first rows and not for the later ones
                g = p + 2 - S + np.arange(n)
                assert (draws[live][g < cfg['min_length']] != END).all()
            # the same arguments again: bit-reproducible
            again, _ = run_rows(x, ids, rec, fin, limit, cfg, n)
            np.testing.assert_array_equal(draws, again)
    print(f'[spec sample rows] V={V}: largest excess {worst:.3e} of S')


def test_every_sequence_live_and_a_draw_does_not_depend_on_n_or_on_the_other_rows():
    """All three sequences live, no limit, no finished array: row (b, i) of a pass of 5 is row (b, i) of a pass of 32 over the same
    leading rows - a draw is a function of its own row, history and (seed, b, g)."""
    import torch
    V, cfg = 1003, dict(top_k=40, top_p=0.9, temperature=0.8, repetition_penalty=1.1, random_seed=3)
    x, ids, rec, _, _, _ = case(V, 32, 0)
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()
    got = {}
    for n in (5, 32):
        xs = np.ascontiguousarray(x.reshape(B, 32, V)[:, :n]).reshape(B * n, V)
        draws = torch.full((B, n), GUARD_I, dtype=torch.int32, device='cuda')
        spec_sample_rows(torch.from_numpy(xs).cuda(), t32(ids[:, :n]), t32(SEQ_LEN), draws, max_input_len=S, end_id=END, out_ids=t32(rec),
                         input_lengths=t32(IN_LEN), **cfg)
        torch.cuda.synchronize()
        got[n] = draws.cpu().numpy()
        rc = SR.Config(**cfg)
        for b in range(B):
            want = R.sample_rows(xs.reshape(B, n, V)[b], rc, b, int(SEQ_LEN[b]), ids[b, :n], rec[b], int(IN_LEN[b]), S, END)
            for i, d in enumerate(want):
                check_draw(d, int(got[n][b, i]), f'all live n={n} row ({b}, {i})')
    np.testing.assert_array_equal(got[5], got[32][:, :5])


def test_refusals():
    import torch
    V, n = 257, 2
    x, ids, rec, fin, limit, _ = case(V, n, 0)
    cfg = dict(top_k=4)
    with pytest.raises(RuntimeError, match=r'n 33 outside \[1, 32\]'):
        z = torch.zeros((B * 33, V), dtype=torch.float32, device='cuda')
        i32 = torch.zeros((B, 33), dtype=torch.int32, device='cuda')
        spec_sample_rows(z, i32, torch.from_numpy(SEQ_LEN).cuda(), torch.zeros(B * 33, dtype=torch.int32, device='cuda'),
                         max_input_len=S, **cfg)
    with pytest.raises(RuntimeError, match='one vocabulary part'):
        run_rows(x, ids, rec, fin, limit, cfg, n, nparts=2)
    with pytest.raises(RuntimeError, match='history'):  # a penalty without the record
        dev = torch.from_numpy(x).cuda()
        spec_sample_rows(dev, torch.from_numpy(ids).cuda(), torch.from_numpy(SEQ_LEN).cuda(),
                         torch.zeros(B * n, dtype=torch.int32, device='cuda'), max_input_len=S, top_k=4, repetition_penalty=1.2)
    with pytest.raises(RuntimeError, match='mutually exclusive'):
        run_rows(x, ids, rec, fin, limit, dict(top_k=4, repetition_penalty=1.2, presence_penalty=0.5), n)
