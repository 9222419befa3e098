"""kernels/spec_decode.hip through its kernel-level entries (tllm_spec_accept, tllm_prompt_lookup): every output array held exactly
to tensorrt_llm/runtime/spec_ref.py on the cases tests/test_spec_ref.py pins on the CPU."""
import numpy as np
import pytest
import torch

from tensorrt_llm.runtime import native as N
from tensorrt_llm.runtime import spec_ref as R
from test_spec_ref import END, accept_cases, lookup_cases

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).to(DEV)


# ------------------------------------------------------------------------------------------------ accept
@pytest.mark.parametrize('vocab', [97, 128], ids=['vocab97-scalar-copy', 'vocab128-vector-copy'])
def test_spec_accept_equals_the_restatement(vocab):
    B, n, hidden, smax, max_in, half, table_len = 3, 5, 64, 24, 6, 16, 20
    r = np.random.default_rng(vocab)
    emb = r.standard_normal((vocab, hidden)).astype(np.float16)
    table = r.standard_normal((table_len, half, 2)).astype(np.float32)
    cases = accept_cases()
    cases = cases + cases[:(-len(cases)) % B]
    epoch = dev([41], np.int32)
    for g0 in range(0, len(cases), B):
        grp = cases[g0:g0 + B]
        seq_len = np.array([c[1] for c in grp], np.int32)
        fin = np.array([c[2] for c in grp], np.int32)
        t = np.array([c[3] for c in grp], np.int32)
        a = np.array([c[4] for c in grp], np.int32)
        has_limit = any(c[5] is not None for c in grp)
        limit = np.array([0x7FFFFFFF if c[5] is None else c[5] for c in grp], np.int32)
        in_len = np.array([4, 6, 1], np.int32)
        out_ids = r.integers(0, vocab, (B, smax)).astype(np.int32)
        cur = np.array([90, 91, 92], np.int32)
        logits = r.standard_normal((B * n, vocab)).astype(np.float32)
        want = R.accept(seq_len, fin, t, a, END, limit if has_limit else None, out_ids=out_ids, cur_ids=cur, input_lengths=in_len,
                        max_input_len=max_in, rope_table_len=table_len)
        d = dict(seq_len=dev(seq_len), finished=dev(fin), cur_ids=dev(cur), out_ids=dev(out_ids))
        accepted = dev(np.full(B, -9, np.int32))
        logits_out = dev(np.full((B, vocab), -5.0, np.float32))
        rope_row = dev(np.full((B, half, 2), -5.0, np.float32))
        rope_pos = dev(np.full(B, -1, np.int32))
        x_out = dev(np.full((B, hidden), 7.0, np.float16))
        N.spec_accept(dev(t), dev(a), logits=dev(logits), end_id=END, limit=dev(limit) if has_limit else None, accepted=accepted,
                      logits_out=logits_out, rope_row_out=rope_row, rope_pos_out=rope_pos, rope_table=dev(table),
                      input_lengths=dev(in_len), max_input_len=max_in, emb_table=dev(emb), x_out=x_out, step_epoch=epoch, **d)
        torch.cuda.synchronize()
        tag = [c[0] for c in grp]
        np.testing.assert_array_equal(accepted.cpu().numpy(), want['accepted'], err_msg=str(tag))
        assert list(want['accepted']) == [c[6][0] for c in grp]  # ... and the restatement gives what the CPU test pins
        for k in ('seq_len', 'finished', 'cur_ids', 'out_ids'):  # out_ids whole: the slots that must stay untouched included
            np.testing.assert_array_equal(d[k].cpu().numpy(), want[k], err_msg=f'{k} {tag}')
        np.testing.assert_array_equal(rope_pos.cpu().numpy(), want['rope_pos'], err_msg=str(tag))
        got_row, got_x, got_l = rope_row.cpu().numpy(), x_out.cpu().numpy(), logits_out.cpu().numpy()
        for b in range(B):
            m = want['accepted'][b]
            if m >= 0:
                np.testing.assert_array_equal(got_row[b], table[want['rope_pos'][b]], err_msg=tag[b])
                np.testing.assert_array_equal(got_x[b], emb[want['bonus'][b]], err_msg=tag[b])
                np.testing.assert_array_equal(got_l[b], logits[b * n + m], err_msg=tag[b])
            else:  # frozen: nothing written but the input row, put back from the unchanged current id
                assert (got_row[b] == -5.0).all() and (got_l[b] == -5.0).all(), tag[b]
                np.testing.assert_array_equal(got_x[b], emb[cur[b]], err_msg=tag[b])
        assert int(epoch.cpu()[0]) == 41 + g0 // B + 1  # once per launch


def test_spec_accept_guards_the_cache_capacity_and_the_vocabulary():
    """slots >= out_stride are not written, an arg-max id >= vocab gathers a zero row, the RoPE position is clamped"""
    B, n, vocab, hidden, smax = 1, 5, 97, 64, 12
    emb = np.ones((vocab, hidden), np.float16)
    out_ids = np.arange(smax, dtype=np.int32)[None] + 100
    d = dict(seq_len=dev([10], np.int32), finished=dev([0], np.int32), cur_ids=dev([0], np.int32), out_ids=dev(out_ids))
    t, a = np.array([[5, 6, 7, 8, 3]], np.int32), np.array([[6, 7, 8, 500, 4]], np.int32)
    x_out = dev(np.full((B, hidden), 7.0, np.float16))
    rope_pos = dev([-1], np.int32)
    table = np.zeros((4, 2, 2), np.float32)
    N.spec_accept(dev(t), dev(a), logits=dev(np.zeros((n, vocab), np.float32)), end_id=-1, emb_table=dev(emb), x_out=x_out,
                  rope_row_out=dev(np.zeros((1, 2, 2), np.float32)), rope_pos_out=rope_pos, rope_table=dev(table),
                  input_lengths=dev([6], np.int32), max_input_len=6, vocab=vocab, **d)
    torch.cuda.synchronize()
    want = R.accept([10], [0], t, a, -1, out_ids=out_ids)
    assert want['accepted'][0] == 3 and want['seq_len'][0] == 14
    np.testing.assert_array_equal(d['out_ids'].cpu().numpy(), want['out_ids'])  # slots 10, 11 written; 12 .. 14 do not exist
    assert int(d['seq_len'].cpu()[0]) == 14 and int(d['cur_ids'].cpu()[0]) == 500
    assert (x_out.cpu().numpy() == 0).all() and int(rope_pos.cpu()[0]) == 3


# ------------------------------------------------------------------------------------------------ prompt lookup
def lookup_both(rows, in_len, seq_len, n, g, max_in, vocab=512, finished=None, limit=None):
    opt = lambda v: None if v is None else dev(v, np.int32)
    ids, dl = N.prompt_lookup(dev(rows, np.int32), dev(seq_len, np.int32), n, g, max_input_len=max_in, vocab=vocab,
                              input_lengths=dev(in_len, np.int32), finished=opt(finished), limit=opt(limit))
    torch.cuda.synchronize()
    want_ids, want_dl = R.prompt_lookup(rows, in_len, max_in, seq_len, n, g, finished, limit)
    np.testing.assert_array_equal(dl.cpu().numpy(), want_dl, err_msg=f'draft_len n {n} g {g}')
    np.testing.assert_array_equal(ids.cpu().numpy(), want_ids, err_msg=f'ids n {n} g {g}')
    return want_ids, want_dl


@pytest.mark.parametrize('n', [2, 5, 8])
@pytest.mark.parametrize('g', [1, 3])
def test_prompt_lookup_equals_the_restatement(n, g):
    cases = lookup_cases()
    cases = cases + cases[:(-len(cases)) % 3]
    for g0 in range(0, len(cases), 3):
        grp = cases[g0:g0 + 3]
        rows = np.stack([c[1] for c in grp])
        assert rows.shape == (3, 40)
        in_len, seq_len = [c[2] for c in grp], [c[3] for c in grp]
        _, dl = lookup_both(rows, in_len, seq_len, n, g, 12)
        for c, got in zip(grp, dl):
            if (n, g) in c[4]:
                assert got == c[4][(n, g)][0], c[0]
        # frozen sequences get no draft: the first finished, the second at its limit, the third live under a limit
        lookup_both(rows, in_len, seq_len, n, g, 12, finished=[1, 0, 0], limit=[99, seq_len[1], seq_len[2] + 1])


def test_prompt_lookup_searches_more_starts_than_a_workgroup_has_threads():
    """one row of 4000 tokens over a small alphabet: every thread walks many candidate starts and the most recent match among
    all of them must win; a second row whose only match is the very first start"""
    r = np.random.default_rng(12)
    L, max_in, smax = 4000, 12, 4100
    rows = np.zeros((2, smax), np.int32)
    rows[0, :10] = r.integers(0, 6, 10)
    rows[0, 10:max_in] = 5  # padding slots: not part of the sequence
    rows[0, max_in:max_in + L - 10] = r.integers(0, 6, L - 10)
    rows[1, :max_in] = [400, 401, 402] + list(range(20, 29))
    rows[1, max_in:max_in + L - max_in] = r.integers(0, 6, L - max_in)
    rows[1, L - 3:L] = [400, 401, 402]  # (slot L - 1 is the pending token)
    in_len, seq_len = [10, max_in], [max_in + L - 10 - 1, L - 1]
    for n, g in ((8, 3), (5, 8), (32, 1)):
        lookup_both(rows, in_len, seq_len, n, g, max_in)
    ids, dl = lookup_both(rows, in_len, seq_len, 8, 3, max_in)
    assert dl[1] == 7 and list(ids[1, 1:4]) == [20, 21, 22]
