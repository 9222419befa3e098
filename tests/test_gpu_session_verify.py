"""tllm_session_verify on the deterministic trained parent (tests/trained_parents.py), prompts 0 and 1 (110 and 64 tokens: a ragged
batch): the verify pass against what defines it - force_tokens + step over the same ids in a second session - and against HF's
teacher-forced logits within the bound of tests/trained_parents.py, K_ALGORITHM x (the restated algorithm's own error) + A_FP16.

Why arg-max equality with HF's tokens is an exact requirement for fp16 and woq8 + int8 cache, and not for SmoothQuant, is checked
on the CPU below (test_margins_...): the parent's top-2 margin is >= 5.6 at every step; an engine within bound b of HF keeps HF's
arg-max while 2 b < margin.  The fp16 / woq8 bounds are a few tenths; SmoothQuant's oracle error of 2.4 gives 3.1, and 6.2 > 5.6."""
import functools

import numpy as np
import pytest

import trained_parents as TP
from tensorrt_llm.runtime import spec_ref as R
from test_gpu_score import load_tiny, quant_session, tiny_session

N_VERIFY, KEPT, PLAIN = 6, (5, 2), 4
STEPS = 1 + N_VERIFY + PLAIN  # logits rows of HF's path the test looks at
NEW = 16                      # setup's max_new_tokens
EXACT_MODES = ('fp16', 'woq8_int8kv')


@functools.lru_cache(maxsize=None)
def prompts():
    ids, lens, hf_tokens, hf_logits, _ = TP.teacher_forced_prompts('deterministic', 2)
    assert lens.tolist() == [110, 64]
    return ids, lens, hf_tokens, hf_logits


@functools.lru_cache(maxsize=None)
def case(mode):
    """(cfg, qmodel, bound): bound = K x max |oracle - HF| + A over the STEPS rows of both prompts"""
    ids, lens, hf_tokens, hf_logits = prompts()
    cfg, qmodel = TP.quantised('deterministic', mode)
    z = TP.oracle_logits(qmodel, ids, lens, hf_tokens, STEPS)
    err = float(np.abs(z - hf_logits[:, :STEPS]).max())
    bound = TP.K_ALGORITHM * err + TP.A_FP16
    print(f'[verify {mode}] oracle error {err:.4f} -> bound {bound:.4f}')
    return cfg, qmodel, bound


def feed_ids(pending, hf_tokens, vocab):
    """[pending, hf_tokens[b][1 .. k_b], wrong ...]: the drafts of sequence b are right up to k_b"""
    f = np.zeros((2, N_VERIFY), np.int32)
    for b in range(2):
        f[b, 0] = pending[b]
        for i in range(1, N_VERIFY):
            f[b, i] = hf_tokens[b, i] if i <= KEPT[b] else (hf_tokens[b, i] + 1) % vocab
    return f


def log_softmax(x):
    x = x.astype(np.float64)
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def within(got, ref, bound, tag):
    d = float(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)).max())
    print(f'[{tag}] max |d| {d:.4f} (bound {bound:.4f})')
    assert d <= bound, f'{tag}: {d:.4f} > {bound:.4f}'


def row_state(s, b, upto):
    st = s.step_state()
    return [s.output_ids()[b, :upto]] + [st[k][b] for k in ('sequence_length', 'next_position', 'masked_tokens', 'input_lengths')]


# ------------------------------------------------------------------------------------------------ CPU: why the checks are sound
def test_margins_make_argmax_equality_exact_for_fp16_and_woq8_but_not_for_smoothquant():
    e = TP.load_eval('deterministic')
    top2 = np.sort(e['hf_logits'][:8], axis=-1)[..., -2:]
    margin = float((top2[..., 1] - top2[..., 0]).min())
    print(f'[verify] smallest top-2 margin of the first 8 prompts {margin:.3f}')
    assert margin >= 5.6
    for mode in EXACT_MODES:
        assert 2 * case(mode)[2] < margin, mode
    assert 2 * case('sq_static_int8kv')[2] > margin  # SmoothQuant is held to logits only


def test_the_append_rule_itself_stays_under_half_the_bound_with_the_int8_cache():
    """The verify pass reads its own n ids un-quantised where teacher-forced steps read them from the int8 cache.
    tests/append_rule_model.py runs that rule in numpy: its logits behind 3 and behind 6 appended ids (the rows the GPU test reads,
    m = 2 of prompt 1 and m = 5 of prompt 0) must stay within half the bound of the oracle's teacher-forced logits, so that the
    GPU test has the other half for the kernels."""
    from append_rule_model import append_logits
    ids, lens, hf_tokens, _ = prompts()
    cfg, qmodel, bound = case('woq8_int8kv')
    for b, n in ((1, KEPT[1] + 1), (0, KEPT[0] + 1)):
        got, ref = append_logits(qmodel, ids, lens, hf_tokens[:, :n])
        d = float(np.abs(got[b].astype(np.float64) - np.asarray(ref)[b]).max())
        print(f'[verify headroom] prompt {b}, {n} ids: rule vs oracle {d:.4f} = {d / bound:.2f} of the bound {bound:.4f}')
        assert d <= 0.5 * bound


# ------------------------------------------------------------------------------------------------ GPU
def open_sessions(cfg, qmodel, count):
    ids, lens, _, _ = prompts()
    out = []
    for _ in range(count):
        s = quant_session(cfg, qmodel)
        s.setup(2, ids.shape[1], NEW)
        s.context(ids, lens)
        out.append(s)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('mode', EXACT_MODES)
def test_verify_equals_forced_steps_and_hf(mode):
    ids, lens, hf_tokens, hf_logits = prompts()
    cfg, qmodel, bound = case(mode)
    S, V = ids.shape[1], cfg['vocab_size']
    a, b, c = open_sessions(cfg, qmodel, 3)  # a: verify; b: force_tokens + step over the same ids; c: plain greedy steps
    pending = a.output_ids()[:, S]
    np.testing.assert_array_equal(pending, hf_tokens[:, 0])
    feed = feed_ids(pending, hf_tokens, V)
    epoch = a.step_epoch()
    acc, lp = a.verify(feed)
    assert acc.tolist() == list(KEPT)
    assert a.step_epoch() == epoch + 1
    np.testing.assert_array_equal(acc, R.accept([S, S], [0, 0], feed, a.verify_top1(N_VERIFY))['accepted'])
    la = a.logits()
    # route B, snapshots behind every step
    forced, states = [], []
    for i in range(N_VERIFY):
        b.force_tokens(feed[:, i])
        b.step(1, use_graph=i >= 2)
        forced.append(b.logits())
        states.append([row_state(b, q, S + i + 2) for q in range(2)])
    for q in range(2):
        m = KEPT[q]
        for got, want, name in zip(row_state(a, q, S + m + 2), states[m][q], ('output_ids', 'sequence_length', 'next_position',
                                                                             'masked_tokens', 'input_lengths')):
            np.testing.assert_array_equal(got, want, err_msg=f'sequence {q} {name}')
        assert a.step_state()['sequence_length'][q] == S + m + 1
        np.testing.assert_array_equal(a.output_ids()[q, S:S + m + 2], hf_tokens[q, :m + 2])
        within(la[q], hf_logits[q, m + 1], bound, f'{mode} verify logits, sequence {q} row {m} vs HF')
        within(la[q], forced[m][q], bound, f'{mode} verify logits, sequence {q} row {m} vs forced steps')
    assert (lp[:, 0] == 0).all()
    for i in range(1, N_VERIFY):
        want = log_softmax(forced[i - 1])[np.arange(2), feed[:, i]]
        within(lp[:, i], want, bound, f'{mode} log_probs of id {i}')
    # four plain steps behind the verify pass: the rejected rows left in the cache are never read
    free = [c.logits()]
    for j in range(max(KEPT) + 1 + PLAIN):
        c.step(1, use_graph=j >= 2)
        free.append(c.logits())  # free[j] = the distribution of token j
    for i in range(1, PLAIN + 1):
        a.step(1, use_graph=i >= 2)
        la = a.logits()
        for q in range(2):
            t = KEPT[q] + 1 + i
            within(la[q], hf_logits[q, t], bound, f'{mode} plain step {i}, sequence {q} vs HF')
            within(la[q], free[t][q], bound, f'{mode} plain step {i}, sequence {q} vs the greedy session')
    for q in range(2):
        upto = S + KEPT[q] + 1 + PLAIN + 1
        np.testing.assert_array_equal(a.output_ids()[q, :upto], c.output_ids()[q, :upto])
        np.testing.assert_array_equal(a.output_ids()[q, S:upto], hf_tokens[q, :upto - S])
    for s in (a, b, c):
        s.close()


@pytest.mark.gpu
def test_smoothquant_is_held_to_logits_and_to_the_rule_on_its_own_argmax():
    mode = 'sq_static_int8kv'
    ids, lens, hf_tokens, hf_logits = prompts()
    cfg, qmodel, bound = case(mode)
    S, V = ids.shape[1], cfg['vocab_size']
    a, = open_sessions(cfg, qmodel, 1)
    feed = feed_ids(hf_tokens[:, 0], hf_tokens, V)  # HF's own token first: every row up to k_b is on HF's path
    acc, lp = a.verify(feed)
    top1 = a.verify_top1(N_VERIFY)
    want = R.accept([S, S], [0, 0], feed, top1)
    np.testing.assert_array_equal(acc, want['accepted'])
    np.testing.assert_array_equal(a.step_state()['sequence_length'], want['seq_len'])
    la = a.logits()
    for q in range(2):
        m = int(acc[q])
        print(f'[verify {mode}] sequence {q}: accepted {m} of {KEPT[q]} right drafts')
        if m <= KEPT[q]:  # (beyond it the row is behind a wrong id, where HF's path says nothing)
            within(la[q], hf_logits[q, m + 1], bound, f'{mode} verify logits, sequence {q} row {m} vs HF')
        for i in range(1, KEPT[q] + 2):
            if i < N_VERIFY:
                within(lp[q, i], log_softmax(hf_logits[q, i])[feed[q, i]], bound, f'{mode} log_prob of id {i}, sequence {q}')
    a.close()


@pytest.mark.gpu
def test_a_frozen_sequence_reports_minus_one_and_is_bit_unchanged():
    ids, lens, hf_tokens, _ = prompts()
    cfg, qmodel, _ = case('fp16')
    S = ids.shape[1]
    s = quant_session(cfg, qmodel)
    s.setup(2, S, NEW)
    end_id = int(hf_tokens[0, 3])
    assert end_id not in hf_tokens[1, :12].tolist() and end_id not in hf_tokens[0, :3].tolist()
    s.generate(ids, lens, 6, end_id=end_id)  # sequence 0 finishes with its fourth token; sequence 1 holds six
    before = row_state(s, 0, S + NEW), s.logits()[0]
    p = S + 5
    assert s.step_state()['sequence_length'].tolist() == [p, p]
    feed = np.stack([np.full(4, end_id, np.int32), hf_tokens[1, 5:9]]).astype(np.int32)
    acc, lp = s.verify(feed)
    assert acc.tolist() == [-1, 3]
    for got, want in zip(row_state(s, 0, S + NEW), before[0]):
        np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(s.logits()[0], before[1])
    np.testing.assert_array_equal(s.output_ids()[1, S:p + 5], hf_tokens[1, :10])
    # the pass used the next step's input row as scratch: a step behind it still sees the finished sequence's own token
    s.step(1)
    assert s.output_ids()[0, p + 1] == end_id and s.output_ids()[1, p + 5] == hf_tokens[1, 10]
    s.close()


@pytest.mark.gpu
def test_refusals():
    t, w = load_tiny()
    ids, lens = t['ids'], t['input_lengths']
    B, S = ids.shape
    new = 6
    tok = np.full((B, 2), 5, np.int32)
    s = tiny_session(w)
    with pytest.raises(RuntimeError, match='setup'):
        s.verify(tok)
    s.setup(B, S, new)
    with pytest.raises(RuntimeError, match='context'):
        s.verify(tok)
    s.context(ids, lens)
    before = s.output_ids(), s.step_state(), s.logits()
    with pytest.raises(RuntimeError, match='TLLM_VERIFY_MAX_TOKENS'):
        s.verify(np.full((B, 33), 5, np.int32))
    with pytest.raises(RuntimeError, match='capacity'):  # p + n + 1 > max_seq_len: no slot for the new pending token
        s.verify(np.full((B, new), 5, np.int32))
    s.set_sampling(top_k=40)
    with pytest.raises(RuntimeError, match='speculative sampling is not built'):
        s.verify(tok)
    s.set_sampling(None)
    after = s.output_ids(), s.step_state(), s.logits()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[2], after[2])
    for k in before[1]:
        assert np.array_equal(before[1][k], after[1][k]), k
    acc, _ = s.verify(np.full((B, new - 1), 5, np.int32))  # exactly up to the capacity is served
    assert (acc >= 0).all() and (s.step_state()['sequence_length'] <= S + new - 1).all()
    s.close()
    for keys, beam in ((dict(paged_kv_cache=1, tokens_per_block=16), 1), ({}, 2)):
        s = tiny_session(w, **keys)
        s.setup(B, S, new, beam)
        s.context(ids, lens)
        with pytest.raises(RuntimeError, match='not built'):
            s.verify(np.full((B, 2), 5, np.int32))
        s.close()
