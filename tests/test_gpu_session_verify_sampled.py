"""Speculative sampling by exact match through the session: tllm_session_verify_sampled on the synthetic
2-layer model of tests/test_gpu_sampling.py (fp16 and SmoothQuant), tllm_session_generate_lookup_sampled on the deterministic
trained parent, and the front-end.

The verify pass is held to the rule on the engine's OWN logits rows (verify_logits): every draw of verify_draws lies in the interval
of spec_ref.sample_rows (check_draw and TOL of tests/test_gpu_sampling.py), and everything the pass commits equals spec_ref.accept
fed with those draws, exactly.

generate_lookup(sampled=True) against generate().  The equality is exact in the rule, not in the arithmetic: a verify row's logits
come from the append pass's GEMMs and attention, a step's from the GEMVs, so a draw whose target lies within that difference of a
prefix-sum boundary may legitimately differ.  The seed is therefore chosen on the CPU, not on the code under test
(tools/spec_sampling_seed_scan.py --seeds 300 --top_p 0: oracle/llama_oracle.py on the trained parent, sampling_ref.draw,
teacher-forced along its own draws, seeds 0 .. 299 at top_k 40 / temperature 0.8 / repetition_penalty 1.1): SEED = 125, whose
smallest margin - the distance of any draw's target from both ends of its interval, as a share of S, over the 48 tokens of every
sequence of LOOKUP_BATCHES - is 9.012e-4, the largest of the 164 seeds whose tokens are not the greedy ones (45 of its 96 tokens of
batch (0, 1) differ from greedy; the seeds that stay on the greedy path reach 5.7e-2 and would test less).  The path difference,
measured once on an MI355X (tools/lookup_timing.py --sampled, profiles/spec_sampling.txt): the largest distance, as a share of S,
between the prefix sums from the verify rows and from the step logits on the same forced tokens is 2.567e-5 (largest logit
difference 0.0074).  The margin is 35 x that; at least 4 x is required - the headroom TOL takes over its derived error in
tests/test_gpu_sampling.py - and asserted below.  Temperature 0.8 / top_k 40 did not have to be lowered.

The front-end test runs on the tiny random HF fixture, whose distributions are flat, so the same logit difference moves the prefix
sums much further: at top_k 40 the best of 60 seeds keeps a margin of 9.4e-4, and seed 42 (7.2e-4) did differ from decode() in one
run.  That test therefore draws from top_k 2 - one boundary per draw - where seed 112 keeps 7.475e-2 (--tiny --new 16 --top_k 2
--top_p 0 --seeds 200) and the path difference, measured in the same run as above, is 4.654e-4 of S: 160 x."""
import functools

import numpy as np
import pytest

import trained_parents as TP
from tensorrt_llm.runtime import sampling_ref as SR
from tensorrt_llm.runtime import spec_ref as R
from tensorrt_llm.runtime.native import APPEND_ATTN_MFMA, attention_append_kernel
from test_gpu_sampling import SAMPLING, build, check_draw, check_session_step
from test_gpu_score import load_tiny, quant_session, tiny_session
from test_spec_ref import LOOKUP_BATCHES, LOOKUP_G, LOOKUP_N, LOOKUP_NEW

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------ the verify pass
S20, NEW = 20, 44  # max_input_len 20: a pass of 17 ids fits the activation buffers; the prompts of build() are 10 / 6 / 8 long
WARM = 2           # generated tokens in the record before the pass


def synthetic(mode, scfg):
    s, cfg, ids10, lens = build(mode)
    ids = np.full((ids10.shape[0], S20), 2, np.int32)
    ids[:, :ids10.shape[1]] = ids10
    s.setup(ids.shape[0], S20, NEW)
    if scfg is not None:
        s.set_sampling(scfg)
    return s, cfg, ids, lens


def start(s, ids, lens):
    """context + WARM steps; returns (record, sequence lengths, pending tokens)"""
    s.context(ids, lens)
    s.step(WARM, use_graph=False)
    out, p = s.output_ids(), s.step_state()['sequence_length']
    return out, p, np.array([out[b, p[b]] for b in range(out.shape[0])], np.int32)


def check_pass(s, rc, feed, before, p, lens, acc, end_id, tag):
    """the sampled pass against the rule on its own rows, and what it committed against spec_ref.accept fed with its draws"""
    B, n = feed.shape
    draws, rows = s.verify_draws(n), s.verify_logits(n)
    for b in range(B):
        want = R.sample_rows(rows[b], rc, b, int(p[b]), feed[b], before[b], int(lens[b]), S20, end_id)
        for i, d in enumerate(want):
            check_draw(d, int(draws[b, i]), f'{tag} row ({b}, {i})')
    ref = R.accept(p, np.zeros(B, np.int32), feed, draws, end_id, out_ids=before, input_lengths=lens, max_input_len=S20)
    np.testing.assert_array_equal(acc, ref['accepted'])
    out, st = s.output_ids(), s.step_state()
    np.testing.assert_array_equal(out, ref['out_ids'])
    np.testing.assert_array_equal(st['sequence_length'], ref['seq_len'])
    np.testing.assert_array_equal(st['next_position'], ref['rope_pos'])
    np.testing.assert_array_equal(st['input_lengths'], lens)
    logits = s.logits()
    for b in range(B):
        np.testing.assert_array_equal(logits[b], rows[b, acc[b]])        # row m of the sequence
        assert out[b, ref['seq_len'][b]] == ref['bonus'][b] == draws[b, acc[b]]  # the pending token (cur_ids) is the draw behind it
    return draws, ref


@pytest.mark.parametrize('n', [1, 4, 17])
@pytest.mark.parametrize('mode', ['fp16', 'sq_static'])
def test_sampled_verify_follows_the_rule_on_the_engines_own_rows(mode, n):
    scfg = dict(SAMPLING, random_seed=77)
    rc = SR.Config(**scfg)
    s, cfg, ids, lens = synthetic(mode, scfg)
    B = ids.shape[0]
    wave0, mfma0 = s.append_launches()
    before, p, pending = start(s, ids, lens)
    masked = s.step_state()['masked_tokens']
    r = np.random.default_rng(n)
    feed = np.concatenate([pending[:, None], r.integers(3, cfg['vocab_size'], (B, n - 1)).astype(np.int32)], 1)
    epoch = s.step_epoch()
    acc, lp = s.verify(feed, sampled=True)
    assert s.step_epoch() == epoch + 1
    draws, _ = check_pass(s, rc, feed, before, p, lens, acc, -1, f'{mode} n={n} random drafts')
    np.testing.assert_array_equal(s.step_state()['masked_tokens'], masked)
    wave, mfma = s.append_launches()
    if attention_append_kernel(n, cfg['hidden_size'] // cfg['num_heads']) == APPEND_ATTN_MFMA:
        assert n == 17 and mfma > mfma0 and wave == wave0  # 17 ids take the MFMA append kernel
    else:
        assert n < 17 and wave > wave0 and mfma == mfma0
    # log_probs stay the raw model's log p: the soft-max of the row before, whatever the sampling configuration
    rows = s.verify_logits(n).astype(np.float64)
    lse = np.log(np.exp(rows - rows.max(-1, keepdims=True)).sum(-1)) + rows.max(-1)
    assert (lp[:, 0] == 0).all()
    for i in range(1, n):
        np.testing.assert_allclose(lp[:, i], rows[np.arange(B), i - 1, feed[:, i]] - lse[:, i - 1], atol=1e-4)
    # a pass whose drafts are the draws of the pass before keeps one more of them each time (row i depends on t[0..i] alone), and a
    # pass whose drafts are ALL draws of the pass before keeps all of them
    for _ in range(n):
        nxt = np.concatenate([pending[:, None], draws[:, :n - 1]], 1)
        before, p, again = start(s, ids, lens)
        np.testing.assert_array_equal(again, pending)  # the same request: the same tokens
        acc, _ = s.verify(nxt, sampled=True)
        draws, ref = check_pass(s, rc, nxt, before, p, lens, acc, -1, f'{mode} n={n} drafts = draws')
        if np.array_equal(nxt[:, 1:], draws[:, :n - 1]):
            break
    np.testing.assert_array_equal(nxt[:, 1:], draws[:, :n - 1])
    assert acc.tolist() == [n - 1] * B
    # generation continues by step from the graph and still follows the rule
    g = int(ref['seq_len'][0]) - S20 + 1
    assert (ref['seq_len'] == S20 + g - 1).all()
    check_session_step(s, rc, lens, S20, g, -1, f'{mode} n={n} pending')
    for k in range(1, 4):
        s.step(1, use_graph=True)
        check_session_step(s, rc, lens, S20, g + k, -1, f'{mode} n={n} step {k} behind the pass')
    s.close()


def test_min_length_and_end_id_inside_a_pass():
    """end_id is the token the sampler draws first behind the pending token: with min_length beyond the pass no row may draw it, with
    min_length inside the pass the mask ends inside the rows; a drawn end_id ends the kept prefix and finishes the sequence."""
    n = 6
    base = dict(SAMPLING, random_seed=5)
    s, cfg, ids, lens = synthetic('fp16', base)
    B = ids.shape[0]
    before, p, pending = start(s, ids, lens)
    feed = np.repeat(pending[:, None], n, 1)
    s.verify(feed, sampled=True)
    end_id = int(s.verify_draws(n)[0, 0])
    for min_length in (1, WARM + 4, 40):  # row i draws token number WARM + 2 + i
        scfg = dict(base, min_length=min_length)
        s.set_sampling(scfg)
        s.generate(ids, lens, 1, end_id=end_id)  # the step API takes end_id from the last generate()
        before, p, pending = start(s, ids, lens)
        fin = np.array([int(end_id in before[b, S20:p[b] + 1]) for b in range(B)])
        feed = np.repeat(pending[:, None], n, 1)
        acc, _ = s.verify(feed, sampled=True)
        draws, rows = s.verify_draws(n), s.verify_logits(n)
        rc = SR.Config(**scfg)
        for b in range(B):
            want = R.sample_rows(rows[b], rc, b, int(p[b]), feed[b], before[b], int(lens[b]), S20, end_id, finished=fin[b])
            if fin[b]:
                assert acc[b] == -1 and (draws[b] == end_id).all()
                continue
            for i, d in enumerate(want):
                check_draw(d, int(draws[b, i]), f'min_length {min_length} row ({b}, {i})')
                if WARM + 2 + i < min_length:
                    assert draws[b, i] != end_id
        ref = R.accept(p, fin, feed, draws, end_id, out_ids=before)
        np.testing.assert_array_equal(acc, ref['accepted'])
        np.testing.assert_array_equal(s.output_ids(), ref['out_ids'])
        if min_length == 1 and not fin[0]:
            assert draws[0, 0] == end_id and acc[0] == 0 and s.output_ids()[0, p[0] + 1] == end_id
    s.close()


def test_a_greedy_configuration_takes_the_greedy_path_bit_for_bit():
    """no configuration, and one that is plain arg-max: sampled=True is sampled=False - no sampler launch, verify_draws are the
    arg-maxes; sequence 0 offers two right drafts, so the kept prefix is not empty"""
    n = 5
    outs, feed = [], None
    for sampled, scfg in ((False, None), (True, None), (True, dict(top_k=1, top_p=0.3, random_seed=9))):
        s, cfg, ids, lens = synthetic('fp16', scfg)
        before, p, pending = start(s, ids, lens)
        if feed is None:
            r = np.random.default_rng(1)
            feed = np.concatenate([pending[:, None], r.integers(3, cfg['vocab_size'], (ids.shape[0], n - 1)).astype(np.int32)], 1)
            for _ in range(2):  # the arg-maxes behind the pending token of sequence 0, one more per pass
                s.verify(feed)
                top = s.verify_top1(n)
                feed[0, 1:3] = top[0, :2]
                before, p, pending = start(s, ids, lens)
        acc, lp = s.verify(feed, sampled=sampled)
        np.testing.assert_array_equal(s.verify_draws(n), s.verify_top1(n))
        outs.append((acc, lp, s.output_ids(), s.logits(), s.verify_top1(n), s.step_state()['sequence_length']))
        s.close()
    assert outs[0][0][0] >= 2
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            np.testing.assert_array_equal(a, b)


def test_refusals_of_the_sampled_entry():
    t, w = load_tiny()
    ids, lens = t['ids'], t['input_lengths']
    B, S = ids.shape
    new = 6
    tok = np.full((B, 2), 5, np.int32)
    s = tiny_session(w)
    with pytest.raises(RuntimeError, match='setup'):
        s.verify(tok, sampled=True)
    s.setup(B, S, new)
    s.set_sampling(top_k=40)
    with pytest.raises(RuntimeError, match='context'):
        s.verify(tok, sampled=True)
    s.context(ids, lens)
    for getter in (s.verify_draws, s.verify_logits):
        with pytest.raises(RuntimeError, match='no verify pass'):  # refused before any verify pass, as verify_top1 is
            getter(2)
    before = s.output_ids(), s.step_state(), s.logits()
    with pytest.raises(RuntimeError, match='TLLM_VERIFY_MAX_TOKENS'):
        s.verify(np.full((B, 33), 5, np.int32), sampled=True)
    with pytest.raises(RuntimeError, match='capacity'):  # p + n + 1 > max_seq_len: no slot for the new pending token
        s.verify(np.full((B, new), 5, np.int32), sampled=True)
    with pytest.raises(RuntimeError, match='speculative sampling is not built'):  # the greedy entry still refuses
        s.verify(tok)
    after = s.output_ids(), s.step_state(), s.logits()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[2], after[2])
    for k in before[1]:
        assert np.array_equal(before[1][k], after[1][k]), k
    acc, _ = s.verify(np.full((B, new - 1), 5, np.int32), sampled=True)  # exactly up to the capacity is served
    assert (acc >= 0).all() and (s.step_state()['sequence_length'] <= S + new - 1).all()
    assert s.verify_draws(new - 1).shape == (B, new - 1) and s.verify_logits(new - 1).shape == (B, new - 1, 128)
    with pytest.raises(RuntimeError, match='no verify pass'):  # n is the last pass's
        s.verify_draws(2)
    s.close()
    for keys, beam in ((dict(paged_kv_cache=1, tokens_per_block=16), 1), ({}, 2)):
        s = tiny_session(w, **keys)
        s.setup(B, S, new, beam)
        s.context(ids, lens)
        with pytest.raises(RuntimeError, match='not built'):
            s.verify(np.full((B, 2), 5, np.int32), sampled=True)
        with pytest.raises(RuntimeError, match='not built'):
            s.generate_lookup(ids, lens, 2, num_draft_tokens=2, sampled=True)
        s.close()


# ------------------------------------------------------------------------------------------------ generate_lookup, sampled
SEED = 125             # chosen by tools/spec_sampling_seed_scan.py (module docstring)
SEED_MARGIN = 9.012e-4 # its smallest margin, share of S (CPU oracle)
PATH_DIFFERENCE = 2.567e-5  # verify rows against step logits, share of S (measured once on an MI355X: profiles/spec_sampling.txt)
OTHER_SEED = 151       # a second seed of the scan whose tokens differ from SEED's on the oracle
LOOKUP_CFG = dict(top_k=40, temperature=0.8, repetition_penalty=1.1)
SETUP_NEW = LOOKUP_NEW + LOOKUP_N


# the front-end test: the tiny HF fixture, top_k 2 (one boundary per draw) - its distributions are flat, so the path difference is
# large and only a configuration with few boundaries leaves seeds with room (the scan with --tiny --new 16 --top_k 2)
TINY_SEED = 112
TINY_SEED_MARGIN = 7.475e-2
TINY_PATH_DIFFERENCE = 4.654e-4  # measured with the above


def test_the_seeds_margin_is_four_times_the_measured_path_difference():
    assert SEED_MARGIN >= 4 * PATH_DIFFERENCE
    assert TINY_SEED_MARGIN >= 4 * TINY_PATH_DIFFERENCE


@functools.lru_cache(maxsize=None)
def batch(rows):
    e = TP.load_eval('deterministic')
    lens = e['lengths'][list(rows)].astype(np.int32)
    ids = np.zeros((len(rows), int(lens.max())), np.int32)
    for i, b in enumerate(rows):
        ids[i, :lens[i]] = e['prompts'][b, :lens[i]]
    return ids, lens


@functools.lru_cache(maxsize=None)
def parent():
    return TP.quantised('deterministic', 'fp16')


def run(rows, seed, lookup, n=LOOKUP_N):
    ids, lens = batch(rows)
    s = quant_session(*parent())
    s.setup(len(rows), ids.shape[1], SETUP_NEW)
    s.set_sampling(dict(LOOKUP_CFG, random_seed=seed))
    try:
        if lookup:
            return s.generate_lookup(ids, lens, LOOKUP_NEW, num_draft_tokens=n, max_ngram=LOOKUP_G, sampled=True)
        return s.generate(ids, lens, LOOKUP_NEW), None
    finally:
        s.close()


@pytest.mark.parametrize('rows', LOOKUP_BATCHES, ids=['prompts-0-1', 'prompts-1-6'])
def test_sampled_lookup_generates_the_tokens_of_generate_in_the_predicted_rounds(rows):
    ids, lens = batch(rows)
    S = ids.shape[1]
    want, _ = run(rows, SEED, False)
    out, st = run(rows, SEED, True)
    np.testing.assert_array_equal(out, want)
    cont = want[:, S:S + LOOKUP_NEW]
    sim = R.simulate_lookup_rounds([ids[i, :lens[i]] for i in range(len(rows))], list(cont), LOOKUP_N, LOOKUP_G, LOOKUP_NEW)
    print(f'[sampled lookup {rows}] {st}')
    for k in ('rounds', 'verify_rounds', 'step_rounds', 'drafted', 'accepted'):
        assert st[k] == sim[k], (k, st, {q: sim[q] for q in st})
    assert st['verify_rounds'] > 0
    again, st2 = run(rows, SEED, True)  # the same request twice
    np.testing.assert_array_equal(again, out)
    assert st2 == st
    if rows == LOOKUP_BATCHES[0]:
        other, _ = run(rows, OTHER_SEED, True)  # another seed differs, and is generate()'s for that seed too
        assert not np.array_equal(other, out)
        for n in (2, 8):  # n does not change the tokens
            np.testing.assert_array_equal(run(rows, SEED, True, n=n)[0], out)


def test_decode_lookup_with_speculative_sampling_returns_what_decode_returns():
    from tensorrt_llm import Mapping
    from tensorrt_llm.quantization import QuantMode
    from tensorrt_llm.runtime import GenerationSession, ModelConfig, SamplingConfig
    from test_frontend import build_tiny_engine
    engine, _, t = build_tiny_engine(QuantMode(0))
    ids, lens = t['ids'], t['input_lengths']
    B, S = ids.shape
    dec = GenerationSession(ModelConfig(vocab_size=128, num_layers=2, num_heads=2, hidden_size=64), engine, Mapping(1, 0))
    dec.setup(B, S, 24)
    scfg = SamplingConfig(end_id=-1, pad_id=0, top_k=2, temperature=0.8, repetition_penalty=1.1)
    scfg.random_seed = TINY_SEED
    want = dec.decode(ids, lens, scfg, max_new_tokens=16)
    got = dec.decode_lookup(ids, lens, scfg, num_draft_tokens=8, max_ngram=3, speculative_sampling=True)
    assert got.shape == want.shape == (B, 1, S + 24)
    np.testing.assert_array_equal(got, want)
    greedy = dec.decode(ids, lens, SamplingConfig(end_id=-1, pad_id=0), max_new_tokens=16)
    assert not np.array_equal(got, greedy)
    st = dec.lookup_stats
    assert st['rounds'] == st['verify_rounds'] + st['step_rounds'] and 1 <= st['rounds'] <= 16
    with pytest.raises(NotImplementedError, match='speculative sampling is not built'):
        dec.decode_lookup(ids, lens, scfg)
    # verify() with a sampling configuration takes the sampled entry: the pending token alone is one sampled step
    dec.decode(ids, lens, scfg, max_new_tokens=4)
    v = dec.verify(want[:, 0, S + 3:S + 4], scfg)
    assert v['accepted'].tolist() == [0] * B and v['logits'].shape == (B, 128)
    np.testing.assert_array_equal(dec.runtime.output_ids()[:, S + 4], want[:, 0, S + 4])
