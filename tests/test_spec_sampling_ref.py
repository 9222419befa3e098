"""Speculative sampling by exact match on the CPU: spec_ref.sample_rows against a step-by-step restatement
on top of sampling_ref.draw, spec_ref.accept fed with draws in the arg-maxes' place, and the front-end's argument handling with a
fake runtime.  No GPU needed."""
import numpy as np
import pytest

from tensorrt_llm.runtime import GenerationSession, SamplingConfig
from tensorrt_llm.runtime import sampling_ref as SR
from tensorrt_llm.runtime import spec_ref as R

V, S, SMAX, END = 97, 10, 64, 2


def rows_and_record(seed, n, in_len, p):
    """n logits rows whose soft-max leaves a handful of likely ids (END among them), the ids of a pass and a token record whose
    generated part and drafts repeat likely ids, so that the penalties change the draw"""
    r = np.random.default_rng(seed)
    x = (r.standard_normal((n, V)) * 2.0).astype(np.float32)
    x[:, END] += 3.0
    likely = np.argsort(-x, axis=1)
    rec = r.integers(0, V, SMAX).astype(np.int32)
    rec[in_len:S] = 90  # padding slots hold an id the rule must NOT penalise
    rec[S:p] = likely[0, :p - S]
    rec[p:] = 91  # slots the pass has not committed: never read (t[0..i] come from the ids)
    t = np.array([likely[min(i + 1, n - 1), i % 3] for i in range(n)], np.int32)
    return x, t, rec


def stepwise(x, cfg, b, p, t, rec, in_len, end_id):
    """the definition: write t[0..i] into a copy of the record, then the step's draw for the token of slot p + i + 1"""
    out = []
    for i in range(x.shape[0]):
        g = p + i + 2 - S
        h = np.array(rec)
        h[p:p + i + 1] = t[:i + 1]
        out.append(SR.draw(x[i], cfg, b, g, end_id, SR.history_ids(h, in_len, S, g)))
    return out


def same(a, b):
    assert a.token == b.token and np.float32(a.u).tobytes() == np.float32(b.u).tobytes()
    np.testing.assert_array_equal(a.cand, b.cand)
    np.testing.assert_array_equal(a.prefix, b.prefix)
    assert a.target == b.target


CONFIGS = [dict(top_k=40, top_p=0.9, temperature=0.8, repetition_penalty=1.1), dict(top_k=0, top_p=0.7),
           dict(top_k=1, presence_penalty=4.0), dict(top_k=8, min_length=6), dict(top_k=5, repetition_penalty=3.0, min_length=5)]


@pytest.mark.parametrize('cfg', CONFIGS, ids=[str(i) for i in range(len(CONFIGS))])
def test_sample_rows_is_the_step_draw_with_the_drafts_in_the_history(cfg):
    for b, (n, in_len, p) in enumerate(((1, 10, 10), (5, 6, 12), (32, 8, 17))):  # in_len < S: padding slots inside the prompt
        c = SR.Config(**dict(cfg, random_seed=11 + b))
        x, t, rec = rows_and_record(100 * b + n, n, in_len, p)
        got = R.sample_rows(x, c, b, p, t, rec, in_len, S, END)
        want = stepwise(x, c, b, p, t, rec, in_len, END)
        assert len(got) == n
        for a, w in zip(got, want):
            same(a, w)
        # the record behind p is not read: the drafts come from the ids alone
        rec2 = np.array(rec)
        rec2[p:] = 5
        for a, w in zip(R.sample_rows(x, c, b, p, t, rec2, in_len, S, END), got):
            same(a, w)


def test_padding_slots_are_skipped_and_the_ids_of_the_pass_count():
    c = SR.Config(top_k=1, presence_penalty=100.0)  # the arg-max of the penalised row: the history decides it
    n, in_len, p = 3, 6, 11
    x = np.zeros((n, V), np.float32)
    x[:, 90], x[:, 40], x[:, 41], x[:, 42] = 4.0, 3.0, 2.0, 1.0
    rec = np.full(SMAX, 7, np.int32)
    rec[in_len:S] = 90     # only in padding slots: 90 stays the arg-max
    t = np.array([7, 90, 40], np.int32)
    d = R.sample_rows(x, c, 0, p, t, rec, in_len, S, END)
    assert [q.token for q in d] == [90, 40, 41]  # row 1 has t[1] = 90 in its history, row 2 also t[2] = 40
    t0 = np.array([90, 7, 7], np.int32)           # t[0] stands in the pending token's place: it counts from row 0 on
    assert [q.token for q in R.sample_rows(x, c, 0, p, t0, rec, in_len, S, END)] == [40, 40, 40]


def test_min_length_masks_end_id_per_row_by_its_own_token_number():
    n, in_len, p = 6, 10, 11
    x = np.zeros((n, V), np.float32)
    x[:, END], x[:, 50] = 9.0, 8.0
    c = SR.Config(top_k=1, min_length=6)
    rec = np.full(SMAX, 7, np.int32)
    d = R.sample_rows(x, c, 1, p, np.full(n, 7, np.int32), rec, in_len, S, END)
    g = [p + i + 2 - S for i in range(n)]
    assert g == [3, 4, 5, 6, 7, 8]
    assert [q.token for q in d] == [50, 50, 50, END, END, END]  # masked while g < 6: the mask ends inside the rows


def test_a_frozen_sequence_is_not_drawn():
    x, t, rec = rows_and_record(3, 4, 10, 12)
    c = SR.Config(top_k=40, random_seed=1)
    assert R.sample_rows(x, c, 0, 12, t, rec, 10, S, END, finished=1) == [None] * 4
    assert R.sample_rows(x, c, 0, 12, t, rec, 10, S, END, limit=12) == [None] * 4
    assert all(d is not None for d in R.sample_rows(x, c, 0, 12, t, rec, 10, S, END, limit=13))


def test_accept_fed_with_draws_keeps_the_longest_prefix_that_equals_them():
    draws = np.array([[5, 6, 7, 8, 9], [5, 6, END, 8, 9], [5, 6, 7, 8, 9], [1, 1, 1, 1, 1]], np.int32)
    ids = np.array([[3, 5, 6, 0, 8],      # drafts 1, 2 equal the draws of rows 0, 1; draft 3 does not
                    [3, 5, 6, END, 8],    # the draw of row 2 is end_id: kept as the pending token, nothing behind it
                    [3, 5, 6, 7, 8],      # every draft equals its draw
                    [3, 1, 1, 1, 1]], np.int32)  # frozen
    out = np.zeros((4, 32), np.int32)
    r = R.accept([10, 10, 10, 10], [0, 0, 0, 1], ids, draws, end_id=END, out_ids=out, cur_ids=np.zeros(4, np.int32))
    assert r['accepted'].tolist() == [2, 2, 4, -1]
    assert r['bonus'].tolist() == [7, END, 9, -1]
    assert r['seq_len'].tolist() == [13, 13, 15, 10]
    assert r['finished'].tolist() == [0, 1, 0, 1]
    np.testing.assert_array_equal(r['out_ids'][0, 10:14], [3, 5, 6, 7])
    np.testing.assert_array_equal(r['out_ids'][1, 10:14], [3, 5, 6, END])
    np.testing.assert_array_equal(r['out_ids'][2, 10:16], [3, 5, 6, 7, 8, 9])
    assert not r['out_ids'][3].any()
    # whatever the drafts, the committed tokens are draws: the sequence is the one the sampler alone would have produced
    for b in range(3):
        m = r['accepted'][b]
        np.testing.assert_array_equal(r['out_ids'][b, 11:11 + m + 1], draws[b, :m + 1])


# ------------------------------------------------------------------------------------------------ front-end
class FakeRuntime:
    def __init__(self, batch, smax):
        self.calls, self.batch, self.smax = [], batch, smax

    def set_sampling(self, cfg):
        self.calls.append(('set_sampling', dict(cfg)))

    def generate_lookup(self, ids, lens, new, **kw):
        self.calls.append(('generate_lookup', new, kw))
        return np.zeros((self.batch, self.smax), np.int32), dict(rounds=1, verify_rounds=1, step_rounds=0, drafted=0, accepted=0)


def session():
    gs = GenerationSession.__new__(GenerationSession)
    gs.batch_size, gs.max_input_length, gs.max_new_tokens, gs.beam_width = 2, 8, 24, 1
    gs.runtime = FakeRuntime(2, 32)
    return gs


def test_decode_lookup_passes_a_sampled_configuration_through_only_when_asked():
    ids, lens = np.zeros((2, 8), np.int32), np.array([8, 3], np.int32)
    scfg = SamplingConfig(end_id=2, pad_id=0, top_k=40, temperature=0.7)
    scfg.random_seed = 9
    gs = session()
    with pytest.raises(NotImplementedError, match='speculative sampling is not built'):  # the default still raises
        gs.decode_lookup(ids, lens, scfg)
    assert gs.runtime.calls == []
    out = gs.decode_lookup(ids, lens, scfg, num_draft_tokens=4, max_ngram=2, speculative_sampling=True)
    assert out.shape == (2, 1, 32)
    (a, cfg), (b, new, kw) = gs.runtime.calls
    assert a == 'set_sampling' and cfg['top_k'] == 40 and cfg['temperature'] == 0.7 and cfg['random_seed'] == 9
    assert b == 'generate_lookup' and new == 20
    assert kw == dict(end_id=2, pad_id=0, num_draft_tokens=4, max_ngram=2, sampled=True)
    # a greedy configuration without the keyword: the call the greedy entry has always received
    gs = session()
    gs.decode_lookup(ids, lens, SamplingConfig(end_id=2, pad_id=0))
    assert gs.runtime.calls[1][2] == dict(end_id=2, pad_id=0, num_draft_tokens=8, max_ngram=3)
    # the keyword lifts the greedy requirement and nothing else
    gs = session()
    with pytest.raises(ValueError, match='num_beams 1'):
        gs.decode_lookup(ids, lens, SamplingConfig(end_id=2, pad_id=0, num_beams=2), speculative_sampling=True)
    with pytest.raises(ValueError, match='num_draft_tokens'):
        gs.decode_lookup(ids, lens, scfg, num_draft_tokens=33, speculative_sampling=True)
    with pytest.raises(ValueError, match='mutually exclusive'):
        gs.decode_lookup(ids, lens, SamplingConfig(end_id=2, pad_id=0, repetition_penalty=1.2, presence_penalty=0.5),
                         speculative_sampling=True)
    assert gs.runtime.calls == []


def test_run_py_takes_the_prompt_lookup_sampling_flag():
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'trtllm-llama_amd', 'examples', 'llama_quant'))
    import run
    a = run.parse_arguments(['--max_output_len', '8'])
    assert a.prompt_lookup_sampling is False
    a = run.parse_arguments(['--max_output_len', '8', '--prompt_lookup_tokens', '8', '--prompt_lookup_sampling', '--top_k', '40'])
    assert a.prompt_lookup_sampling is True and a.top_k == 40


def test_library_exports_the_speculative_sampling_symbols():
    import os
    import re
    from tensorrt_llm.plugin import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'tllm_runtime_api.h')).read(), flags=re.S)
    lib = capi.load_library()
    for name in ('tllm_session_verify_sampled', 'tllm_session_generate_lookup_sampled', 'tllm_spec_sample_rows',
                 'tllm_session_verify_draws', 'tllm_session_verify_logits'):
        assert re.search(r'\b' + name + r'\s*\(', text), f'{name} is not declared'
        assert hasattr(lib, name), f'{name} is declared but not exported'
