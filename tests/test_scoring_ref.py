"""The token-scoring rule restated in numpy float64 (tensorrt_llm/runtime/scoring_ref.py) - the reference the GPU tests hold the
device to - checked on the CPU against torch.log_softmax in float64, on its special values, on the part / merge layout and on
the index convention of sequence scores; and the argument checks of GenerationSession.score that need no device."""
import numpy as np
import pytest
import torch

from tensorrt_llm.runtime import scoring_ref as R
from tensorrt_llm.runtime.generation import GenerationSession

NINF = -np.inf


def test_token_logprobs_match_torch_log_softmax_float64():
    rng = np.random.default_rng(0)
    for rows, V, std in ((7, 257, 1.0), (3, 32003, 8.0), (5, 1, 2.0), (4, 1000, 16.0)):
        x = rng.normal(0, std, (rows, V))
        t = rng.integers(0, V, rows)
        lp, lse, top = R.token_logprobs(x, t)
        ref = torch.log_softmax(torch.from_numpy(x), dim=-1).numpy()
        assert np.abs(lp - ref[np.arange(rows), t]).max() < 1e-12
        assert np.abs(lse - torch.logsumexp(torch.from_numpy(x), dim=-1).numpy()).max() < 1e-12
        assert (top == x.argmax(axis=1)).all() and top.dtype == np.int32


def test_padding_columns_are_not_read():
    rng = np.random.default_rng(1)
    x = rng.normal(0, 2, (4, 40))
    t = np.array([0, 36, 5, 17])
    padded = np.concatenate([x[:, :37], np.full((4, 3), 1e30)], axis=1)
    a = R.token_logprobs(x[:, :37], t)
    b = R.token_logprobs(padded, t, vocab=37)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


def test_special_values():
    x = np.array([[0.0, 1.0, NINF, 2.0],
                  [NINF, NINF, NINF, NINF],
                  [3.0, 3.0, 1.0, 3.0],
                  [NINF, 5.0, NINF, NINF]])
    # no target (-1), out of range (4 = vocab), a -inf entry, the row of only -inf
    lp, lse, top = R.token_logprobs(x, [-1, 0, 4, 0])
    assert lp[0] == 0.0 and lp[2] == 0.0                  # no target / outside [0, vocab): 0
    assert lp[1] == NINF and lse[1] == NINF and top[1] == 0  # only -inf: lse -inf, log_prob -inf, top1 0
    assert lp[3] == NINF and lse[3] == 5.0 and top[3] == 1   # -inf target in a live row
    assert top[2] == 0                                       # ties -> lowest id
    lp2, _, _ = R.token_logprobs(x, [2, 1, 3, 1])
    assert lp2[0] == NINF and lp2[1] == NINF and lp2[3] == 0.0
    assert abs(lp2[2] - (3.0 - np.log(3 * np.exp(3.0) + np.exp(1.0)))) < 1e-12
    assert not np.isnan(lp).any() and not np.isnan(lp2).any()


@pytest.mark.parametrize('nparts', [1, 3, 4])
def test_merge_of_parts_equals_the_unsharded_result(nparts):
    rng = np.random.default_rng(2 + nparts)
    rows, V = 9, 1001
    x = rng.normal(0, 4, (rows, V))
    x[1] = np.round(x[1])            # exact ties
    x[2, rng.random(V) < 0.9] = NINF  # mostly -inf: whole parts may be dead
    x[3] = NINF
    t = rng.integers(0, V, rows)
    t[4], t[5], t[6] = -1, 0, V - 1
    vp = (V + nparts - 1) // nparts
    parts = np.full((nparts, rows, vp), 1e30)  # padding ids hold a value that would dominate if read
    for p in range(nparts):
        n = max(min(V - p * vp, vp), 0)
        parts[p, :, :n] = x[:, p * vp:p * vp + n]
    rec = R.partials(parts, t, V)
    assert rec.shape == (nparts, rows, 5)
    lp, lse, top = R.merge(rec, t, V)
    lp0, lse0, top0 = R.token_logprobs(x, t)
    fin = np.isfinite(lp0)
    assert np.array_equal(fin, np.isfinite(lp)) and np.array_equal(lp[~fin], lp0[~fin])
    assert np.abs(lp[fin] - lp0[fin]).max() < 1e-12
    fin = np.isfinite(lse0)
    assert np.array_equal(lse[~fin], lse0[~fin]) and np.abs(lse[fin] - lse0[fin]).max() < 1e-12
    assert np.array_equal(top, top0)
    if nparts == 1:  # one part: the merge is the identity on the record
        assert np.array_equal(lse[fin], rec[0, fin, 0] + np.log(rec[0, fin, 1]))
        assert np.array_equal(top, rec[0, :, 4].astype(np.int32))


def test_a_part_without_valid_ids():
    x = np.full((2, 2, 4), 1e30)
    x[0] = [[1.0, 2.0, 3.0, 0.5], [0.0, 0.0, 0.0, 0.0]]
    rec = R.partials(x, [2, -1], 4)  # vocab 4: part 1 is padding only
    assert (rec[1, :, 0] == NINF).all() and (rec[1, :, 1] == 0).all() and (rec[1, :, 4] == R.NO_ID).all()
    lp, lse, top = R.merge(rec, [2, -1], 4)
    assert abs(lp[0] - (3.0 - np.log(np.exp([1.0, 2.0, 3.0, 0.5]).sum()))) < 1e-12 and lp[1] == 0.0
    assert list(top) == [2, 0]


def test_sequence_scores_index_convention():
    # 2 x 4, V = 3: position_logits[b][t] is the distribution of token t + 1
    z = np.log(np.array([[[.5, .25, .25], [.1, .2, .7], [.3, .3, .4], [.9, .05, .05]],
                         [[.2, .2, .6], [.6, .3, .1], [.1, .8, .1], [1 / 3, 1 / 3, 1 / 3]]]))
    ids = np.array([[2, 1, 2, 0], [0, 2, 9, 9]])
    lens = [4, 2]
    lp, top = R.sequence_scores(z, ids, lens)
    want = np.array([[0, np.log(.25), np.log(.7), np.log(.3)], [0, np.log(.6), 0, 0]])
    assert np.abs(lp - want).max() < 1e-12
    assert top.tolist() == [[-1, 0, 2, 2], [-1, 2, -1, -1]] and top.dtype == np.int32
    assert abs(R.perplexity(lp, lens) - np.exp(-(np.log(.25) + np.log(.7) + np.log(.3) + np.log(.6)) / 4)) < 1e-12
    assert abs(R.perplexity(lp[1], lens[1:]) - 1 / .6) < 1e-12
    assert np.isnan(R.perplexity(np.zeros(4), [1]))


def test_generation_session_score_argument_errors():
    gs = GenerationSession.__new__(GenerationSession)
    gs.batch_size, gs.max_input_length, gs.max_new_tokens, gs.beam_width = 2, 4, 2, 1
    gs.runtime = None  # nothing may reach the device
    ids, lens = np.zeros((2, 4), np.int32), np.array([4, 2], np.int32)
    with pytest.raises(ValueError, match='matching sizes'):
        gs.score(ids[:, :3], lens)
    with pytest.raises(ValueError, match='matching sizes'):
        gs.score(ids[0], lens)
    with pytest.raises(ValueError, match='one length per sequence'):
        gs.score(ids, lens[:1])
    with pytest.raises(ValueError, match=r'\[1, 4\]'):
        gs.score(ids, np.array([0, 2], np.int32))
    with pytest.raises(ValueError, match=r'\[1, 4\]'):
        gs.score(torch.from_numpy(ids), torch.tensor([4, 5], dtype=torch.int32))
    with pytest.raises(TypeError):
        gs.score(ids.astype(np.float32), lens)
    gs.beam_width = 2
    with pytest.raises(ValueError, match='beam_width 1'):
        gs.score(ids, lens)
