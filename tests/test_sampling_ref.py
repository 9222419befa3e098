"""The sampling rule without a GPU: the counter-based generator against its published known-answer vectors, the numpy
restatement (tensorrt_llm/runtime/sampling_ref.py) on hand-made rows, and what the front-end accepts and refuses."""
import numpy as np
import pytest

from tensorrt_llm.runtime import sampling_ref as R
from tensorrt_llm.runtime.generation import GenerationSession, SamplingConfig

# Random123 (D. E. Shaw Research) kat_vectors, philox4x32 with 10 rounds: counter words, key words -> output words
PHILOX_KAT = [
    ((0x00000000, ) * 4, (0x00000000, ) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, ) * 4, (0xffffffff, ) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize('ctr,key,want', PHILOX_KAT)
def test_philox4x32_10_known_answers(ctr, key, want):
    assert R.philox4x32_10(ctr, key) == want


def test_uniform_is_a_function_of_seed_row_and_token_number_in_0_1():
    seen = set()
    for seed in (0, 1, 2**40 + 7, 2**64 - 1):
        for b in (0, 1, 5):
            for g in (1, 2, 300):
                u = R.uniform(seed, b, g)
                assert u.dtype == np.float32 and 0.0 < u <= 1.0
                assert u == R.uniform(seed, b, g)
                w0 = R.philox4x32_10((b, g, 0, 0), (seed & 0xffffffff, seed >> 32))[0]
                assert float(u) == ((w0 >> 8) + 1) / 2.0**24
                seen.add(float(u))
    assert len(seen) == 36  # no two of them collide
    us = np.array([R.uniform(3, 0, g) for g in range(1, 4001)], np.float64)
    assert abs(us.mean() - 0.5) < 5 * (1 / 12 / 4000)**0.5


def test_ties_go_to_the_lowest_id_and_top_k_1_is_argmax():
    x = np.array([0.5, 2.0, -1.0, 2.0, 2.0, 0.0], np.float32)
    assert list(R.order(x)) == [1, 3, 4, 0, 5, 2]
    for u in (1e-7, 0.5, 1.0):
        assert R.sample(x, R.Config(top_k=1), 0, 1, u=u) == 1
    # -0 and +0 are one value: the lower id wins
    assert R.sample(np.array([-0.0, 0.0, -3.0], np.float32), R.Config(top_k=1), 0, 1) == 0
    # three equal candidates share the mass in id order
    cfg = R.Config(top_k=3)
    assert [R.sample(x, cfg, 0, 1, u=u) for u in (0.2, 1 / 3, 0.34, 0.66, 0.67, 1.0)] == [1, 1, 3, 3, 4, 4]


def test_u_1_selects_the_last_candidate_reached_and_never_one_past_k():
    x = np.log(np.array([0.4, 0.3, 0.2, 0.1], np.float32))
    assert R.sample(x, R.Config(top_k=2), 0, 1, u=1.0) == 1         # k' = 2: the mass of ids 0, 1 only
    assert R.sample(x, R.Config(top_k=3), 0, 1, u=1.0) == 2
    assert R.sample(x, R.Config(top_k=0, top_p=1.0), 0, 1, u=1.0) == 3
    assert R.sample(x, R.Config(top_k=0, top_p=0.65), 0, 1, u=1.0) == 1  # 0.4 + 0.3 >= 0.65
    assert R.sample(x, R.Config(top_k=0, top_p=0.75), 0, 1, u=1.0) == 2
    assert R.sample(x, R.Config(top_k=2000), 0, 1, u=1.0) == 3      # clipped to the vocabulary
    # -inf candidates carry no mass: u = 1 stops at the last id that moved the prefix sum
    y = np.array([1.0, -np.inf, 0.0, -np.inf], np.float32)
    d = R.draw(y, R.Config(top_k=4), 0, 1, u=1.0)
    assert d.token == 2 and list(d.cand) == [0, 2, 1, 3]
    # a row of -inf yields the first id of the order
    assert R.sample(np.full(5, -np.inf, np.float32), R.Config(top_k=3), 0, 1, u=0.9) == 0


def test_top_p_0_substitutions_and_clipping():
    assert R.Config(top_k=0, top_p=0.0).effective(100) == (1, 0.0)       # arg-max
    assert R.Config(top_k=5, top_p=0.0).effective(100) == (5, 1.0)       # top-k only
    assert R.Config(top_k=0, top_p=0.5).effective(100) == (100, 0.5)     # top-p only
    assert R.Config(top_k=5000, top_p=3.0).effective(32000) == (1024, 1.0)
    assert R.Config(top_k=50, top_p=0.9).effective(20)[0] == 20
    x = np.array([0.0, 1.0, 3.0, 2.0], np.float32)
    for u in (0.01, 0.5, 1.0):
        assert R.sample(x, R.Config(top_k=0, top_p=0.0), 0, 1, u=u) == 2


def test_a_repeated_id_is_penalised_once_and_padding_slots_are_not():
    x = np.array([2.0, -2.0, 1.0, 4.0, 3.0], np.float32)
    max_in, in_len = 4, 2
    row = np.array([3, 1, 0, 0, 3, 1, 3], np.int32)  # prompt [3, 1], padding [0, 0] (id 0!), generated [3, 1, 3]
    hist = R.history_ids(row, in_len, max_in, g=4)
    assert sorted(hist.tolist()) == [1, 1, 3, 3, 3]
    y = R.transform(x, R.Config(repetition_penalty=2.0), 4, history=hist)
    np.testing.assert_array_equal(y, np.array([2.0, -4.0, 1.0, 2.0, 3.0], np.float32))  # id 0 untouched, id 3 halved ONCE
    y = R.transform(x, R.Config(presence_penalty=0.5), 4, history=hist)
    np.testing.assert_array_equal(y, np.array([2.0, -2.5, 1.0, 3.5, 3.0], np.float32))
    # g = 1: only the real prompt counts
    assert sorted(R.history_ids(row, in_len, max_in, g=1).tolist()) == [1, 3]
    # temperature comes first, in fp32
    y = R.transform(x, R.Config(temperature=0.5, presence_penalty=1.0), 1, history=np.array([0]))
    inv = np.float32(1.0) / (np.float32(0.5) + np.float32(1e-6))
    np.testing.assert_array_equal(y, np.array([x[0] * inv - np.float32(1.0)] + [v * inv for v in x[1:]], np.float32))
    with pytest.raises(ValueError):
        R.transform(x, R.Config(repetition_penalty=1.2, presence_penalty=0.1), 1, history=hist)


def test_min_length_masks_end_id_for_exactly_the_first_min_length_minus_1_tokens():
    x = np.array([0.0, 9.0, 1.0], np.float32)  # end_id 1 is the arg-max
    cfg = R.Config(top_k=1, min_length=4)
    assert [R.sample(x, cfg, 0, g, end_id=1) for g in (1, 2, 3, 4, 5)] == [2, 2, 2, 1, 1]
    assert R.transform(x, cfg, 3, end_id=1)[1] == -np.finfo(np.float32).max
    assert [R.sample(x, R.Config(top_k=1), 0, g, end_id=1) for g in (1, 2)] == [1, 1]  # default min_length 1 masks nothing


def test_probabilities_are_the_cut_softmax():
    x = np.log(np.array([0.1, 0.4, 0.2, 0.3], np.float32))
    np.testing.assert_allclose(R.probabilities(x, R.Config(top_k=0, top_p=1.0)), [0.1, 0.4, 0.2, 0.3], atol=1e-6)
    np.testing.assert_allclose(R.probabilities(x, R.Config(top_k=2)), [0, 4 / 7, 0, 3 / 7], atol=1e-6)
    np.testing.assert_allclose(R.probabilities(x, R.Config(top_k=0, top_p=0.5)), [0, 0.8, 0, 0.2], atol=1e-6)
    # the empirical frequencies of the restatement's own draws follow them
    cfg = R.Config(top_k=3, top_p=0.8, random_seed=11)
    p = R.probabilities(x, cfg)
    n = 4000
    cnt = np.bincount([R.sample(x, cfg, 0, g) for g in range(1, n + 1)], minlength=4)
    assert np.all(np.abs(cnt / n - p) <= 5 * np.sqrt(p * (1 - p) / n) + 1e-12)


def test_front_end_accepts_what_the_sampler_honours():
    scfg = SamplingConfig(end_id=2, pad_id=2, top_k=40, top_p=0.9, temperature=0.8, repetition_penalty=1.1)
    assert scfg.random_seed is None
    GenerationSession._check_sampling_config(scfg)
    scfg.random_seed = 1234
    assert GenerationSession._native_sampling(scfg) == dict(top_k=40, top_p=0.9, temperature=0.8, repetition_penalty=1.1,
                                                            presence_penalty=0.0, min_length=1, random_seed=1234)
    GenerationSession._check_sampling_config(SamplingConfig(end_id=2, pad_id=2, top_k=0, top_p=0.5, presence_penalty=0.3,
                                                            min_length=8))
    GenerationSession._check_sampling_config(SamplingConfig(end_id=2, pad_id=2))
    GenerationSession._check_sampling_config(SamplingConfig(end_id=2, pad_id=2, num_beams=4, top_k=40))


def test_front_end_still_refuses_what_is_not_built():
    S = lambda **kw: SamplingConfig(end_id=2, pad_id=2, **kw)
    for kw in (dict(num_beams=2, repetition_penalty=1.1), dict(num_beams=2, presence_penalty=0.5), dict(num_beams=2, min_length=3),
               dict(num_beams=2, temperature=0.7), dict(num_beams=2, length_penalty=0.5)):
        with pytest.raises(NotImplementedError):
            GenerationSession._check_sampling_config(S(**kw))
    for kw in (dict(repetition_penalty=1.1, presence_penalty=0.5), dict(temperature=0.0), dict(temperature=-1.0)):
        with pytest.raises(ValueError):
            GenerationSession._check_sampling_config(S(**kw))
