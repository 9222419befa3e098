"""A different number of tokens per sequence in an append: the new C-ABI symbols, append_ref's `lengths`,
what GenerationSession._check_append_args refuses, and the headroom of the one-byte-cache cases of
tests/test_gpu_session_append_ragged.py.  No GPU."""
import os
import re

import numpy as np
import pytest

from tensorrt_llm.runtime import append_ref as R
from test_append_ref import DH, H, HKV, SCALE, rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED_LENGTHS = (20, 9)  # the synthetic-model cases of tests/test_gpu_session_append_ragged.py


def test_library_exports_the_ragged_append_symbols():
    from tensorrt_llm.plugin import capi
    text = open(os.path.join(ROOT, 'include', 'tllm_runtime_api.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    lib = capi.load_library()
    for name in ('tllm_attention_append_ragged', 'tllm_session_append_ragged', 'tllm_session_append_ragged_generate'):
        assert re.search(r'\b' + name + r'\s*\(', text), f'{name} is not declared'
        assert hasattr(lib, name), f'{name} is declared but not exported'


def ragged_inputs():
    r = np.random.default_rng(4)
    B, n, past = 3, 5, (6, 3, 0)
    q, k, v = rows(r, B, n)
    cache = r.standard_normal((B, 2, HKV, 6 + n, DH)).astype(np.float16)
    masked = np.zeros((B, 6 + n), np.int32)
    masked[0, 1:3] = 1
    return q, k, v, cache, past, masked


def test_lengths_equal_to_n_are_the_call_without_lengths():
    q, k, v, cache, past, masked = ragged_inputs()
    a = R.append_ref(q, k, v, cache, past, H, HKV, DH, SCALE, 'fp16', None, masked)
    b = R.append_ref(q, k, v, cache, past, H, HKV, DH, SCALE, 'fp16', None, masked, lengths=[5, 5, 5])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_a_ragged_sequence_is_the_uniform_call_on_its_first_rows_and_padding_is_never_read():
    q, k, v, cache, past, masked = ragged_inputs()
    lengths = (5, 1, 3)
    out, mass = R.append_ref(q, k, v, cache, past, H, HKV, DH, SCALE, 'fp16', None, masked, lengths=lengths)
    for b, nb in enumerate(lengths):
        s = slice(b, b + 1)
        want, wmass = R.append_ref(q[s, :nb], k[s, :nb], v[s, :nb], cache[s], past[s], H, HKV, DH, SCALE, 'fp16', None, masked[s])
        assert np.array_equal(out[b, :nb], want[0]) and np.array_equal(mass[b, :nb], wmass[0]), b
        assert (out[b, nb:] == 0).all() and (mass[b, nb:] == 0).all(), b
    # NaN in the padded rows of q, k and v changes nothing
    qn, kn, vn = q.copy(), k.copy(), v.copy()
    for b, nb in enumerate(lengths):
        for x in (qn, kn, vn):
            x[b, nb:] = np.nan
    out2, mass2 = R.append_ref(qn, kn, vn, cache, past, H, HKV, DH, SCALE, 'fp16', None, masked, lengths=lengths)
    assert np.array_equal(out, out2) and np.array_equal(mass, mass2)
    # positions() is what it was: the rows below n_b sit where the uniform call puts them
    assert R.positions([8, 10], 3, 8, [8, 5]).tolist() == [[8, 9, 10], [7, 8, 9]]
    with pytest.raises(ValueError):
        R.append_ref(q, k, v, cache, past, H, HKV, DH, SCALE, lengths=[5, 6, 1])
    with pytest.raises(ValueError):
        R.append_ref(q, k, v, cache, past, H, HKV, DH, SCALE, lengths=[5, 5])


def test_check_append_args_with_lengths():
    from tensorrt_llm.runtime import GenerationSession
    chk = GenerationSession._check_append_args
    B, W, S, V = 2, 4, 8, 128
    ids = np.full((B, W), 5, np.int32)
    chk(ids, B, S, V)                       # None: as before
    chk(ids, B, S, V, 1, None)
    chk(ids, B, S, V, 1, np.array([4, 1]))
    chk(ids, B, S, V, lengths=np.array([1, 4], np.int64))
    for bad in (np.array([4]), np.array([[4, 1]]), np.array([4, 1, 1]), np.array([0, 4]), np.array([4, W + 1]), np.array([-1, 2])):
        with pytest.raises(ValueError):
            chk(ids, B, S, V, 1, bad)
    with pytest.raises(TypeError):
        chk(ids, B, S, V, 1, np.array([4.0, 1.0]))
    # ids are range-checked below their length only
    behind = ids.copy()
    behind[0, 3], behind[1, 1] = -1, V
    chk(behind, B, S, V, 1, np.array([3, 1]))
    with pytest.raises(ValueError):
        chk(behind, B, S, V)
    for lens in ([4, 1], [3, 2]):
        with pytest.raises(ValueError):
            chk(behind, B, S, V, 1, np.array(lens))
    # everything refused without lengths is refused with them
    with pytest.raises(ValueError):
        chk(ids, B, S, V, 2, np.array([4, 1]))
    with pytest.raises(ValueError):
        chk(np.full((B, S + 1), 5, np.int32), B, S, V, 1, np.array([4, 1]))
    with pytest.raises(TypeError):
        chk(ids.astype(np.float32), B, S, V, 1, np.array([4, 1]))


def _int8_cache_modes():
    from test_gpu_session_append import INT8_CACHE_MODES
    return INT8_CACHE_MODES


@pytest.mark.parametrize('mode', _int8_cache_modes())
def test_headroom_of_the_one_byte_cache_ragged_session_cases(mode):
    """The pattern of tests/test_append_ref.py::test_headroom_of_the_one_byte_cache_session_cases for the ragged cases with a
    one-byte cache of tests/test_gpu_session_append_ragged.py (ONE_BYTE_INPUTS, lengths (20, 9)): for sequence b the ragged call is
    the uniform call with n = n_b, so the append rule runs once per distinct n_b, uniformly, on feed[:, :n_b], and row b of its
    logits is held to HALF of synth_bounds against the oracle's teacher-forced logits there - the GPU test has the other half.
    Measured: woq8 max 0.39 / 0.28 of the bound for sequences 0 / 1 and mean 0.40 / 0.32; sq_dyn_pc max 0.26 / 0.38, mean
    0.36 / 0.40."""
    from append_rule_model import append_logits
    from test_gpu_score import synth_bounds
    from test_gpu_session_append import ONE_BYTE_INPUTS, synth_inputs
    from oracle import quant_oracle as QO
    cfg, w, ids, lens, feed = synth_inputs(**ONE_BYTE_INPUTS)
    qmodel = QO.quantise_model(cfg, w, mode, 1, calib_ids=ids, calib_lens=lens)
    for b, nb in enumerate(RAGGED_LENGTHS):
        got, ref = append_logits(qmodel, ids, lens, feed[:, :nb])
        bmax, bmean = synth_bounds(mode, ref)  # (the oracle's logits at that index, both rows: the scale of the model's logits)
        d = np.abs(got[b].astype(np.float64) - ref[b])
        print(f'[headroom {mode} b={b} n_b={nb}] max {d.max():.4f} / {bmax:.4f} = {d.max() / bmax:.2f}, '
              f'mean {d.mean():.4f} / {bmean:.4f} = {d.mean() / bmean:.2f}')
        assert d.max() < 0.5 * bmax and d.mean() < 0.5 * bmean
