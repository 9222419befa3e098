"""Session key stream_gemm: a session with it is held bit for bit - logits, tokens, the whole KV cache - to one without, on the
synthetic SmoothQuant model (hidden 256, inter 512) of the append tests.  Prompts of 72 rows: the prefill stays outside the range."""
import functools

import numpy as np
import pytest

from oracle import quant_oracle as QO
from tensorrt_llm.runtime.native import NativeSession
from test_gpu_score import kv_bytes, quant_session, synth_model

pytestmark = pytest.mark.gpu
NEW = 20
GEMMS_PER_LAYER = 5  # qkv, dense, fc, gate, proj (below 32 rows the dual SwiGLU GEMM does not run)


@functools.lru_cache(maxsize=None)
def model(mode, B):
    cfg, w = synth_model(11)
    cfg = dict(cfg, max_position_embeddings=256)
    S = 72 // B
    r = np.random.default_rng(5)
    ids = r.integers(3, cfg['vocab_size'], (B, S)).astype(np.int32)
    lens = np.array([S - 2 * b for b in range(B)], np.int32)
    for b in range(B):
        ids[b, lens[b]:] = 2
    feed = r.integers(3, cfg['vocab_size'], (B, 16)).astype(np.int32)
    return cfg, QO.quantise_model(cfg, w, mode, 0, calib_ids=ids, calib_lens=lens), ids, lens, feed


def append_12(s, feed):
    s.append(feed[:, :12])
    return [s.logits()]


def verify_16(s, feed):
    accepted, log_probs = s.verify(feed[:, :16])
    return [s.verify_logits(16), accepted, log_probs, s.logits()]


def ragged_5_3_4(s, feed):
    s.append(feed[:, :5], lengths=np.array([5, 3, 4], np.int32))
    return [s.logits()]


@pytest.mark.parametrize('mode,B,scenario', [('sq_dyn_pc', 1, append_12), ('sq_static_pc', 1, verify_16), ('sq_dyn_pc', 1, verify_16),
                                             ('sq_static_pc', 3, ragged_5_3_4)],
                         ids=['append12-dyn', 'verify16-static', 'verify16-dyn', 'ragged15-static'])
def test_the_key_changes_no_bit(mode, B, scenario):
    cfg, qmodel, ids, lens, feed = model(mode, B)
    S, L = ids.shape[1], cfg['num_layers']
    got = []
    for keys in (dict(stream_gemm=1), {}):
        s = quant_session(cfg, qmodel, **keys)
        s.setup(B, S, NEW)
        s.context(ids, lens)
        assert s.stream_gemm_launches() == 0  # 72 rows
        out = scenario(s, feed)
        assert s.stream_gemm_launches() == (GEMMS_PER_LAYER * L if keys else 0)
        s.step(1)  # the session goes on from the state the pass left
        out += [s.logits(), s.output_ids()]
        out += kv_bytes(s, L, B * 2 * cfg['num_heads'] * (S + NEW) * (cfg['hidden_size'] // cfg['num_heads']) * 2)
        got.append(out)
        s.close()
    for a, b in zip(*got):
        np.testing.assert_array_equal(a, b)


def test_passes_outside_the_range_and_plain_generate_do_not_count():
    cfg, qmodel, ids, lens, feed = model('sq_dyn_pc', 1)
    s = quant_session(cfg, qmodel, stream_gemm=1)
    s.setup(1, ids.shape[1], NEW)
    s.generate(ids, lens, 4)
    assert s.stream_gemm_launches() == 0
    s.context(ids, lens)
    s.append(feed[:, :8])
    assert s.stream_gemm_launches() == 0
    s.close()


def test_the_key_is_refused_on_an_engine_that_is_not_smoothquant():
    cfg, _ = synth_model(11)
    with pytest.raises(RuntimeError, match='stream_gemm'):
        NativeSession(dict(cfg, quant_mode=0, stream_gemm=1))
