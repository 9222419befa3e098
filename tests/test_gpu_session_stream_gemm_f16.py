"""Session key stream_gemm = 2: fp16 weights on kernels/gemm_stream_f16.hip.  An fp16 engine runs the projections of an append of 12
ids and a verify of 16 ids (24 / 32 rows at batch 2) and the verify's lm_head on it, held to the teacher-forced oracle and the
bounds tests/test_gpu_session_append.py holds the keyless session to; a SmoothQuant engine keeps the layers of value 1 bit for bit
and streams its fp16 head.  Prompts of 36 rows each: the prefill of 72 rows stays outside the range."""
import numpy as np
import pytest

from tensorrt_llm.runtime.native import NativeSession
from test_gpu_score import kv_bytes, quant_session, synth_bounds, synth_model
from test_gpu_session_append import close, forced_steps
from test_gpu_session_stream_gemm_woq import N_APPEND, N_VERIFY, model

pytestmark = pytest.mark.gpu


def routed(rows, layers, head_rows):
    """calls value 2 sends to a stream in a pass of `rows` rows whose head runs on `head_rows` rows: all five projections of a
    layer at 9 .. 64 rows, and the head where 9 .. 32 rows go through it outside the generation step"""
    return (5 * layers if 9 <= rows <= 64 else 0) + (1 if 9 <= head_rows <= 32 else 0)


def test_fp16_append_and_verify_against_the_teacher_forced_oracle():
    cfg, qmodel, ids, lens, feed, ref = model('fp16')
    L = cfg['num_layers']
    held = lambda got, z, tag: close(got, z, *synth_bounds('fp16', z), tag=f'fp16 {tag}')
    s = quant_session(cfg, qmodel, stream_gemm=2)
    s.setup(2, ids.shape[1], N_APPEND + N_VERIFY + 2)
    s.context(ids, lens)
    assert s.stream_gemm_launches() == 0  # 72 rows, and the head on 2
    s.append(feed[:, :N_APPEND])
    held(s.logits(), ref[N_APPEND], 'append 12')
    want = routed(2 * N_APPEND, L, 2)
    assert s.stream_gemm_launches() == want
    # the session goes on from the state the pass left; a generation step streams nothing
    held(forced_steps(s, feed[:, N_APPEND:N_APPEND + 1])[0], ref[N_APPEND + 1], 'step behind the append')
    assert s.stream_gemm_launches() == want
    s.close()
    # verify from the prompt: row i is the distribution behind feed[:, i]; all 32 rows go through the head
    s = quant_session(cfg, qmodel, stream_gemm=2)
    s.setup(2, ids.shape[1], N_APPEND + N_VERIFY + 2)
    s.context(ids, lens)
    accepted, _ = s.verify(feed[:, :N_VERIFY])
    rows = s.verify_logits(N_VERIFY)
    for i in range(N_VERIFY):
        held(rows[:, i], ref[i + 1], f'verify row {i}')
    assert s.stream_gemm_launches() == routed(2 * N_VERIFY, L, 2 * N_VERIFY)
    assert accepted.tolist() == [0, 0]  # random drafts: none is kept
    held(forced_steps(s, feed[:, 1:2])[0], ref[2], 'step behind the verify')
    s.close()


def test_smoothquant_layers_keep_the_bits_of_value_1_and_the_head_streams():
    mode = 'sq_static_pc'
    cfg, qmodel, ids, lens, feed, ref = model(mode)
    L, S, NEW = cfg['num_layers'], ids.shape[1], N_VERIFY + 2
    got = {}
    for value in (1, 2):
        s = quant_session(cfg, qmodel, stream_gemm=value)
        s.setup(2, S, NEW)
        s.context(ids, lens)
        assert s.stream_gemm_launches() == 0
        s.verify(feed[:, :N_VERIFY])
        rows = s.verify_logits(N_VERIFY)
        for i in range(N_VERIFY):
            close(rows[:, i], ref[i + 1], *synth_bounds(mode, ref[i + 1]), tag=f'{mode} value {value} verify row {i}')
        got[value] = (s.stream_gemm_launches(), kv_bytes(s, L, 2 * 2 * cfg['num_heads'] * (S + NEW) * (cfg['hidden_size'] // cfg['num_heads']) * 2))
        s.close()
    assert got[1][0] > 0 and got[2][0] == got[1][0] + 1  # one head call
    for a, b in zip(got[1][1], got[2][1]):
        np.testing.assert_array_equal(a, b)


def test_another_value_is_refused():
    cfg, _ = synth_model(11)
    with pytest.raises(RuntimeError, match='stream_gemm'):
        NativeSession(dict(cfg, quant_mode=0, stream_gemm=3))
