"""Session key stream_gemm on weight-only engines: the projections of an append of 12 ids and a verify of 16 ids (24 / 32 rows at
batch 2) run kernels/gemm_stream_woq.hip, held to the teacher-forced oracle and the bounds tests/test_gpu_session_append.py holds
the keyless session to.  Prompts of 36 rows each: the prefill of 72 rows stays outside the range."""
import functools

import numpy as np
import pytest

from oracle import quant_oracle as QO
from test_gpu_score import quant_session, synth_bounds
from test_gpu_session_append import close, forced_steps, synth_inputs

pytestmark = pytest.mark.gpu
N_APPEND, N_VERIFY = 12, 16


def routed(rows, layers):
    """gemm() calls the session's rule sends to the stream in a pass of `rows` rows: all five projections of a layer at 9 .. 64"""
    return 5 * layers if 9 <= rows <= 64 else 0


@functools.lru_cache(maxsize=None)
def model(mode):
    cfg, w, ids, lens, _ = synth_inputs(S=36)
    feed = np.random.default_rng(7).integers(3, cfg['vocab_size'], (2, N_APPEND + N_VERIFY)).astype(np.int32)
    qmodel = QO.quantise_model(cfg, w, mode, 0, calib_ids=ids, calib_lens=lens)
    ref, _ = QO.run_model(qmodel, ids, lens, 1 + N_VERIFY, feed_ids=feed[:, :N_VERIFY])
    return cfg, qmodel, ids, lens, feed, ref


@pytest.mark.parametrize('keys', [dict(stream_gemm=1), {}], ids=['key', 'keyless'])
@pytest.mark.parametrize('mode', ['woq8', 'woq4'])
def test_append_and_verify_against_the_teacher_forced_oracle(mode, keys):
    cfg, qmodel, ids, lens, feed, ref = model(mode)
    L = cfg['num_layers']
    held = lambda got, z, tag: close(got, z, *synth_bounds(mode, z), tag=f'{mode} {tag} {keys}')
    s = quant_session(cfg, qmodel, **keys)
    s.setup(2, ids.shape[1], N_APPEND + N_VERIFY + 2)
    s.context(ids, lens)
    assert s.stream_gemm_launches() == 0  # 72 rows
    s.append(feed[:, :N_APPEND])
    held(s.logits(), ref[N_APPEND], 'append 12')
    want = routed(2 * N_APPEND, L) if keys else 0
    assert s.stream_gemm_launches() == want
    # the session goes on from the state the pass left
    held(forced_steps(s, feed[:, N_APPEND:N_APPEND + 1])[0], ref[N_APPEND + 1], 'step behind the append')
    assert s.stream_gemm_launches() == want
    s.close()
    # verify from the prompt: row i is the distribution behind feed[:, i]
    s = quant_session(cfg, qmodel, **keys)
    s.setup(2, ids.shape[1], N_APPEND + N_VERIFY + 2)
    s.context(ids, lens)
    accepted, _ = s.verify(feed[:, :N_VERIFY])
    rows = s.verify_logits(N_VERIFY)
    for i in range(N_VERIFY):
        held(rows[:, i], ref[i + 1], f'verify row {i}')
    assert s.stream_gemm_launches() == (routed(2 * N_VERIFY, L) if keys else 0)
    # random drafts: none is kept, the cache holds feed[:, 0] alone behind the prompt, and a forced step goes on from there
    assert accepted.tolist() == [0, 0]
    held(forced_steps(s, feed[:, 1:2])[0], ref[2], 'step behind the verify')
    s.close()
