"""Session key append_split: the append passes of N <= 32 ids run the split-KV attention kernel (head size 64: the synthetic model and
the trained parent), held to the oracle and the bounds tests/test_gpu_session_append.py holds the keyless session to."""
import numpy as np
import pytest

import test_gpu_generate_lookup as GL
import trained_parents as TP
from oracle import quant_oracle as QO
from tensorrt_llm.runtime.native import NativeSession
from test_gpu_score import quant_session, synth_bounds
from test_gpu_session_append import close, forced_steps, synth_inputs

pytestmark = pytest.mark.gpu
N_APPEND, N_VERIFY = 5, 4


def test_append_and_verify_on_the_split_kernel_against_the_teacher_forced_oracle():
    cfg, w, ids, lens, feed = synth_inputs()
    feed = feed[:, :N_APPEND + N_VERIFY + 1]
    L = cfg['num_layers']
    qmodel = QO.quantise_model(cfg, w, 'fp16', 0, calib_ids=ids, calib_lens=lens)
    ref, _ = QO.run_model(qmodel, ids, lens, 1 + feed.shape[1], feed_ids=feed)
    for keys in (dict(append_split=1), {}):
        s = quant_session(cfg, qmodel, **keys)
        s.setup(2, ids.shape[1], feed.shape[1] + 1)
        s.context(ids, lens)
        s.append(feed[:, :N_APPEND])
        z = ref[N_APPEND]
        close(s.logits(), z, *synth_bounds('fp16', z), tag=f'append {N_APPEND} {keys}')
        s.verify(feed[:, N_APPEND:N_APPEND + N_VERIFY])
        rows = s.verify_logits(N_VERIFY)
        for i in range(N_VERIFY):  # row i: the distribution behind feed[:, N_APPEND + i]
            z = ref[N_APPEND + i + 1]
            close(rows[:, i], z, *synth_bounds('fp16', z), tag=f'verify row {i} {keys}')
        # one launch per layer and pass, on the split kernel with the key and on the rule's (the wave kernel at n < 16) without
        assert s.append_split_launches() == (2 * L if keys else 0)
        assert s.append_launches() == ((0, 0) if keys else (2 * L, 0))
        # a pass the split kernel does not serve follows the rule: the session goes on from here one forced step
        forced_steps(s, feed[:, -1:])
        s.close()


def test_lookup_generates_the_greedy_tokens_with_the_key():
    rows = GL.LOOKUP_BATCHES[0]
    ids, lens, hf = GL.batch(rows)
    cfg, qmodel = TP.quantised('deterministic', 'fp16')
    S = ids.shape[1]
    s = quant_session(cfg, qmodel, append_split=1)
    s.setup(len(rows), S, GL.SETUP_NEW)
    out, st = s.generate_lookup(ids, lens, GL.LOOKUP_NEW, num_draft_tokens=GL.LOOKUP_N, max_ngram=GL.LOOKUP_G)
    assert st['verify_rounds'] > 0 and s.append_split_launches() == st['verify_rounds'] * cfg['num_layers']
    assert s.append_launches() == (0, 0)
    s.close()
    g = quant_session(cfg, qmodel)
    g.setup(len(rows), S, GL.SETUP_NEW)
    want = g.generate(ids, lens, GL.LOOKUP_NEW)
    g.close()
    np.testing.assert_array_equal(out, want)
    np.testing.assert_array_equal(out[:, S:S + GL.LOOKUP_NEW], hf[:, :GL.LOOKUP_NEW])


def test_the_key_is_refused_on_a_paged_cache():
    cfg, _, _, _, _ = synth_inputs()
    with pytest.raises(RuntimeError, match='append_split'):
        NativeSession(dict(cfg, quant_mode=0, paged_kv_cache=1, append_split=1))
