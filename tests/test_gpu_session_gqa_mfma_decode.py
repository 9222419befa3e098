"""Session key gqa_mfma_decode: the generation step of a grouped session runs its attention on the grouped MFMA kernel.  The model
is the grouped synthetic one of tests/test_gpu_session_append.py (H 4, Hkv 2, head size 64 - the smallest the kernel serves; the
head size 32 of tests/test_gpu_gqa_session.py is refused), the oracle the multi-head model with every K/V head repeated.  Bounds:
synth_bounds for the fp16 cache; and, the rule of tests/test_gpu_gqa_session.py, at most 1.25 x the error of the sibling engine that
computes the same function - here the keyless session on the same cache type - against the same oracle logits."""
import numpy as np
import pytest

from oracle import quant_oracle as QO
from tensorrt_llm.runtime import gqa_ref as G
from tensorrt_llm.runtime.native import NativeSession
from test_gpu_score import synth_bounds
from test_gpu_session_append import synth_inputs

pytestmark = pytest.mark.gpu
H, HKV, DH, STEPS, INT8_KV = 4, 2, 64, 4, 32
_state = {}


def model():
    if not _state:
        cfg, w, ids, lens, feed = synth_inputs()
        wg, wm = dict(w), dict(w)
        for i in range(cfg['num_layers']):
            k = f'layers.{i}.attention.qkv.weight'
            wg[k] = np.ascontiguousarray(G.fold_qkv(w[k].T, H, HKV, DH).T)
            wm[k] = np.ascontiguousarray(G.expand_qkv_weight(wg[k], H, HKV, DH))
        feed = feed[:, :STEPS]
        ref, _ = QO.run_fp16_model(cfg, wm, ids, lens, 1 + STEPS, feed_ids=feed)
        _state.update(cfg=cfg, wg=wg, ids=ids, lens=lens, feed=feed, ref=ref)
    return _state


def session(kind='fp16', **keys):
    m = model()
    s = NativeSession(dict(m['cfg'], quant_mode=INT8_KV if kind == 'int8' else 0, **keys))
    for k, v in m['wg'].items():
        s.set_tensor(k, v)
    if kind == 'int8':
        for i in range(m['cfg']['num_layers']):
            s.set_tensor(f'layers.{i}.attention.kv_orig_quant_scale', np.array([16.0], np.float32))
            s.set_tensor(f'layers.{i}.attention.kv_quant_orig_scale', np.array([1 / 16.0], np.float32))
    s.finalize()
    return s


def forced(s, use_graph):
    m = model()
    s.context(m['ids'], m['lens'])
    out = []
    for i in range(STEPS):
        s.force_tokens(m['feed'][:, i])
        s.step(1, use_graph=use_graph)
        out.append(s.logits())
    return np.stack(out)


@pytest.mark.parametrize('kind', ['fp16', 'int8'])
def test_forced_steps_with_the_key_against_the_oracle_eager_and_replayed(kind):
    m = model()
    L, ref = m['cfg']['num_layers'], np.stack(m['ref'][1:1 + STEPS])
    got = {}
    for keyed in (True, False):
        s = session(kind, num_kv_heads=HKV, **(dict(gqa_mfma_decode=1) if keyed else {}))
        s.setup(2, m['ids'].shape[1], STEPS + 1)
        eager = forced(s, False)
        assert s.grouped_decode_launches() == (L * STEPS if keyed else 0)
        graph = forced(s, True)
        assert s.grouped_decode_launches() == (2 * L * STEPS if keyed else 0)
        assert s.decode_form() & 1 == 0  # grouped heads run the separate-launch step
        s.close()
        np.testing.assert_array_equal(eager.view(np.uint32), graph.view(np.uint32))
        got[keyed] = eager
    e_key, e_rule = np.abs(got[True] - ref).max(), np.abs(got[False] - ref).max()
    print(f'[{kind}] max |logits - oracle| over {STEPS} forced steps: with the key {e_key:.3e}, without {e_rule:.3e}')
    assert np.isfinite(got[True]).all() and e_key <= 1.25 * e_rule
    if kind == 'fp16':
        for i in range(STEPS):
            bmax, bmean = synth_bounds('fp16', ref[i])
            d = np.abs(got[True][i] - ref[i])
            assert d.max() <= bmax and d.mean() <= bmean, (i, d.max(), bmax, d.mean(), bmean)


def test_sessions_the_kernel_does_not_serve_refuse_the_key_by_name():
    m = model()
    with pytest.raises(RuntimeError, match='gqa_mfma_decode'):  # multi-head
        NativeSession(dict(m['cfg'], quant_mode=0, gqa_mfma_decode=1))
    with pytest.raises(RuntimeError, match='gqa_mfma_decode'):  # paged
        NativeSession(dict(m['cfg'], quant_mode=0, num_kv_heads=HKV, paged_kv_cache=1, gqa_mfma_decode=1))
    s = session('fp16', num_kv_heads=HKV, gqa_mfma_decode=1)
    with pytest.raises(RuntimeError, match='gqa_mfma_decode'):  # beam
        s.setup(2, m['ids'].shape[1], STEPS + 1, 2)
    s.close()
