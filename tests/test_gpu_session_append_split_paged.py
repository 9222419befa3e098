"""Session key append_split = 2 on the paged KV cache: a linear and a paged session, both with the value, side by side on the inputs
of tests/test_gpu_session_append_paged.py - everything equal element for element (tests/test_gpu_session_append_split.py holds the
linear session with the key to the oracle)."""
import numpy as np
import pytest

from tensorrt_llm.runtime.native import NativeSession
from test_gpu_session_append_paged import MODES, NEW, engine, side_by_side, state

pytestmark = pytest.mark.gpu


def script(cfg, ids, lens, feed, lookup_drafts):
    more = np.random.default_rng(17).integers(3, 500, (2, 9)).astype(np.int32)
    rep = ids.copy()
    for b in range(2):  # a prompt that repeats itself: the lookup loop finds drafts in it
        rep[b, :lens[b]] = np.resize(ids[b, :4], lens[b])

    def run(s):
        s.setup(2, ids.shape[1], NEW)
        s.context(ids, lens)
        s.append(feed[:, :3])
        out = [s.logits()] + state(s)
        s.step(1, use_graph=True)
        out.append(s.logits())
        acc, lp = s.verify(feed[:, 3:7])
        out += [acc, lp, s.logits(), s.verify_top1(4)] + state(s)
        s.append(more[:, :5], [5, 2])
        out += [s.logits()] + state(s)
        out.append(s.append_generate(more[:, 5:9], 3))
        out += [s.logits()] + state(s)
        assert s.append_split_launches() == 4 * cfg['num_layers'] and s.append_launches() == (0, 0)
        tok, stats = s.generate_lookup(rep, lens, 24, num_draft_tokens=5, max_ngram=3)
        assert stats['verify_rounds'] > 0 or not lookup_drafts  # (a quantised model may leave the prompt's tokens at once)
        assert s.append_split_launches() == (4 + stats['verify_rounds']) * cfg['num_layers'] and s.append_launches() == (0, 0)
        return out + [tok, np.array([stats[k] for k in sorted(stats)])] + state(s)
    return run


@pytest.mark.parametrize('T', [8, 64])
@pytest.mark.parametrize('mode', MODES)
def test_every_append_pass_equals_the_linear_session_with_the_key(mode, T):
    cfg, tensors, keys, ids, lens, feed = engine(mode)
    side_by_side(script(cfg, ids, lens, feed, mode == 'fp16-fp16'), cfg, tensors, keys, T, append_split=2)


def test_the_value_pairs_with_paged_append_at_create():
    paged = dict(engine('fp16-fp16')[0], quant_mode=0, paged_kv_cache=1, tokens_per_block=8)
    NativeSession(dict(paged, paged_append=1, append_split=2)).close()
    with pytest.raises(RuntimeError, match='paged_append'):
        NativeSession(dict(paged, append_split=2))
    with pytest.raises(RuntimeError, match='append_split'):
        NativeSession(dict(paged, paged_append=1, append_split=1))
