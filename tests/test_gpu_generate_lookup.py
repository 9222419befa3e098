"""tllm_session_generate_lookup on the deterministic trained parent: the tokens of plain greedy generation (a second session's
generate, and HF's - exact for fp16 and woq8 + int8 cache, see tests/test_gpu_session_verify.py), in the number and kinds of rounds
tensorrt_llm/runtime/spec_ref.py::simulate_lookup_rounds predicts (pinned on the CPU in tests/test_spec_ref.py)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import trained_parents as TP
from tensorrt_llm.runtime import spec_ref as R
from test_gpu_score import EX, quant_session
from test_spec_ref import LOOKUP_BATCHES, LOOKUP_G, LOOKUP_N, LOOKUP_NEW

pytestmark = pytest.mark.gpu
SETUP_NEW = LOOKUP_NEW + LOOKUP_N  # 56: the room the last verify pass needs behind the 48 generated tokens


@functools.lru_cache(maxsize=None)
def batch(rows):
    e = TP.load_eval('deterministic')
    lens = e['lengths'][list(rows)].astype(np.int32)
    S = int(lens.max())
    ids = np.zeros((len(rows), S), np.int32)
    for i, b in enumerate(rows):
        ids[i, :lens[i]] = e['prompts'][b, :lens[i]]
    return ids, lens, e['hf_tokens'][list(rows)].astype(np.int32)


def simulate(rows, n=LOOKUP_N):
    ids, lens, hf = batch(rows)
    return R.simulate_lookup_rounds([ids[i, :lens[i]] for i in range(len(rows))], list(hf), n, LOOKUP_G, LOOKUP_NEW)


def lookup(cfg, qmodel, rows, n=LOOKUP_N, new=LOOKUP_NEW, setup_new=SETUP_NEW):
    ids, lens, _ = batch(rows)
    s = quant_session(cfg, qmodel)
    s.setup(len(rows), ids.shape[1], setup_new)
    try:
        return s.generate_lookup(ids, lens, new, num_draft_tokens=n, max_ngram=LOOKUP_G)
    finally:
        s.close()


@pytest.mark.parametrize('rows', LOOKUP_BATCHES, ids=['prompts-0-1', 'prompts-1-6'])
@pytest.mark.parametrize('mode', ['fp16', 'woq8_int8kv'])
def test_lookup_generates_greedy_tokens_in_the_predicted_rounds(mode, rows):
    """prompts 0 and 1: prompt 0 reaches its limit in 6 rounds while prompt 1 runs 42 - the frozen path; every round of this
    batch is a verify pass, because prompt 0 has a draft in each of its rounds and a plain step is taken only while all sequences
    are live.  prompts 1 and 6: plain steps (from the graph) and verify passes alternate, and prompt 1 freezes one round early."""
    ids, lens, hf = batch(rows)
    cfg, qmodel = TP.quantised('deterministic', mode)
    S = ids.shape[1]
    out, st = lookup(cfg, qmodel, rows)
    g = quant_session(cfg, qmodel)
    g.setup(len(rows), S, SETUP_NEW)
    want = g.generate(ids, lens, LOOKUP_NEW)
    g.close()
    np.testing.assert_array_equal(out, want)
    np.testing.assert_array_equal(out[:, S:S + LOOKUP_NEW], hf[:, :LOOKUP_NEW])
    sim = simulate(rows)
    print(f'[lookup {mode} {rows}] {st}')
    for k in ('rounds', 'verify_rounds', 'step_rounds', 'drafted', 'accepted'):
        assert st[k] == sim[k], (k, st, {q: sim[q] for q in st})
    assert st['verify_rounds'] > 0 and st['rounds'] < LOOKUP_NEW
    if rows == LOOKUP_BATCHES[0]:
        solo = [simulate((b, ))['rounds'] for b in rows]
        assert solo[0] < solo[1] == st['rounds']  # prompt 0 is frozen for most of the call
    else:
        assert st['step_rounds'] > 0  # both kinds of round run


def test_a_repetitive_prompt_needs_a_third_of_the_passes_and_n_does_not_change_the_tokens():
    ids, lens, hf = batch((0, ))
    cfg, qmodel = TP.quantised('deterministic', 'fp16')
    S = ids.shape[1]
    out8, st8 = lookup(cfg, qmodel, (0, ))
    assert st8['rounds'] * 3 <= LOOKUP_NEW and st8['rounds'] == simulate((0, ))['rounds']
    out2, st2 = lookup(cfg, qmodel, (0, ), n=2)
    np.testing.assert_array_equal(out2, out8)
    np.testing.assert_array_equal(out8[0, S:S + LOOKUP_NEW], hf[0, :LOOKUP_NEW])
    assert st2['rounds'] == simulate((0, ), n=2)['rounds'] > st8['rounds']


def test_an_end_id_stops_a_sequence_as_generate_stops_it():
    rows = LOOKUP_BATCHES[0]
    ids, lens, hf = batch(rows)
    cfg, qmodel = TP.quantised('deterministic', 'fp16')
    end_id = int(hf[0, 20])
    a = quant_session(cfg, qmodel)
    a.setup(2, ids.shape[1], SETUP_NEW)
    out, st = a.generate_lookup(ids, lens, LOOKUP_NEW, end_id=end_id, pad_id=0, num_draft_tokens=LOOKUP_N, max_ngram=LOOKUP_G)
    want = a.generate(ids, lens, LOOKUP_NEW, end_id=end_id, pad_id=0)
    a.close()
    np.testing.assert_array_equal(out, want)
    first = int(np.nonzero(hf[0] == end_id)[0][0])
    assert first < LOOKUP_NEW and (out[0, ids.shape[1] + first:] == end_id).all()


def test_refusals():
    cfg, qmodel = TP.quantised('deterministic', 'fp16')
    with pytest.raises(RuntimeError, match="exceed setup's max_new_tokens"):
        lookup(cfg, qmodel, (0, ), new=LOOKUP_NEW + 1)  # 49 + 8 > 56
    with pytest.raises(RuntimeError, match='num_draft_tokens'):
        lookup(cfg, qmodel, (0, ), n=1)
    with pytest.raises(RuntimeError, match='num_draft_tokens'):
        lookup(cfg, qmodel, (0, ), n=33, setup_new=LOOKUP_NEW + 33)
    ids, lens, _ = batch((0, ))
    s = quant_session(cfg, qmodel)
    s.setup(1, ids.shape[1], SETUP_NEW)
    s.set_sampling(top_k=40)
    with pytest.raises(RuntimeError, match='speculative sampling is not built'):
        s.generate_lookup(ids, lens, LOOKUP_NEW)
    s.close()
    s = quant_session(cfg, qmodel)
    s.setup(1, ids.shape[1], SETUP_NEW, 2)
    with pytest.raises(RuntimeError, match='not built'):
        s.generate_lookup(ids, lens, LOOKUP_NEW)
    s.close()


# ------------------------------------------------------------------------------------------------ front-end
def test_decode_lookup_returns_what_decode_returns():
    from tensorrt_llm import Mapping
    from tensorrt_llm.quantization import QuantMode
    from tensorrt_llm.runtime import GenerationSession, ModelConfig, SamplingConfig
    from test_frontend import build_tiny_engine
    engine, _, t = build_tiny_engine(QuantMode(0))
    ids, lens = t['ids'], t['input_lengths']
    B, S = ids.shape
    dec = GenerationSession(ModelConfig(vocab_size=128, num_layers=2, num_heads=2, hidden_size=64), engine, Mapping(1, 0))
    dec.setup(B, S, 24)
    scfg = SamplingConfig(end_id=-1, pad_id=0)
    want = dec.decode(ids, lens, scfg, max_new_tokens=16)
    got = dec.decode_lookup(ids, lens, scfg, num_draft_tokens=8, max_ngram=3)  # max_new_tokens: 24 - 8
    assert got.shape == want.shape == (B, 1, S + 24)
    np.testing.assert_array_equal(got, want)
    st = dec.lookup_stats
    assert st['rounds'] == st['verify_rounds'] + st['step_rounds'] and 1 <= st['rounds'] <= 15
    v = dec.verify(want[:, 0, S + 15:S + 16])  # the pending token alone: a greedy step
    assert v['accepted'].tolist() == [0] * B and v['logits'].shape == (B, 128) and v['log_probs'].shape == (B, 1)
    with pytest.raises(ValueError):
        dec.decode_lookup(ids, lens, scfg, max_new_tokens=17)


def test_run_py_prints_the_same_tokens_with_prompt_lookup(tmp_path):
    from test_frontend import TINY
    out = tmp_path / 'eng'
    subprocess.run([sys.executable, os.path.join(EX, 'build.py'), '--output_dir', str(out), '--log_level', 'error'] + TINY,
                   check=True, cwd=EX, timeout=300)
    np.save(tmp_path / 'in.npy', np.array([5, 17, 99, 3, 64, 5, 17, 99], np.int32))
    got = {}
    for name, extra in (('plain', []), ('lookup', ['--prompt_lookup_tokens', '8'])):
        r = subprocess.run([sys.executable, os.path.join(EX, 'run.py'), '--max_output_len', '12', '--engine_dir', str(out),
                            '--input_tokens', str(tmp_path / 'in.npy'), '--output_npy', str(tmp_path / f'{name}.npy'),
                            '--num_runs', '1'] + extra, check=True, cwd=EX, timeout=600, capture_output=True, text=True)
        assert 'llama-run (mean latency:' in r.stdout and ('prompt lookup:' in r.stdout) == bool(extra)
        got[name] = np.load(tmp_path / f'{name}.npy')
    assert got['plain'].shape == (1, 20)
    np.testing.assert_array_equal(got['lookup'], got['plain'])
