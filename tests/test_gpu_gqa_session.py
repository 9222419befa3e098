"""A grouped-query LLaMA end to end on the GPU: a random HF LlamaForCausalLM with num_key_value_heads = 2 (4 heads, hidden 128,
2 layers) goes through hf_llama_convert.py and build.py (--model_dir, the K/V head count read from config.ini) into an engine, the engine through
tllm_engine_verify into the C++ session.  Context logits and the logits of 8 teacher-forced generation steps are held to the numpy
oracle's layer functions on weights expanded by gqa_ref.expand_qkv_weight.

Tolerance: the K/V-REPLICATED multi-head engine of the same model (k_proj / v_proj rows repeated per query head - the same
function) is built in the same test and its error against the same oracle logits is measured; the grouped engine is allowed 1.25 x
that error (the margin tests/test_gpu_trained_accuracy.py gives teacher-forced logits).  Both errors are printed.  The oracle
logits are those of fp16 weights and an fp16 cache in every mode, so a mode's quantisation error is in both engines' figures."""
import ctypes
import os
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, 'trtllm-llama_amd', 'examples', 'llama_quant')
sys.path.insert(0, EX)

from oracle import llama_oracle as O  # noqa: E402
from tensorrt_llm.runtime import gqa_ref as G  # noqa: E402
from tensorrt_llm.runtime.native import NativeSession  # noqa: E402

pytestmark = pytest.mark.gpu

H, HKV, D, DH, V, LAYERS, INTER = 4, 2, 128, 32, 96, 2, 128
B, S, NEW, STEPS = 2, 12, 10, 8
LENS = np.array([S, 7], np.int32)
MODES = {'fp16': [], 'fp16_kv8': ['--int8_kv_cache'], 'fp16_fp8kv': ['--fp8_kv_cache'], 'woq8': ['--use_weight_only']}
_state = {}


def hf_models():
    """(grouped state dict, replicated multi-head state dict, HF directories of both)"""
    if 'hf' not in _state:
        import torch
        from transformers import LlamaConfig, LlamaForCausalLM
        cfg = dict(hidden_size=D, num_attention_heads=H, num_key_value_heads=HKV, intermediate_size=INTER, vocab_size=V,
                   num_hidden_layers=LAYERS, max_position_embeddings=64, rms_norm_eps=1e-6, attention_bias=False,
                   tie_word_embeddings=False)
        torch.manual_seed(0)
        m = LlamaForCausalLM(LlamaConfig(**cfg)).float().eval()
        with torch.no_grad():
            for p in m.parameters():
                if p.ndim == 2:
                    p.mul_(2.0)
        mha = LlamaForCausalLM(LlamaConfig(**dict(cfg, num_key_value_heads=H))).float().eval()
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        for k in list(sd):
            if 'k_proj' in k or 'v_proj' in k:
                sd[k] = sd[k].reshape(HKV, DH, D).repeat_interleave(H // HKV, dim=0).reshape(H * DH, D)
        mha.load_state_dict(sd)
        root = tempfile.mkdtemp()
        dirs = []
        for name, model in (('gqa', m), ('mha', mha)):
            d = os.path.join(root, name)
            model.save_pretrained(d, safe_serialization=True)
            dirs.append(d)
        _state['hf'] = (m, mha, dirs)
    return _state['hf']


def engine(kind, mode, extra=()):
    """HF directory -> hf_llama_convert (KV-cache calibration on seeded prompts) -> build.py --model_dir -> engine bytes"""
    key = (kind, mode, tuple(extra))
    if key not in _state:
        import build as Bd
        import hf_llama_convert as C
        _, _, dirs = hf_models()
        if ('ft', kind) not in _state:
            _state[('ft', kind)] = str(C.run_conversion(C.ProgArgs(out_dir=tempfile.mkdtemp(), in_file=dirs[0 if kind == 'gqa' else 1],
                                                                  calibrate_kv_cache=True, calib_samples=2, calib_len=16)))
        out = tempfile.mkdtemp()
        Bd.run_build(['--model_dir', _state[('ft', kind)], '--output_dir', out, '--max_batch_size', '4', '--max_input_len', str(S),
                      '--max_output_len', str(NEW), '--log_level', 'error'] + MODES[mode] + list(extra))
        f, = [f for f in os.listdir(out) if f.endswith('.engine')]
        _state[key] = open(os.path.join(out, f), 'rb').read()
        _state[('dir', ) + key] = out
    return _state[key]


def prompts():
    r = np.random.default_rng(5)
    ids = r.integers(3, V, (B, S)).astype(np.int32)
    ids[1, LENS[1]:] = 2
    return ids


def oracle_weights():
    """the oracle's weight dict of the grouped model: fp16 values, the fused QKV weight expanded to the multi-head layout"""
    if 'weights' not in _state:
        m, _, _ = hf_models()
        sd = {k: v.detach().numpy().astype(np.float16).astype(np.float32) for k, v in m.state_dict().items()}
        w = {'vocab_embedding.weight': sd['model.embed_tokens.weight'], 'ln_f.weight': sd['model.norm.weight'],
             'lm_head.weight': sd['lm_head.weight'], 'layers': []}
        for i in range(LAYERS):
            p = f'model.layers.{i}.'
            qkv = np.concatenate([sd[p + f'self_attn.{n}_proj.weight'] for n in 'qkv'], axis=0)
            w['layers'].append({'input_layernorm.weight': sd[p + 'input_layernorm.weight'],
                                'attention.qkv.weight': G.expand_qkv_weight(qkv, H, HKV, DH),
                                'attention.dense.weight': sd[p + 'self_attn.o_proj.weight'],
                                'post_layernorm.weight': sd[p + 'post_attention_layernorm.weight'],
                                'mlp.fc.weight': sd[p + 'mlp.gate_proj.weight'], 'mlp.gate.weight': sd[p + 'mlp.up_proj.weight'],
                                'mlp.proj.weight': sd[p + 'mlp.down_proj.weight']})
        _state['weights'] = w
    return _state['weights']


def oracle_logits(forced):
    """context logits + the logits after each teacher-forced step, fp16 weights and cache, expanded weights"""
    if 'oracle' not in _state:
        w = oracle_weights()
        ids = prompts()
        smax = S + NEW
        caches = [np.zeros((B, 2, H, smax, DH), np.float16) for _ in range(LAYERS)]
        out = [O.llama_logits_context(ids, w, caches, LENS, H)]
        masked = np.zeros((B, smax), np.int32)
        for b in range(B):
            masked[b, LENS[b]:S] = 1
        for t in range(STEPS):
            out.append(O.llama_logits_decode(forced[t], w, caches, [S + t] * B, LENS, S, S + t, H, masked))
        _state['oracle'] = (np.stack(out), caches)
    return _state['oracle']


FORCED = np.random.default_rng(11).integers(3, V, (STEPS, B)).astype(np.int32)


def run_forced(eng):
    s = NativeSession(engine=eng)
    try:
        s.setup(B, S, NEW)
        s.context(prompts(), LENS)
        form = s.decode_form()
        out = [s.logits()]
        for t in range(STEPS):
            s.force_tokens(FORCED[t])
            s.step(1, use_graph=False)
            out.append(s.logits())
        return np.stack(out), form
    finally:
        s.close()


@pytest.mark.parametrize('mode', sorted(MODES))
def test_logits_against_the_oracle_within_the_replicated_mha_engines_error(mode):
    ref, _ = oracle_logits(FORCED)
    got, form = run_forced(engine('gqa', mode))
    mha, _ = run_forced(engine('mha', mode))
    assert form & 1 == 0  # grouped heads run the separate-launch step
    assert np.isfinite(got).all()
    e_ctx, m_ctx = np.abs(got[0] - ref[0]).max(), np.abs(mha[0] - ref[0]).max()
    e_dec, m_dec = np.abs(got[1:] - ref[1:]).max(), np.abs(mha[1:] - ref[1:]).max()
    print(f'[{mode}] max |logits - oracle|: context gqa {e_ctx:.3e} mha {m_ctx:.3e}; 8 forced steps gqa {e_dec:.3e} mha {m_dec:.3e}')
    assert e_ctx <= 1.25 * m_ctx and e_dec <= 1.25 * m_dec


_hip = None


def read_cache(s, layer, nbytes, dtype):
    global _hip
    if _hip is None:
        _hip = ctypes.CDLL('libamdhip64.so')
        _hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    host = np.empty(nbytes // np.dtype(dtype).itemsize, dtype)
    assert _hip.hipDeviceSynchronize() == 0
    assert _hip.hipMemcpy(host.ctypes.data, s.kv_cache_ptr(layer), nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return host


@pytest.mark.parametrize('mode,dtype', [('fp16', np.float16), ('fp16_kv8', np.int8)])
def test_the_cache_after_context_is_the_fold_of_the_mha_engines_cache(mode, dtype):
    smax = S + NEW
    caches = {}
    for kind, heads in (('gqa', HKV), ('mha', H)):
        s = NativeSession(engine=engine(kind, mode))
        try:
            s.setup(B, S, NEW)
            s.context(prompts(), LENS)
            n = B * 2 * heads * smax * DH
            assert s.step_bytes(S) > 0
            caches[kind] = [read_cache(s, li, n * np.dtype(dtype).itemsize, dtype).reshape(B, 2, heads, smax, DH) for li in range(LAYERS)]
            if kind == 'gqa':
                bytes_gqa = s.step_bytes(S)
            else:
                assert bytes_gqa < s.step_bytes(S)  # Hkv cache rows and a smaller QKV weight
        finally:
            s.close()
    for li in range(LAYERS):
        want = G.fold_cache(caches['mha'][li], HKV)  # (checks that the replicated engine's copies are identical)
        got = caches['gqa'][li]
        assert got.any()
        np.testing.assert_array_equal(got[:, 1], want[:, 1])  # V: no RoPE precedes the store
        if dtype == np.float16:
            np.testing.assert_allclose(got[:, 0].astype(np.float32), want[:, 0].astype(np.float32), atol=2e-4, rtol=2e-3)
        else:
            d = np.abs(got[:, 0].astype(np.int32) - want[:, 0].astype(np.int32))
            assert d.max() <= 1 and np.mean(d == 0) > 0.98


def generate(eng, use_graph, beam=1):
    s = NativeSession(engine=eng)
    try:
        s.setup(B, S, NEW, beam) if beam > 1 else s.setup(B, S, NEW)
        s.context(prompts(), LENS)
        s.step(STEPS, use_graph=use_graph)
        assert s.decode_form() & 1 == 0
        return (s.beam_output() if beam > 1 else s.output_ids()), s.logits()
    finally:
        s.close()


def test_graph_replay_equals_eager_and_paged_equals_linear():
    eager, l0 = generate(engine('gqa', 'fp16'), False)
    graph, l1 = generate(engine('gqa', 'fp16'), True)
    np.testing.assert_array_equal(eager, graph)
    np.testing.assert_array_equal(l0, l1)
    np.testing.assert_array_equal(eager[:, :S], prompts())
    paged, l2 = generate(engine('gqa', 'fp16', ['--paged_kv_cache']), True)
    np.testing.assert_array_equal(paged, eager)
    packed, _ = generate(engine('gqa', 'fp16', ['--remove_input_padding']), True)
    np.testing.assert_array_equal(packed, eager)


def test_beam_width_2_runs_and_returns_sorted_scores():
    (ids, cum), _ = generate(engine('gqa', 'fp16', ['--max_beam_width', '2']), False, beam=2)
    assert ids.shape == (B, 2, S + NEW) and np.isfinite(cum).all()
    assert (cum[:, 0] >= cum[:, 1]).all()
    np.testing.assert_array_equal(ids[:, 0, :S], prompts())


# the session-against-oracle logits tolerance of the project (smoke(), tests/test_gpu_session.py: 2e-2), twice: a log-probability is
# x[t] - lse(x), and each of the two terms moves by at most the largest logit error - the derivation of tests/test_gpu_score.py's
# TINY_BOUND for the fp16 tiny model.  (Measured here: the fp16 engine's logits are 1.4e-3 from this oracle.)
SCORE_BOUND = 2 * 2e-2


@pytest.mark.parametrize('extra', [[], ['--remove_input_padding'], ['--paged_kv_cache']], ids=['padded', 'packed', 'paged'])
def test_score_agrees_with_scoring_ref_on_the_oracles_position_logits(extra):
    """score(): log-prob and top-1 of every prompt token, against tensorrt_llm/runtime/scoring_ref.py on the ORACLE's logits of every
    position (the unchanged llama_logits_context on the tiled prefixes of each prompt, expanded weights) - the construction and the
    checks (values, the 0 / -1 places, top-1 within the bound of the oracle's maximum) of tests/test_gpu_score.py."""
    from test_gpu_score import check_scores, position_logits
    w = oracle_weights()

    def context_logits(ids, lens):
        T, n = ids.shape
        caches = [np.zeros((T, 2, H, n + 1, DH), np.float16) for _ in range(LAYERS)]
        return O.llama_logits_context(ids, w, caches, lens, H)

    key = 'position_logits'
    if key not in _state:
        _state[key] = position_logits(context_logits, prompts(), LENS, V)
    s = NativeSession(engine=engine('gqa', 'fp16', extra))
    try:
        s.setup(B, S, NEW)
        lp, top = s.score(prompts(), LENS)
        check_scores(lp, top, _state[key], prompts(), LENS, SCORE_BOUND, tag=f'gqa fp16 {extra}')
        lp2, top2 = s.score(prompts(), LENS)  # a second call on the same session: the same bits
        assert np.array_equal(lp.view(np.uint32), lp2.view(np.uint32)) and np.array_equal(top, top2)
        s.step(1)  # generation continues from it
        assert np.isfinite(s.logits()).all()
    finally:
        s.close()


def test_generation_session_from_run_py_decodes_the_native_sessions_tokens():
    """examples/llama_quant/run.py::load_session on the grouped engine directory: ModelConfig carries the K/V head count of
    config.json, GenerationSession.decode returns the tokens the native session generates."""
    import run as Rn
    from tensorrt_llm.runtime import SamplingConfig
    eng = engine('gqa', 'fp16')
    sess, rank = Rn.load_session(_state[('dir', 'gqa', 'fp16', ())])
    assert rank == 0 and sess._model_config.num_heads == H and sess._model_config.num_kv_heads == HKV and sess.num_kv_heads == HKV
    sess.setup(B, S, NEW)
    got = sess.decode(prompts(), LENS, SamplingConfig(end_id=1, pad_id=2))
    s = NativeSession(engine=eng)
    try:
        s.setup(B, S, NEW)
        want = s.generate(prompts(), LENS, NEW, end_id=1, pad_id=2)
    finally:
        s.close()
    assert got.shape == (B, 1, S + NEW)
    np.testing.assert_array_equal(got[:, 0], want)
    np.testing.assert_array_equal(got[:, 0, :LENS[1]], prompts()[:, :LENS[1]])
