"""The fp8 (OCP E4M3) KV cache through the C++ host loop (quant_mode bit 64): the prefill never reads the cache, so an fp8-KV
session must reproduce the fp16-KV session's context logits bit for bit and hold exactly kv_store_fp8 of its cache; the
generation step runs the separate launches (bit 0 of the decode form clear), eager and from the step graph alike; beam search,
the paged pool, scoring and the front-end's GenerationSession go through the same launches."""
import ctypes
import os
import sys
import tempfile

import numpy as np
import pytest

from tensorrt_llm.runtime import kv_fp8_ref as R
from tensorrt_llm.runtime.native import NativeSession
from test_gpu_session import TINY_CFG, load_tiny, synth_model

pytestmark = pytest.mark.gpu

FP8_KV = 64
SCALES = [(1.0, 1.0), (np.float32(1.0) / np.float32(0.37), np.float32(0.37))]  # per layer (kv_orig_quant, kv_quant_orig)


def models():
    t, w = load_tiny()  # hidden 64, 2 heads of 32
    yield 'tiny_dh32', dict(TINY_CFG), w, t['ids'], t['input_lengths']
    cfg, w = synth_model(31, L=2, H=2, D=256, I=512, V=512)  # 2 heads of 128
    r = np.random.default_rng(4)
    ids = r.integers(3, cfg['vocab_size'], (2, 19)).astype(np.int32)
    lens = np.array([19, 11], np.int32)
    ids[1, 11:] = 2
    yield 'synth_dh128', dict(cfg), w, ids, lens


MODELS = {name: rest for name, *rest in models()}


def session(cfg, w, fp8, **extra):
    s = NativeSession(dict(cfg, quant_mode=FP8_KV if fp8 else 0, **extra))
    for k, v in w.items():
        s.set_tensor(k, v)
    if fp8:
        for i in range(cfg['num_layers']):
            oq, qo = SCALES[i % len(SCALES)]
            s.set_tensor(f'layers.{i}.attention.kv_orig_quant_scale', np.array([oq], np.float32))
            s.set_tensor(f'layers.{i}.attention.kv_quant_orig_scale', np.array([qo], np.float32))
    s.finalize()
    return s


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


def cache_elems(cfg, B, smax, paged_T=0):
    H, Dh = cfg['num_heads'], cfg['hidden_size'] // cfg['num_heads']
    if paged_T:
        return 2 * B * (-(-smax // paged_T)) * H * paged_T * Dh
    return B * 2 * H * smax * Dh


@pytest.mark.parametrize('paged', [0, 16], ids=['linear', 'paged16'])
@pytest.mark.parametrize('name', sorted(MODELS))
def test_context_logits_equal_the_fp16_cache_session_and_the_cache_holds_the_rule(name, paged):
    cfg, w, ids, lens = MODELS[name]
    B, S = ids.shape
    NEW = 9
    extra = dict(paged_kv_cache=1, tokens_per_block=paged) if paged else {}
    n = cache_elems(cfg, B, S + NEW, paged)
    s16, s8 = session(cfg, w, False, **extra), session(cfg, w, True, **extra)
    try:
        for s in (s16, s8):
            s.setup(B, S, NEW)
            s.context(ids, lens)
        np.testing.assert_array_equal(s8.logits(), s16.logits())  # bit-identical: the prefill never reads the cache
        assert s8.decode_form() & 1 == 0
        assert s8.step_bytes(S) < s16.step_bytes(S)
        for li in range(cfg['num_layers']):
            c16 = read_cache(s16, li, n * 2, np.float16)
            c8 = read_cache(s8, li, n, np.uint8)
            assert c16.any()
            np.testing.assert_array_equal(c8, R.kv_store_fp8(c16, SCALES[li % len(SCALES)][0]), err_msg=f'layer {li}')
    finally:
        s16.close()
        s8.close()


@pytest.mark.parametrize('name', sorted(MODELS))
def test_generation_graph_equals_eager_and_stays_near_the_fp16_cache(name):
    cfg, w, ids, lens = MODELS[name]
    B, S = ids.shape
    NEW = 9
    outs, logits = [], []
    for use_graph in (False, True):
        s = session(cfg, w, True)
        s.setup(B, S, NEW)
        s.context(ids, lens)
        s.step(8, use_graph=use_graph)
        assert s.decode_form() & 1 == 0
        outs.append(s.output_ids())
        logits.append(s.logits())
        s.close()
    np.testing.assert_array_equal(outs[0], outs[1])
    np.testing.assert_array_equal(logits[0], logits[1])
    np.testing.assert_array_equal(outs[0][:, :S], ids)
    assert np.isfinite(logits[0]).all()
    # teacher-forced on the fp8 session's tokens, the fp16-cache session's logits differ by the cache's rounding only: E4M3 keeps
    # 3 mantissa bits (relative step 2^-3, rms error ~ 2.7 % of a value), which moves a logit by a few per cent of the logit range
    s = session(cfg, w, False)
    s.setup(B, S, NEW)
    s.context(ids, lens)
    for step in range(8):
        s.force_tokens(outs[0][:, S + step])
        s.step(1, use_graph=False)
    ref = s.logits()
    s.close()
    scale = max(np.abs(ref).max(), 1.0)
    print(f'[{name}] fp8 vs fp16 cache after 8 steps: max |d logit| / range = {np.abs(logits[0] - ref).max() / scale:.4f}')
    assert np.abs(logits[0] - ref).max() < 0.25 * scale


def test_fake_context_fills_finite_codes_only():
    cfg, w, ids, lens = MODELS['tiny_dh32']
    B, S, NEW = 2, 16, 4
    s = session(cfg, w, True)
    s.setup(B, S, NEW)
    s.fake_context(12, seed=5)
    n = cache_elems(cfg, B, S + NEW)
    for li in range(cfg['num_layers']):
        c = read_cache(s, li, n, np.uint8)
        assert not np.any((c & 0x7f) == 0x7f), 'a NaN code in the fake context'
        assert len(np.unique(c)) > 64  # random, both signs
    s.step(2, use_graph=False)
    assert np.isfinite(s.logits()).all()
    s.close()


def test_score_leaves_the_session_as_context_does():
    cfg, w, ids, lens = MODELS['tiny_dh32']
    B, S = ids.shape
    NEW = 4
    n = cache_elems(cfg, B, S + NEW)
    a, b = session(cfg, w, True), session(cfg, w, True)
    ref = session(cfg, w, False)
    try:
        for s in (a, b, ref):
            s.setup(B, S, NEW)
        a.context(ids, lens)
        lp, top1 = b.score(ids, lens)
        lp16, top16 = ref.score(ids, lens)
        np.testing.assert_array_equal(lp, lp16)  # prompt scores never read the cache
        np.testing.assert_array_equal(top1, top16)
        np.testing.assert_array_equal(a.logits(), b.logits())
        for li in range(cfg['num_layers']):
            np.testing.assert_array_equal(read_cache(a, li, n, np.uint8), read_cache(b, li, n, np.uint8))
        a.step(3, use_graph=False)
        b.step(3, use_graph=False)
        np.testing.assert_array_equal(a.output_ids(), b.output_ids())
    finally:
        for s in (a, b, ref):
            s.close()


def test_beam_search_runs_on_the_fp8_cache():
    cfg, w, ids, lens = MODELS['synth_dh128']
    B, S = ids.shape
    NEW, W = 6, 2
    s = session(cfg, w, True)
    s.setup(B, S, NEW, beam_width=W)
    s.context(ids, lens)
    s.step(NEW - 1, use_graph=False)
    out, cum = s.beam_output()
    s.close()
    assert out.shape == (B, W, S + NEW) and cum.shape == (B, W)
    for b in range(B):
        for k in range(W):
            np.testing.assert_array_equal(out[b, k, :lens[b]], ids[b, :lens[b]])
        assert cum[b, 0] >= cum[b, 1] and np.isfinite(cum[b]).all()
    assert (out[:, :, S:] >= 0).all() and (out[:, :, S:] < cfg['vocab_size']).all()


def test_generation_session_end_to_end_through_the_build_script():
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'trtllm-llama_amd', 'examples', 'llama_quant')
    if ex not in sys.path:
        sys.path.insert(0, ex)
    import build as B
    from tensorrt_llm import Mapping
    from tensorrt_llm.runtime import GenerationSession, ModelConfig, SamplingConfig
    from test_engine_check import TINY
    d = tempfile.mkdtemp()
    B.run_build(TINY + ['--output_dir', d, '--fp8_kv_cache', '--random_seed', '3'])
    blob = open(os.path.join(d, 'llama_float16_tp1_rank0.engine'), 'rb').read()
    assert b'quant_mode=64' in blob[:4096]
    sess = GenerationSession(ModelConfig(vocab_size=128, num_layers=2, num_heads=2, hidden_size=64), blob, Mapping(1, 0))
    ids = np.random.default_rng(1).integers(3, 128, (2, 10)).astype(np.int32)
    lens = np.array([10, 6], np.int32)
    sess.setup(2, 10, 8)
    out = sess.decode(ids, lens, SamplingConfig(end_id=-1, pad_id=2))
    assert out.shape == (2, 1, 18)
    for b in range(2):
        np.testing.assert_array_equal(out[b, 0, :lens[b]], ids[b, :lens[b]])
    assert sess.runtime.decode_form() & 1 == 0
    assert np.isfinite(sess.runtime.logits()).all()
    np.testing.assert_array_equal(out, sess.decode(ids, lens, SamplingConfig(end_id=-1, pad_id=2)))
