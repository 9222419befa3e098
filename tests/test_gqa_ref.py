"""tensorrt_llm/runtime/gqa_ref.py - grouped-query attention restated through the multi-head oracle on expanded inputs - against
a direct float64 grouped attention written here (einsum over [Hkv, G] query heads, no expansion).  Host-only.

Tolerance, from the oracle's rounding points (oracle/llama_oracle.py mmha_decode / context_attention): RoPE'd q and k are fp16
in both (the same apply_rope), the scores, the softmax and the sum over time are fp32 in the oracle (relative 2^-24 per
operation: noise), the normalised probabilities are rounded to fp16 before P.V (relative 2^-11 each) and the result is rounded
to fp16 once (relative 2^-11).  So per output element d

    |oracle - float64|  <=  2^-11 * (sum_t p_t |v_td|  +  |out_d|)  +  1e-6 * |out_d| (the normaliser's + 1e-6)  +  fp32 noise,

which the tests evaluate per element with the float64 p and out; 2e-6 covers the fp32 noise of sums of <= 64 terms of size ~1."""
import numpy as np
import pytest

from oracle import llama_oracle as O
from tensorrt_llm.runtime import gqa_ref as R

SHAPES = [(4, 2), (8, 1), (6, 2)]
DH = 32


def rng(seed):
    return np.random.default_rng(seed)


def bound(p64, v64, out64):
    return 2.0 ** -11 * (p64 @ np.abs(v64) + np.abs(out64)) * 1.001 + 1e-6 * np.abs(out64) + 2e-6


def test_the_module_needs_no_torch():
    import subprocess
    import sys
    code = ('import sys; sys.path[:0] = %r; import tensorrt_llm.runtime.gqa_ref as R; import numpy as np; '
            'assert "torch" not in sys.modules; assert R.expand_qkv(np.zeros((1, 16)), 2, 1, 4).shape == (1, 24)' % (sys.path, ))
    subprocess.run([sys.executable, '-c', code], check=True)


@pytest.mark.parametrize('H,Hkv', SHAPES + [(4, 4), (16, 1)])
@pytest.mark.parametrize('dtype', [np.float16, np.int8, np.uint8])
def test_expand_fold_round_trip(H, Hkv, dtype):
    r = rng(H * 10 + Hkv)
    G = H // Hkv
    cache = r.integers(-100, 100, (2, 2, Hkv, 5, DH)).astype(dtype)
    big = R.expand_cache(cache, H)
    assert big.shape == (2, 2, H, 5, DH) and big.dtype == cache.dtype
    for h in range(H):
        np.testing.assert_array_equal(big[:, :, h], cache[:, :, h // G])
    np.testing.assert_array_equal(R.fold_cache(big, Hkv), cache)
    if G > 1:
        big[0, 1, 1, 2, 3] += 1  # a copy that differs from its K/V head
        with pytest.raises(ValueError):
            R.fold_cache(big, Hkv)
        R.fold_cache(big, Hkv, check=False)
    qkv = r.standard_normal((3, 2, (H + 2 * Hkv) * DH)).astype(np.float32)
    e = R.expand_qkv(qkv, H, Hkv, DH)
    assert e.shape == (3, 2, 3 * H * DH)
    e5 = e.reshape(3, 2, 3, H, DH)
    kv = qkv[..., H * DH:].reshape(3, 2, 2, Hkv, DH)
    np.testing.assert_array_equal(e5[:, :, 0].reshape(3, 2, -1), qkv[..., :H * DH])
    for h in range(H):
        np.testing.assert_array_equal(e5[:, :, 1, h], kv[:, :, 0, h // G])
        np.testing.assert_array_equal(e5[:, :, 2, h], kv[:, :, 1, h // G])
    np.testing.assert_array_equal(R.fold_qkv(e, H, Hkv, DH), qkv)
    # the weight: rows are output channels in the same block order; y = x W^T commutes with the expansion
    w = r.standard_normal(((H + 2 * Hkv) * DH, 24)).astype(np.float32)
    x = r.standard_normal((4, 24)).astype(np.float32)
    we = R.expand_qkv_weight(w, H, Hkv, DH)
    assert we.shape == (3 * H * DH, 24)
    np.testing.assert_array_equal(x @ we.T, R.expand_qkv(x @ w.T, H, Hkv, DH))
    np.testing.assert_array_equal(R.expand_qkv_weight(w[:, 0], H, Hkv, DH), we[:, 0])  # per-channel vectors


@pytest.mark.parametrize('bad', [(4, 3), (4, 0), (2, 4)])
def test_a_head_count_that_does_not_divide_is_refused(bad):
    with pytest.raises(ValueError):
        R.expand_qkv(np.zeros((1, (bad[0] + 2 * bad[1]) * 4)), bad[0], bad[1], 4)


@pytest.mark.parametrize('H,Hkv', SHAPES)
def test_decode_against_a_direct_float64_grouped_attention(H, Hkv):
    r = rng(1000 + H * 10 + Hkv)
    G, B, smax, L = H // Hkv, 2, 40, 29
    max_in = L - 3
    in_len = [max_in, max_in // 2]
    masked = np.zeros((B, smax), np.int32)
    masked[1, in_len[1]:max_in] = 1
    cache0 = np.zeros((B, 2, Hkv, smax, DH), np.float16)
    cache0[:, :, :, :L] = r.standard_normal((B, 2, Hkv, L, DH)).astype(np.float16)
    qkv = O.f16(r.standard_normal((B, (H + 2 * Hkv) * DH)))
    cache = cache0.copy()
    out = R.decode(qkv, cache, [L, L], in_len, max_in, L, H, Hkv, DH, DH, True, 1.0, masked)
    assert out.shape == (B, H * DH)
    keep = np.ones(smax, bool)
    keep[L] = False
    np.testing.assert_array_equal(cache[:, :, :, keep], cache0[:, :, :, keep])
    for b in range(B):
        pos = L - (max_in - in_len[b])
        q = O.apply_rope(qkv[b, :H * DH].reshape(Hkv, G, DH), pos, DH, True).astype(np.float64)
        k_new = O.apply_rope(qkv[b, H * DH:(H + Hkv) * DH].reshape(Hkv, DH), pos, DH, True)
        v_new = qkv[b, (H + Hkv) * DH:].reshape(Hkv, DH)
        # the append: once per K/V head, the fp16 rows themselves
        np.testing.assert_array_equal(cache[b, 0, :, L].astype(np.float32), k_new)
        np.testing.assert_array_equal(cache[b, 1, :, L].astype(np.float32), v_new)
        keys = cache[b, 0, :, :L + 1].astype(np.float64)  # [Hkv, T, Dh], slot L included
        vals = cache[b, 1, :, :L + 1].astype(np.float64)
        s = np.einsum('jgd,jtd->jgt', q, keys) / np.sqrt(DH)
        valid = np.ones(L + 1, bool)
        valid[:L] = masked[b, :L] == 0
        s = np.where(valid, s, -np.inf)
        p = np.exp(s - s.max(axis=-1, keepdims=True))
        p /= p.sum(axis=-1, keepdims=True)
        ref = np.einsum('jgt,jtd->jgd', p, vals)
        tol = np.stack([bound(p[j], vals[j], ref[j]) for j in range(Hkv)])
        err = np.abs(out[b].reshape(Hkv, G, DH) - ref)
        assert (err <= tol).all(), (err / tol).max()


@pytest.mark.parametrize('H,Hkv', SHAPES)
def test_context_against_a_direct_float64_grouped_attention(H, Hkv):
    r = rng(2000 + H * 10 + Hkv)
    G, B, S, smax = H // Hkv, 2, 21, 24
    in_len = [S, S // 2]
    qkv = O.f16(r.standard_normal((B, S, (H + 2 * Hkv) * DH)))
    cache = np.zeros((B, 2, Hkv, smax, DH), np.float16)
    out, roped = R.context(qkv, cache, in_len, H, Hkv, DH, DH)
    assert out.shape == (B, S, H * DH) and roped.shape == qkv.shape
    for b in range(B):
        n = in_len[b]
        q = np.stack([O.apply_rope(qkv[b, s, :H * DH].reshape(Hkv, G, DH), s, DH, True) for s in range(n)])  # [n, Hkv, G, Dh]
        k = np.stack([O.apply_rope(qkv[b, s, H * DH:(H + Hkv) * DH].reshape(Hkv, DH), s, DH, True) for s in range(n)])
        v = qkv[b, :n, (H + Hkv) * DH:].reshape(n, Hkv, DH)
        np.testing.assert_array_equal(roped[b, :n, :H * DH], q.reshape(n, -1))
        np.testing.assert_array_equal(roped[b, :n, H * DH:(H + Hkv) * DH], k.reshape(n, -1))
        np.testing.assert_array_equal(roped[b, n:], 0)
        np.testing.assert_array_equal(cache[b, 0, :, :n].astype(np.float32), k.transpose(1, 0, 2))
        np.testing.assert_array_equal(cache[b, 1, :, :n].astype(np.float32), v.transpose(1, 0, 2))
        np.testing.assert_array_equal(cache[b, :, :, n:], 0)  # padding rows are stored as zero
        s = np.einsum('sjgd,tjd->jgst', q.astype(np.float64), k.astype(np.float64)) / np.sqrt(DH)
        s = np.where(np.tril(np.ones((n, n), bool)), s, -np.inf)
        p = np.exp(s - s.max(axis=-1, keepdims=True))
        p /= p.sum(axis=-1, keepdims=True)
        ref = np.einsum('jgst,tjd->sjgd', p, v.astype(np.float64))
        got = out[b, :n].reshape(n, Hkv, G, DH)
        for j in range(Hkv):
            for g in range(G):
                tol = bound(p[j, g], v[:, j].astype(np.float64), ref[:, j, g])
                err = np.abs(got[:, j, g] - ref[:, j, g])
                assert (err <= tol).all(), (j, g, (err / tol).max())
        np.testing.assert_array_equal(out[b, n:], 0)


@pytest.mark.parametrize('kind', ['int8', 'fp8'])
def test_quantised_caches_store_once_per_kv_head(kind):
    """int8 / E4M3 caches: the folded cache holds the oracle's own store of every K/V row, and with Hkv == H the module is the
    oracle itself."""
    from tensorrt_llm.runtime import kv_fp8_ref as F8
    r = rng(7)
    H, Hkv, B, smax, L = 4, 2, 1, 12, 8
    scale = 20.0
    store = (lambda x: O.kv_store(x, scale)) if kind == 'int8' else (lambda x: F8.kv_store_fp8(x, scale))
    dt = np.int8 if kind == 'int8' else np.uint8
    cache = np.zeros((B, 2, Hkv, smax, DH), dt)
    cache[:, :, :, :L] = store(r.standard_normal((B, 2, Hkv, L, DH)) * 0.5)
    qkv = O.f16(r.standard_normal((B, (H + 2 * Hkv) * DH)))
    R.decode(qkv, cache, [L], [L], L, L, H, Hkv, DH, DH, True, 1.0, None, scale, 1.0 / scale)
    k_new = O.apply_rope(qkv[0, H * DH:(H + Hkv) * DH].reshape(Hkv, DH), L, DH, True)
    np.testing.assert_array_equal(cache[0, 0, :, L], store(k_new))
    np.testing.assert_array_equal(cache[0, 1, :, L], store(qkv[0, (H + Hkv) * DH:].reshape(Hkv, DH)))
    # Hkv == H: identical to the oracle, cache and output
    q3 = O.f16(r.standard_normal((B, 3 * H * DH)))
    c1 = np.zeros((B, 2, H, smax, DH), dt)
    c1[:, :, :, :L] = store(r.standard_normal((B, 2, H, L, DH)) * 0.5)
    c2 = c1.copy()
    a = R.decode(q3, c1, [L], [L], L, L, H, H, DH, DH, True, 1.0, None, scale, 1.0 / scale)
    if kind == 'int8':
        b = O.mmha_decode(q3, c2, [L], [L], L, L, H, DH, DH, True, 1.0, None, scale, 1.0 / scale)
    else:
        b = F8.mmha_decode_fp8(q3, c2, [L], [L], L, L, H, DH, DH, scale, 1.0 / scale)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(c1, c2)


def test_hf_gqa_model_through_the_weight_loader_and_the_expanded_oracle():
    """A random HF LlamaForCausalLM with num_key_value_heads = 2 (4 heads, hidden 64, 2 layers): its weights go through
    examples/llama_quant/weight.py::load_from_hf_llama into the grouped model definition, expand_qkv_weight turns the fused
    QKV weight into the multi-head one, and the oracle's llama_logits_context agrees with HF's fp32 logits within what
    tests/test_oracle_golden.py holds the multi-head fixture to (atol 1e-1 of the reference's model test, and 3e-2)."""
    import os
    import sys
    import torch
    from transformers import LlamaConfig, LlamaForCausalLM
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'trtllm-llama_amd', 'examples', 'llama_quant')
    if ex not in sys.path:
        sys.path.insert(0, ex)
    from weight import load_from_hf_llama
    from tensorrt_llm.models import LLaMAForCausalLM
    H, Hkv, D, V = 4, 2, 64, 96
    torch.manual_seed(0)
    hf = LlamaForCausalLM(LlamaConfig(hidden_size=D, num_attention_heads=H, num_key_value_heads=Hkv, intermediate_size=128,
                                      vocab_size=V, num_hidden_layers=2, max_position_embeddings=64, rms_norm_eps=1e-6,
                                      attention_bias=False, tie_word_embeddings=False)).float().eval()
    with torch.no_grad():
        for p in hf.parameters():
            if p.ndim == 2:
                p.mul_(2.0)  # wider logits than the 0.02-std init
    m = LLaMAForCausalLM(num_layers=2, num_heads=H, hidden_size=D, vocab_size=V, hidden_act='silu', max_position_embeddings=64,
                         dtype='float16', mlp_hidden_size=128, num_kv_heads=Hkv)
    load_from_hf_llama(m, hf, 0, 1, 'float16')
    params = {k: np.asarray(p.raw_value).astype(np.float32) for k, p in m.named_parameters()}
    assert params['layers.0.attention.qkv.weight'].shape == ((H + 2 * Hkv) * (D // H), D)
    w = {k: params[k] for k in ('vocab_embedding.weight', 'ln_f.weight', 'lm_head.weight')}
    w['layers'] = []
    for i in range(2):
        lw = {k[len(f'layers.{i}.'):]: v for k, v in params.items() if k.startswith(f'layers.{i}.')}
        lw['attention.qkv.weight'] = R.expand_qkv_weight(lw['attention.qkv.weight'], H, Hkv, D // H)
        w['layers'].append(lw)
    r = rng(5)
    B, S = 2, 12
    lens = [S, 7]
    ids = r.integers(3, V, (B, S))
    with torch.no_grad():
        ref = np.stack([hf(torch.from_numpy(ids[b:b + 1, :lens[b]])).logits[0, -1].numpy() for b in range(B)])
    caches = [np.zeros((B, 2, H, 16, D // H), np.float16) for _ in range(2)]
    logits = O.llama_logits_context(ids, w, caches, lens, H)
    err = np.abs(logits - ref).max()
    print(f'oracle on expanded GQA weights vs HF fp32: max |logit diff| = {err:.3e}')
    np.testing.assert_allclose(logits, ref, atol=1e-1)
    assert err < 3e-2
    np.testing.assert_array_equal(logits.argmax(-1), ref.argmax(-1))
    # the oracle's caches hold every K/V head G times: they fold
    for c in caches:
        assert R.fold_cache(c, Hkv).shape == (B, 2, Hkv, 16, D // H)
