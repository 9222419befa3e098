"""No GPU: oracle/attention_oracle.py against the project's fp32 restatements of the context attention, and its witness matrices
against hand-counted values.

The bound tolerance() is meant for the HIP kernels (tests/test_gpu_ctx_attn_instances.py).  It is sound only if a computation with
the kernels' rounding points - fp32 scores and sums, probabilities rounded to fp16 once, the result rounded to fp16 once - meets it
on its own: llama_oracle.context_attention (and gqa_ref.context, the same on expanded K/V heads) is such a computation, and so is
the un-normalised-p variant below (the kernels round exp(s - m) and divide by the fp32 sum at the end)."""
import numpy as np
import pytest

from oracle import attention_oracle as A
from oracle import llama_oracle as O
from tensorrt_llm.runtime import gqa_ref as G

F32 = np.float32


def f16(x):
    return np.asarray(x, dtype=F32).astype(np.float16).astype(F32)


def split(roped, H, Hkv, Dh):
    return roped[..., :H * Dh], roped[..., H * Dh:(H + Hkv) * Dh], roped[..., (H + Hkv) * Dh:]


def unnormalised_p(q, k, v, lens, H, Hkv, Dh, scale):
    """the kernels' order in fp32: p = fp16(exp(s - max)), l = sum of the unrounded exp, out = fp16((sum p v) / (l + 1e-6))"""
    B, S = q.shape[:2]
    q, k, v = (np.asarray(x, F32).reshape(B, S, -1, Dh) for x in (q, k, v))
    out = np.zeros((B, S, H, Dh), F32)
    for b in range(B):
        n = int(lens[b])
        for h in range(H):
            s = (q[b, :n, h] @ k[b, :n, h // (H // Hkv)].T).astype(F32) * F32(scale)
            s[~np.tril(np.ones((n, n), dtype=bool))] = -np.inf
            e = np.exp(s - s.max(axis=1, keepdims=True), dtype=F32)
            acc = (f16(e) @ v[b, :n, h // (H // Hkv)]).astype(F32)
            out[b, :n, h] = f16(acc / (e.sum(axis=1, keepdims=True, dtype=F32) + F32(1e-6)))
    return out.reshape(B, S, H * Dh)


@pytest.mark.parametrize('H,Hkv,Dh,S,amp', [(2, 2, 32, 33, 1.0), (4, 2, 64, 130, 1.0), (4, 1, 128, 257, 2.0), (2, 1, 256, 65, 2.0),
                                           (1, 1, 64, 600, 1.0)])
def test_the_fp32_restatements_meet_the_bound(H, Hkv, Dh, S, amp):
    r = np.random.default_rng(S + Dh)
    lens = [S, S // 2, 1]
    qkv = f16(amp * r.standard_normal((3, S, (H + 2 * Hkv) * Dh)))
    cache = np.zeros((3, 2, Hkv, S, Dh), np.float16)
    ref, roped = G.context(qkv, cache, lens, H, Hkv, Dh, Dh)
    q, k, v = split(roped, H, Hkv, Dh)
    scale = 1.0 / np.sqrt(Dh)
    out, absmass = A.causal_attention_f64(q, k, v, lens, H, Hkv, Dh, scale)
    tol = A.tolerance(out, absmass, S, np.abs(v).max())
    for b, n in enumerate(lens):
        assert not out[b, n:].any() and not absmass[b, n:].any() and not ref[b, n:].any()
    worst = {}
    for name, got in (('gqa_ref.context', ref), ('un-normalised p', unnormalised_p(q, k, v, lens, H, Hkv, Dh, scale))):
        worst[name] = float((np.abs(got - out) / tol).max())
    if Hkv == H:
        cache = np.zeros((3, 2, H, S, Dh), np.float16)
        got, roped2 = O.context_attention(qkv, cache, lens, H, Dh, Dh)
        assert np.array_equal(roped2, roped)
        worst['llama_oracle.context_attention'] = float((np.abs(got - out) / tol).max())
    print(f'H={H} Hkv={Hkv} Dh={Dh} S={S} amp={amp}: worst |restatement - oracle| / tolerance {worst}, median tolerance '
          f'{np.median(tol[0]):.2e}')
    assert max(worst.values()) <= 1.0, worst


def test_the_oracle_is_a_plain_softmax_on_a_hand_checked_case():
    """one head of size 2, three tokens, scale 1: q . k = 0 for the first two queries (q = 0) and log 2, log 4 apart for the third"""
    q = np.array([[[0, 0], [0, 0], [1, 0]]], float)
    k = np.array([[[5, 5], [7, -3], [0, 0]]], float)
    k[0, :, 0] = [0.0, np.log(2.0), np.log(4.0)]
    v = np.array([[[1, -1], [2, 2], [-4, 8]]], float)
    out, absmass = A.causal_attention_f64(q, k, v, [3], 1, 1, 2, 1.0)
    want = np.array([[1, -1], [1.5, 0.5], [(1 + 2 * 2 - 4 * 4) / 7, (-1 + 2 * 2 + 4 * 8) / 7]])
    mass = np.array([[1, 1], [1.5, 1.5], [(1 + 4 + 16) / 7, (1 + 4 + 32) / 7]])
    np.testing.assert_allclose(out[0], want, rtol=1e-14, atol=0)
    np.testing.assert_allclose(absmass[0], mass, rtol=1e-14, atol=0)
    out, _ = A.causal_attention_f64(q, k, v, [2], 1, 1, 2, 1.0)
    np.testing.assert_allclose(out[0], np.array([[1, -1], [1.5, 0.5], [0, 0]]), rtol=1e-14, atol=0)
    t = A.tolerance(np.array([-2.0]), np.array([3.0]), 100, 4.0)
    assert t[0] == 2 * 2.0 ** -11 * 5 + 2.0 ** -24 * 400


def test_the_witness_expectations_by_hand():
    V, want = A.witness('key', 6, 4)  # keys 0 .. 5 carry the codes 0 1 2 3 0 1
    assert V.tolist() == [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [1, 0, 0, 0], [0, 1, 0, 0]]
    assert want[0].tolist() == [1, 0, 0, 0] and want[3].tolist() == [0.25] * 4
    assert want[4].tolist() == [2 / 5, 1 / 5, 1 / 5, 1 / 5] and want[5].tolist() == [2 / 6, 2 / 6, 1 / 6, 1 / 6]
    V, want = A.witness('block', 130, 2)  # blocks 0, 1, 2 carry the codes 0 1 0
    assert V[:64].tolist() == [[1, 0]] * 64 and V[64:128].tolist() == [[0, 1]] * 64 and V[128:].tolist() == [[1, 0]] * 2
    assert want[63].tolist() == [1, 0] and want[64].tolist() == [64 / 65, 1 / 65] and want[127].tolist() == [0.5, 0.5]
    assert want[129].tolist() == [66 / 130, 64 / 130]
    with pytest.raises(ValueError):
        A.witness('other', 4, 4)


@pytest.mark.parametrize('kind', A.WITNESS_KINDS)
def test_the_oracle_counts_the_witness_keys(kind):
    """q = 0 makes the oracle itself the counter the witness describes - and one key moved changes an element by 1 / (q + 1)"""
    S, Dh = 200, 32
    V, want = A.witness(kind, S, Dh)
    r = np.random.default_rng(1)
    k = r.standard_normal((1, S, Dh))
    out, _ = A.causal_attention_f64(np.zeros((1, S, Dh)), k, V[None], [S], 1, 1, Dh, 0.25)
    np.testing.assert_allclose(out[0], want, rtol=0, atol=1e-13)
    V2 = V.copy()
    V2[100] = V2[99 if kind == 'key' else 63]  # key 100 counted under another code
    out2, _ = A.causal_attention_f64(np.zeros((1, S, Dh)), k, V2[None], [S], 1, 1, Dh, 0.25)
    moved = np.abs(out2[0] - want).max(axis=1)
    assert moved[:100].max() < 1e-13 and np.allclose(moved[100:], 1.0 / (np.arange(100, S) + 1.0), rtol=1e-9)
