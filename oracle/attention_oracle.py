"""The context (prompt) attention (csrc/kernels/context_attn.hip) in numpy float64 - TEST INFRASTRUCTURE ONLY (see llama_oracle.py
header).

    out[b, q, h, :] = sum_{j <= q} p_j v[b, j, kv(h), :],   p = softmax_j(score_scale * q[b, q, h, :] . k[b, j, kv(h), :])

for q < len[b]; rows q >= len[b] are zero.  The inputs are the fp16 values of the rows AFTER RoPE - what the launch leaves in the
fused QKV buffer - carried as float64, so the oracle contains no rounding of its own: every product and sum is float64, the softmax
is exact.  The kernels' rounding points enter through tolerance() below, not through the oracle.

tolerance(): both attention kernels (one wave per query; MFMA flash-style) keep scores, the running maximum, the normaliser and the
accumulation in fp32, round every probability to fp16 ONCE before it multiplies v (relative 2^-11; absolute 2^-25 below the fp16
normal range) and round the result to fp16 ONCE (relative 2^-11 of |out|).  With absmass = sum_j p_j |v_j|:

    |got - out| <= 2^-11 * absmass          the probabilities' rounding, weighted by |v_j|
                 + 2^-11 * |out|            the result's rounding
                 + 2^-25 * S * vmax         probabilities in the subnormal range, S of them at most, each times |v| <= vmax
                 + fp32 terms               (scores, exp, the sums: relative ~1e-6 each, far below 2^-11)

tolerance = 2 * 2^-11 * (absmass + |out|) + 2^-24 * S * vmax: the factor 2 is the margin for the fp32 terms and the exp
approximations (tests/test_attention_oracle.py holds two fp32 restatements with the kernels' rounding points inside it).

witness(): 0/1 value matrices that turn the attention into a key counter - with q = 0 every probability is exactly 1 / (q + 1), so
out[q, d] = (number of keys j <= q with V[j, d] = 1) / (q + 1), and one dropped or doubled key moves an element by 1 / (q + 1)."""
import numpy as np

F64 = np.float64


def causal_attention_f64(q16, k16, v16, lens, num_heads, num_kv_heads, head_size, score_scale):
    """q16 [B, S, H*Dh], k16 / v16 [B, S, Hkv*Dh]: fp16 values (any float dtype), rows beyond lens[b] ignored.
    Returns (out, absmass), float64 [B, S, H*Dh]: sum_j p_j v_j and sum_j p_j |v_j|; rows >= lens[b] are zero."""
    H, Hkv, Dh = int(num_heads), int(num_kv_heads), int(head_size)
    if not (1 <= Hkv <= H and H % Hkv == 0):
        raise ValueError(f'num_kv_heads {Hkv} must divide num_heads {H}')
    G = H // Hkv
    q = np.asarray(q16, dtype=F64)
    B, S = q.shape[:2]
    q = q.reshape(B, S, H, Dh)
    k = np.asarray(k16, dtype=F64).reshape(B, S, Hkv, Dh)
    v = np.asarray(v16, dtype=F64).reshape(B, S, Hkv, Dh)
    out = np.zeros((B, S, H, Dh), F64)
    absmass = np.zeros((B, S, H, Dh), F64)
    for b in range(B):
        n = int(lens[b])
        if n <= 0:
            continue
        future = ~np.tril(np.ones((n, n), dtype=bool))
        for h in range(H):
            kk, vv = k[b, :n, h // G], v[b, :n, h // G]
            s = (q[b, :n, h] @ kk.T) * F64(score_scale)
            s[future] = -np.inf
            e = np.exp(s - s.max(axis=1, keepdims=True))
            p = e / e.sum(axis=1, keepdims=True)
            out[b, :n, h] = p @ vv
            absmass[b, :n, h] = p @ np.abs(vv)
    return out.reshape(B, S, H * Dh), absmass.reshape(B, S, H * Dh)


def tolerance(out, absmass, S, vmax):
    """per element: 2 * 2^-11 * (absmass + |out|) + 2^-24 * S * vmax (the derivation is in the module docstring)"""
    return 2.0 * 2.0 ** -11 * (np.asarray(absmass, dtype=F64) + np.abs(np.asarray(out, dtype=F64))) + 2.0 ** -24 * S * F64(vmax)


WITNESS_KINDS = ('key', 'block')


def witness(kind, S, head_size):
    """(V [S, Dh] of zeros and ones, expected [S, Dh] float64) for q = 0 (every probability 1 / (q + 1)):
    'key':   V[j, d] = (j % Dh == d)          - counts the keys of every residue: a key dropped, doubled or swapped for another
                                                within Dh neighbours shows;
    'block': V[j, d] = ((j // 64) % Dh == d)  - counts the keys of every 64-key block: a whole block (a stale or repeated operand
                                                stage) or part of one shows, even where 'key' sees the right residues.
    expected[q, d] = count_d(q) / (q + 1), with count_d(q) the ones among V[0 .. q, d]."""
    if kind not in WITNESS_KINDS:
        raise ValueError(kind)
    Dh = int(head_size)
    j = np.arange(S)
    code = j % Dh if kind == 'key' else (j // 64) % Dh
    V = (code[:, None] == np.arange(Dh)[None, :]).astype(F64)
    return V, np.cumsum(V, axis=0) / (j[:, None] + 1.0)
