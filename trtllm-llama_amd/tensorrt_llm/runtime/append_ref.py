"""The append attention (csrc/kernels/append_attn.hip) restated in numpy float64 - for tests.

n new tokens per sequence onto a live KV cache, the parallel form of n decode steps.  With p_b the cache slots of sequence b in use:

    placement   appended token i occupies cache slot p_b + i; its rotary position is p_b + i - (max_input_len - input_lengths[b]);
    visibility  its query sees every slot t < p_b with masked_tokens[b][t] == 0, plus the appended tokens 0 .. i;
    values      a past slot counts with the value the decode kernel reads: the fp16 element itself, or value(byte) * kv_quant_orig for
                the one-byte types (the exact product: no rounding between the byte and the score / the p.v sum); an appended
                token's own k and v count un-quantised, as the fp16 values the launch leaves in the QKV buffer (k after RoPE);
    store       cache slot p_b + i receives store_rows(k), store_rows(v): the store rule of the cache type.

append_ref returns (out, absmass) like oracle.attention_oracle.causal_attention_f64: the exact soft-max attention over the visible
keys in float64, and sum_j p_j |v_j| for attention_oracle.tolerance() (the kernels' rounding points - fp32 arithmetic, fp16
probabilities, one final fp16 rounding - enter through that bound, not through this restatement)."""
import numpy as np

from .kv_fp8_ref import _TABLE as _E4M3, kv_store_fp8

F32, F64 = np.float32, np.float64
KV_TYPES = ('fp16', 'int8', 'fp8')


def positions(past, n, max_input_len, input_lengths):
    """int [B, n]: the rotary position of appended token i of sequence b."""
    past = np.asarray(past, dtype=np.int64)
    lens = np.asarray(input_lengths, dtype=np.int64)
    return past[:, None] + np.arange(n)[None, :] - (int(max_input_len) - lens)[:, None]


def visible(past_b, i, masked_row=None):
    """(bool [past_b] over the cache slots, number of appended tokens seen) for appended token i of one sequence."""
    seen = np.ones(int(past_b), dtype=bool)
    if masked_row is not None:
        seen &= np.asarray(masked_row[:int(past_b)]) == 0
    return seen, i + 1


def store_rows(x16, kv_type, scale_orig_quant=None):
    """What a cache slot receives for the fp16 values x16: float16 as they are, int8 = sat(rni(float32(x) * float32(s))) (ties to
    even, NaN -> 0), or the E4M3 codes of kv_fp8_ref.kv_store_fp8 (uint8)."""
    if kv_type == 'fp16':
        return np.asarray(x16, dtype=F32).astype(np.float16)
    if kv_type == 'int8':
        p = (np.asarray(x16, dtype=F32) * F32(scale_orig_quant)).astype(F32)
        return np.clip(np.rint(np.nan_to_num(p, nan=0.0)), -128, 127).astype(np.int8)
    if kv_type == 'fp8':
        return kv_store_fp8(x16, scale_orig_quant)
    raise ValueError(kv_type)


def effective(cache_rows, kv_type, scale_quant_orig=None):
    """float64 values of cache rows as the attention reads them."""
    if kv_type == 'fp16':
        return np.asarray(cache_rows).astype(F64)
    s = F64(F32(scale_quant_orig))
    if kv_type == 'int8':
        return np.asarray(cache_rows).astype(np.int8).astype(F64) * s
    if kv_type == 'fp8':
        return _E4M3[np.asarray(cache_rows).view(np.uint8)].astype(F64) * s
    raise ValueError(kv_type)


def append_ref(q16, k16, v16, cache, past, num_heads, num_kv_heads, head_size, score_scale, kv_type='fp16',
               kv_scale_quant_orig=None, masked_tokens=None, lengths=None):
    """q16 [B, n, H*Dh], k16 / v16 [B, n, Hkv*Dh]: the fp16 values of the appended rows after RoPE (any float dtype); cache
    [B, 2, Hkv, Smax, Dh] float16 / int8 / uint8 as it was BEFORE the append (only slots < past[b] are read); past int [B];
    masked_tokens int [B, Smax] or None.  Returns (out, absmass) float64 [B, n, H*Dh].
    lengths int [B] or None (= n for every sequence): sequence b appends its first lengths[b] rows alone - for it the call is the
    one on q16[b, :lengths[b]] ...; rows from lengths[b] on are padding that is never read (NaN there reaches nothing) and whose
    rows of out and absmass are zero."""
    H, Hkv, Dh = int(num_heads), int(num_kv_heads), int(head_size)
    if not (1 <= Hkv <= H and H % Hkv == 0):
        raise ValueError(f'num_kv_heads {Hkv} must divide num_heads {H}')
    G = H // Hkv
    q = np.asarray(q16, dtype=F64)
    B, n = q.shape[:2]
    q = q.reshape(B, n, H, Dh)
    k = np.asarray(k16, dtype=F64).reshape(B, n, Hkv, Dh)
    v = np.asarray(v16, dtype=F64).reshape(B, n, Hkv, Dh)
    out = np.zeros((B, n, H, Dh), F64)
    absmass = np.zeros((B, n, H, Dh), F64)
    if lengths is not None:
        lengths = np.asarray(lengths)
        if lengths.shape != (B, ) or (lengths < 0).any() or (lengths > n).any():
            raise ValueError(f'lengths must be [B] with values in [0, n = {n}]')
    for b in range(B):
        p = int(past[b])
        nb = n if lengths is None else int(lengths[b])  # the rows of this sequence; the rest is padding, never touched
        seen, _ = visible(p, 0, None if masked_tokens is None else masked_tokens[b])
        allowed = np.concatenate([np.broadcast_to(seen, (nb, p)), np.tril(np.ones((nb, nb), dtype=bool))], axis=1)
        for h in range(H if nb else 0):
            kk = np.concatenate([effective(cache[b, 0, h // G, :p], kv_type, kv_scale_quant_orig), k[b, :nb, h // G]], axis=0)
            vv = np.concatenate([effective(cache[b, 1, h // G, :p], kv_type, kv_scale_quant_orig), v[b, :nb, h // G]], axis=0)
            # a slot that is not seen never enters a product (what it holds, NaN included, is irrelevant)
            kk = np.where(np.concatenate([seen, np.ones(nb, dtype=bool)])[:, None], kk, 0.0)
            vv = np.where(np.concatenate([seen, np.ones(nb, dtype=bool)])[:, None], vv, 0.0)
            s = (q[b, :nb, h] @ kk.T) * F64(score_scale)
            s[~allowed] = -np.inf
            e = np.exp(s - s.max(axis=1, keepdims=True))
            pr = e / e.sum(axis=1, keepdims=True)
            out[b, :nb, h] = pr @ vv
            absmass[b, :nb, h] = pr @ np.abs(vv)
    return out.reshape(B, n, H * Dh), absmass.reshape(B, n, H * Dh)
