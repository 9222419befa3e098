"""Grouped-query attention, restated in numpy (no torch) through the multi-head oracle.

Hkv K/V heads serve H query heads, 1 <= Hkv <= H, H % Hkv == 0, G = H / Hkv: query head h reads K/V head h // G.  That is
multi-head attention with every K/V head repeated G times, so the repository's oracle (oracle/llama_oracle.py, and
kv_fp8_ref.py for the E4M3 cache) is the oracle here too, applied to expanded inputs:

    fused QKV row   [ q: H*Dh | k: Hkv*Dh | v: Hkv*Dh ]   --expand_qkv-->         [ q: H*Dh | k: H*Dh | v: H*Dh ]
    cache           [B, 2, Hkv, Smax, Dh]                 --expand_cache-->       [B, 2, H, Smax, Dh]   (<--fold_cache--)
    QKV weight      [(H + 2*Hkv)*Dh, hidden]              --expand_qkv_weight-->  [3*H*Dh, hidden]

RoPE, the cache quantisation and the cache store are functions of one K/V row alone, so the G copies the oracle writes are
identical and fold_cache (which checks that) keeps one of them: what the kernels store once per K/V head.

decode / context take the cache element type from the cache array: np.float16, np.int8, or np.uint8 for E4M3 codes."""
import numpy as np

F32 = np.float32


def _group(num_heads, num_kv_heads):
    H, Hkv = int(num_heads), int(num_kv_heads)
    if not (1 <= Hkv <= H and H % Hkv == 0):
        raise ValueError(f'num_kv_heads {Hkv} must divide num_heads {H}')
    return H // Hkv


def expand_qkv(qkv, num_heads, num_kv_heads, head_size):
    """[..., (H + 2*Hkv)*Dh] -> [..., 3*H*Dh]: K/V head j repeated for the query heads j*G .. j*G + G - 1."""
    H, Hkv, Dh = num_heads, num_kv_heads, head_size
    G = _group(H, Hkv)
    qkv = np.asarray(qkv)
    if qkv.shape[-1] != (H + 2 * Hkv) * Dh:
        raise ValueError(f'last extent {qkv.shape[-1]} is not (H + 2*Hkv)*Dh = {(H + 2 * Hkv) * Dh}')
    lead = qkv.shape[:-1]
    q = qkv[..., :H * Dh]
    k = qkv[..., H * Dh:(H + Hkv) * Dh].reshape(lead + (Hkv, Dh))
    v = qkv[..., (H + Hkv) * Dh:].reshape(lead + (Hkv, Dh))
    k = np.repeat(k, G, axis=-2).reshape(lead + (H * Dh, ))
    v = np.repeat(v, G, axis=-2).reshape(lead + (H * Dh, ))
    return np.concatenate([q, k, v], axis=-1)


def fold_qkv(qkv, num_heads, num_kv_heads, head_size):
    """The inverse of expand_qkv on its image: [..., 3*H*Dh] -> [..., (H + 2*Hkv)*Dh] (the first copy of every K/V head)."""
    H, Hkv, Dh = num_heads, num_kv_heads, head_size
    G = _group(H, Hkv)
    qkv = np.asarray(qkv)
    lead = qkv.shape[:-1]
    q = qkv[..., :H * Dh]
    k = qkv[..., H * Dh:2 * H * Dh].reshape(lead + (H, Dh))[..., ::G, :].reshape(lead + (Hkv * Dh, ))
    v = qkv[..., 2 * H * Dh:].reshape(lead + (H, Dh))[..., ::G, :].reshape(lead + (Hkv * Dh, ))
    return np.concatenate([q, k, v], axis=-1)


def expand_cache(cache, num_heads):
    """[B, 2, Hkv, S, Dh] -> [B, 2, H, S, Dh] (a copy)."""
    cache = np.asarray(cache)
    G = _group(num_heads, cache.shape[2])
    return np.repeat(cache, G, axis=2)


def fold_cache(cache, num_kv_heads, check=True):
    """[B, 2, H, S, Dh] -> [B, 2, Hkv, S, Dh]; with `check` the G copies of every K/V head must be identical."""
    cache = np.asarray(cache)
    G = _group(cache.shape[2], num_kv_heads)
    folded = cache[:, :, ::G]
    if check and not np.array_equal(np.repeat(folded, G, axis=2), cache):
        raise ValueError('fold_cache: the copies of a K/V head differ')
    return np.ascontiguousarray(folded)


def expand_qkv_weight(w, num_heads, num_kv_heads, head_size):
    """[(H + 2*Hkv)*Dh, ...] -> [3*H*Dh, ...]: the rows (output channels) of k and v repeated per query head.  Serves the weight
    [rows, hidden] and anything per output channel (a bias, per-channel scales) alike."""
    w = np.asarray(w)
    return np.moveaxis(expand_qkv(np.moveaxis(w, 0, -1), num_heads, num_kv_heads, head_size), -1, 0)


def decode(qkv16, cache, seq_len, input_lengths, max_input_len, timestep, num_heads, num_kv_heads, head_size, rot_dim,
           neox=True, q_scaling=1.0, masked_tokens=None, kv_scale_orig_quant=None, kv_scale_quant_orig=None,
           exact_kv_dequant=False):
    """One generation step.  qkv16 [B, (H + 2*Hkv)*Dh]; cache [B, 2, Hkv, Smax, Dh] (np.float16, np.int8 or np.uint8 = E4M3
    codes) updated IN PLACE at slot seq_len[b]; returns the context [B, H*Dh] as float32 holding fp16 values."""
    from oracle import llama_oracle as O
    H, Hkv, Dh = num_heads, num_kv_heads, head_size
    big = expand_cache(cache, H)
    q3 = expand_qkv(np.asarray(qkv16, dtype=F32), H, Hkv, Dh)
    if big.dtype == np.uint8:
        from . import kv_fp8_ref as F8
        out = F8.mmha_decode_fp8(q3, big, seq_len, input_lengths, max_input_len, timestep, H, Dh, rot_dim, kv_scale_orig_quant,
                                 kv_scale_quant_orig, neox, q_scaling, masked_tokens, exact_kv_dequant)
    else:
        out = O.mmha_decode(q3, big, seq_len, input_lengths, max_input_len, timestep, H, Dh, rot_dim, neox, q_scaling,
                            masked_tokens, kv_scale_orig_quant, kv_scale_quant_orig, False, exact_kv_dequant)
    cache[...] = fold_cache(big, Hkv)
    return out


def context(qkv16, cache, input_lengths, num_heads, num_kv_heads, head_size, rot_dim, neox=True, q_scaling=1.0,
            kv_scale_orig_quant=None):
    """The prompt pass.  qkv16 [B, S, (H + 2*Hkv)*Dh] (float32 holding fp16 values); cache [B, 2, Hkv, Smax, Dh] written for
    t < S.  Returns (ctx [B, S, H*Dh], qkv_after_rope [B, S, (H + 2*Hkv)*Dh])."""
    from oracle import llama_oracle as O
    H, Hkv, Dh = num_heads, num_kv_heads, head_size
    big = expand_cache(cache, H)
    q3 = expand_qkv(np.asarray(qkv16, dtype=F32), H, Hkv, Dh)
    if big.dtype == np.uint8:
        from . import kv_fp8_ref as F8
        out, roped = F8.context_attention_fp8(q3, big, input_lengths, H, Dh, rot_dim, kv_scale_orig_quant, neox, q_scaling)
    else:
        out, roped = O.context_attention(q3, big, input_lengths, H, Dh, rot_dim, neox, q_scaling, kv_scale_orig_quant)
    cache[...] = fold_cache(big, Hkv)
    return out, fold_qkv(roped, H, Hkv, Dh)
