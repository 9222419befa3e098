"""The fp8 KV cache rule, restated in numpy (no torch): what kernels/dev_utils.h quant8_fp8 / dequant8_fp8, the cache-write
site of context_attn.hip and the E4M3 instance of mmha_decode.hip compute.

Element type: OCP E4M3 ("e4m3fn"): 1 sign, 4 exponent (bias 7), 3 mantissa bits; no infinities; S.1111.111 is NaN; largest
finite value 448 (0x7e); smallest subnormal 2^-9 (0x01); the subnormals are k * 2^-9, k = 1..7.

Store (wherever the int8 cache stores):
    byte = e4m3fn_rne(clamp(float(x_fp16) * kv_orig_quant_scale, -448, +448))
the product formed in fp32 (one rounding), round-to-nearest-even into the normals and the subnormals alike (2^-10 ties to 0),
the sign of zero kept, the clamp in front of the conversion (the NaN codes are never written).  NaN input is undefined.

Load: the reference computes fp16(float(byte) * kv_quant_orig_scale) per element (`exact=False`).  Every E4M3 value is an fp16
value, so the kernel decodes the bytes to fp16 exactly and applies the scale once to the q.k dot product and once to the
sum of p.v (`exact=True`: float(byte) * scale without the fp16 rounding) - as the int8 instance does.

mmha_decode_fp8 / context_attention_fp8 follow oracle.llama_oracle.mmha_decode / context_attention line for line, with
kv_store_fp8 / kv_load_fp8 in place of kv_store / kv_load."""
import numpy as np

F32 = np.float32
E4M3_MAX = 448.0


def f16(x):
    """Round to IEEE fp16 (nearest-even) and return as float32 (oracle.llama_oracle.f16)."""
    return np.asarray(x, dtype=F32).astype(np.float16).astype(F32)


def _decode_table():
    t = np.zeros(256, dtype=F32)
    for c in range(256):
        e, m = (c >> 3) & 15, c & 7
        if e == 15 and m == 7:
            v = np.nan
        elif e == 0:
            v = m * 2.0 ** -9
        else:
            v = (1.0 + m / 8.0) * 2.0 ** (e - 7)
        t[c] = -v if c & 0x80 else v
    return t


_TABLE = _decode_table()


def kv_store_fp8(x, scale):
    """uint8 E4M3 codes of clamp(float32(x) * float32(scale), +-448), round-to-nearest-even."""
    p = (np.asarray(x, dtype=F32) * F32(scale)).astype(F32)  # one rounding, in fp32
    sign = np.signbit(p)
    a = np.minimum(np.abs(p), F32(E4M3_MAX)).astype(np.float64)  # the clamp; everything below is exact in float64
    # subnormals and zero: multiples of 2^-9 (np.rint rounds half to even); 8 * 2^-9 is the smallest normal, code 0x08
    sub = np.rint(a * 2.0 ** 9)
    # normals: a = (1 + f) * 2^e, the 3-bit mantissa rounded half to even; a mantissa that rounds up to 8 carries into e
    _, ex = np.frexp(np.where(a > 0, a, 1.0))
    e = ex - 1
    mant = np.rint((a / np.exp2(e) - 1.0) * 8.0)
    carry = mant == 8
    e = np.where(carry, e + 1, e)
    mant = np.where(carry, 0.0, mant)
    normal = (e + 7).astype(np.int64) * 8 + mant.astype(np.int64)
    code = np.where(a < 2.0 ** -6, sub.astype(np.int64), normal)
    return (code | np.where(sign, 0x80, 0)).astype(np.uint8)


def kv_load_fp8(codes, scale, exact=False):
    """float32: fp16(value(byte) * scale) (the reference's per-element form), or with `exact` value(byte) * scale in fp32."""
    v = (_TABLE[np.asarray(codes, dtype=np.uint8)] * F32(scale)).astype(F32)
    return v if exact else f16(v)


def mmha_decode_fp8(qkv16, cache, seq_len, input_lengths, max_input_len, timestep, num_heads, head_size, rot_dim,
                    kv_scale_orig_quant, kv_scale_quant_orig, neox=True, q_scaling=1.0, masked_tokens=None,
                    exact_kv_dequant=False):
    """qkv16 [B, 3*H*Dh]; cache [B,2,H,Smax,Dh] np.uint8 (E4M3 codes) updated IN PLACE at slot seq_len[b]; returns the context
    [B, H*Dh] as float32 holding fp16 values.  One fp32 sum for P.V (what the split-KV kernel does)."""
    from oracle.llama_oracle import apply_rope  # the repository's numpy oracle (RoPE: fp32 -> fp16)
    assert cache.dtype == np.uint8
    B = qkv16.shape[0]
    H, Dh = num_heads, head_size
    smax = cache.shape[3]
    inv_sqrt_dh = F32(1.0) / (np.sqrt(F32(Dh)) * F32(q_scaling))
    out = np.zeros((B, H * Dh), dtype=F32)
    qkv = np.asarray(qkv16, dtype=F32).reshape(B, 3, H, Dh)
    for b in range(B):
        tl = int(seq_len[b])
        pos = int(timestep) - (int(max_input_len) - int(input_lengths[b]))
        for h in range(H):
            q = apply_rope(qkv[b, 0, h], pos, rot_dim, neox)
            k = apply_rope(qkv[b, 1, h], pos, rot_dim, neox)
            v = f16(qkv[b, 2, h])
            slot = tl % smax
            cache[b, 0, h, slot] = kv_store_fp8(k, kv_scale_orig_quant)
            cache[b, 1, h, slot] = kv_store_fp8(v, kv_scale_orig_quant)
            kc = kv_load_fp8(cache[b, 0, h, :tl], kv_scale_quant_orig, exact_kv_dequant)
            vc = kv_load_fp8(cache[b, 1, h, :tl], kv_scale_quant_orig, exact_kv_dequant)
            # the current token uses the un-quantised k, v
            keys = np.concatenate([kc, k[None, :]], axis=0)
            vals = np.concatenate([vc, v[None, :]], axis=0)
            qk = (keys @ q).astype(F32) * inv_sqrt_dh
            valid = np.ones(tl + 1, dtype=bool)
            if masked_tokens is not None:
                valid[:tl] = np.asarray(masked_tokens[b, :tl]) == 0
            mx = np.max(qk[valid])
            logit = np.where(valid, np.exp(qk - mx, dtype=F32), F32(0.0)).astype(F32)
            inv_sum = F32(1.0) / (np.sum(logit, dtype=F32) + F32(1e-6))
            p16 = f16(logit * inv_sum)
            out[b, h * Dh:(h + 1) * Dh] = f16((p16[:, None] * vals).sum(axis=0, dtype=F32))
    return out


def context_attention_fp8(qkv16, cache, input_lengths, num_heads, head_size, rot_dim, kv_scale_orig_quant, neox=True,
                          q_scaling=1.0):
    """qkv16 [B, S, 3*H*Dh] (float32 holding fp16 values); cache [B,2,H,Smax,Dh] np.uint8 written for t < S (the prefill
    itself never reads the cache).  Returns (ctx [B,S,H*Dh], qkv_after_rope [B,S,3*H*Dh])."""
    from oracle.llama_oracle import apply_rope
    assert cache.dtype == np.uint8
    B, S, _ = qkv16.shape
    H, Dh = num_heads, head_size
    inv_sqrt_dh = F32(1.0) / (np.sqrt(F32(Dh)) * F32(q_scaling))
    qkv = np.array(qkv16, dtype=F32, copy=True).reshape(B, S, 3, H, Dh)
    out = np.zeros((B, S, H * Dh), dtype=F32)
    for b in range(B):
        n = int(input_lengths[b])
        qkv[b, n:] = 0.0
        for s in range(n):
            qkv[b, s, 0] = apply_rope(qkv[b, s, 0], s, rot_dim, neox)
            qkv[b, s, 1] = apply_rope(qkv[b, s, 1], s, rot_dim, neox)
        for h in range(H):
            k = f16(qkv[b, :, 1, h])
            v = f16(qkv[b, :, 2, h])
            cache[b, 0, h, :S] = kv_store_fp8(k, kv_scale_orig_quant)
            cache[b, 1, h, :S] = kv_store_fp8(v, kv_scale_orig_quant)
            q = f16(qkv[b, :n, 0, h])
            sc = (q @ k[:n].T).astype(F32) * inv_sqrt_dh
            mask = np.tril(np.ones((n, n), dtype=bool))
            sc = sc + np.where(mask, F32(0.0), F32(-10000.0))
            sc = sc - sc.max(axis=-1, keepdims=True)
            e = np.exp(sc, dtype=F32)
            p16 = f16(e / e.sum(axis=-1, keepdims=True, dtype=F32))
            out[b, :n, h * Dh:(h + 1) * Dh] = f16(p16 @ v[:n])
    return out, f16(qkv.reshape(B, S, 3 * H * Dh))
