"""The row-wise and element-wise kernels (csrc/kernels/pointwise.hip) in numpy float64 - TEST INFRASTRUCTURE ONLY (see
llama_oracle.py header).

Every stage is evaluated in float64 and rounded only where the kernel rounds; fp16 values travel as float64 arrays that hold
fp16-representable numbers (gemv_oracle.py, whose helpers this module uses as they are).  Two groups are not float64:

  * the quantiser tails `*_f32` restate the kernel step by step in float32 - `float32(y16) * float32(scale)`, `127.f / amax`,
    `amax / 127.f`, each a single IEEE operation in a build without fast-math - and reproduce q and the row scales bit for bit
    when fed the kernel's own y;
  * fill_random: hash32 in uint32 and single float32 operations, bit for bit."""
import numpy as np

from .gemv_oracle import f16, quant_per_token, quant_static, rmsnorm, rni_sat, silu_mul_fp16, ulp16  # noqa: F401

F64, F32 = np.float64, np.float32
DT_FLOAT, DT_HALF, DT_INT8, DT_FP8 = 0, 1, 2, 6  # kernels.h DType


# ---------------------------------------------------------------------------------------------- norms
def add_rmsnorm(x16, gamma16, eps=1e-6, residual16=None):
    """x' = f16(x + residual) (x itself without a residual); returns (rmsnorm(x') gamma, x' = what sum_out receives or None)"""
    x = np.asarray(x16, dtype=F64)
    if residual16 is None:
        return rmsnorm(x, gamma16, eps), None
    s = f16(x + np.asarray(residual16, dtype=F64))
    return rmsnorm(s, gamma16, eps), s


def layernorm(x16, gamma16, beta16, eps=1e-5, use_diff_of_squares=True):
    """y = f16((x - mean) * rstd * gamma + beta), one rounding; var = E[x^2] - mean^2 or E[(x - mean)^2], clamped at 0"""
    x = np.asarray(x16, dtype=F64)
    mean = x.mean(axis=-1, keepdims=True)
    if use_diff_of_squares:
        var = (x * x).mean(axis=-1, keepdims=True) - mean * mean
    else:
        var = ((x - mean) ** 2).mean(axis=-1, keepdims=True)
    rstd = 1.0 / np.sqrt(np.maximum(var, 0.0) + F64(F32(eps)))
    return f16((x - mean) * rstd * np.asarray(gamma16, dtype=F64) + np.asarray(beta16, dtype=F64))


def norm(x16, gamma16, eps, residual16=None, beta16=None, layernorm_=False, use_diff_of_squares=True):
    """the RmsnormParams call: (y, sum_out or None)"""
    if not layernorm_:
        return add_rmsnorm(x16, gamma16, eps, residual16)
    s = None if residual16 is None else f16(np.asarray(x16, dtype=F64) + np.asarray(residual16, dtype=F64))
    return layernorm(x16 if s is None else s, gamma16, beta16, eps, use_diff_of_squares), s


# ---------------------------------------------------------------------------------------------- quantiser tails, float32
def _rni_sat_i8_f32(v):
    with np.errstate(invalid='ignore'):
        return np.clip(np.where(np.isnan(v), F32(0), np.rint(v)), -128, 127).astype(np.int8)


def quant_static_f32(y16, scale):
    """q = sat(rni(float32(y16) * float32(scale))), NaN -> 0: the kernels' static tail (and quantize_tensor), step by step"""
    with np.errstate(over='ignore', invalid='ignore'):
        return _rni_sat_i8_f32(np.asarray(y16).astype(F32) * F32(scale))


def quant_per_token_f32(y16, floor=None):
    """amax = max(|y|, f16(1e-6)) per row; qs = 127.f / amax; q = sat(rni(float32(y16) * qs)); scale = amax / 127.f.
    Returns (q int8, scale float32 [rows], amax float32 [rows])"""
    y = np.asarray(y16).astype(F32)
    floor = F32(np.float16(F32(1e-6))) if floor is None else F32(floor)
    amax = np.maximum(np.abs(y).max(axis=-1), floor).astype(F32)
    qs = (F32(127.0) / amax).astype(F32)
    return _rni_sat_i8_f32(y * qs[..., None]), (amax / F32(127.0)).astype(F32), amax


# ---------------------------------------------------------------------------------------------- element-wise
def swiglu(a16, b16):
    """f16(f16(silu(a)) * b) (gemv_oracle.silu_mul_fp16; exp overflows to inf for a = -65504: silu = -0)"""
    with np.errstate(over='ignore', invalid='ignore'):
        return silu_mul_fp16(a16, b16)


def swiglu_quant(a16, b16, scale):
    """sat(rni(swiglu * scale)), NaN -> 0, +-inf saturate"""
    with np.errstate(over='ignore', invalid='ignore'):
        return rni_sat(swiglu(a16, b16) * F64(F32(scale)), -128, 127).astype(np.int8)


def add(a16, b16):
    """f16(a + b): one rounding (the float32 sum of two fp16 values is exact or rounds as the float64 one does to fp16)"""
    with np.errstate(invalid='ignore'):
        return f16(np.asarray(a16, dtype=F64) + np.asarray(b16, dtype=F64))


def embedding(ids, table):
    """out[t] = table[ids[t]]; an id outside [0, vocab) gives a zero row.  The table's dtype is kept (bits travel)"""
    ids = np.asarray(ids, dtype=np.int64)
    table = np.asarray(table)
    ok = (ids >= 0) & (ids < table.shape[0])
    out = table[np.where(ok, ids, 0)].copy()
    out[~ok] = 0
    return out


def gather_last_token(hidden, last_token_ids):
    """hidden [batch, seq, hs]: out[b] = hidden[b, clamp(id - 1, 0, seq - 1)]"""
    hidden = np.asarray(hidden)
    pos = np.clip(np.asarray(last_token_ids, dtype=np.int64) - 1, 0, hidden.shape[1] - 1)
    return hidden[np.arange(hidden.shape[0]), pos].copy()


def gather_rows(hidden, rows):
    return np.asarray(hidden)[np.asarray(rows, dtype=np.int64)].copy()


def exclusive_scan(lens):
    """cu[0] = 0, cu[i + 1] = cu[i] + lens[i] in int32 (n + 1 entries)"""
    lens = np.asarray(lens, dtype=np.int64)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64).astype(np.int32)


# ---------------------------------------------------------------------------------------------- fills
def hash32(x):
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def fill_random(dtype, n, seed, scale=1.0):
    """fill_random_kernel, bit for bit: r = hash32(uint32(i) * 2654435761 + seed) ^ hash32(uint32(i >> 32) + seed * 31);
    fp16 / fp32: ((float32(r >> 8) * 2^-23) - 1) * scale (every step exact or a single float32 operation), fp16 rounded once
    more; int8: r % 255 - 127; E4M3: (r & 0x80) | ((r >> 8) & 0x3f)"""
    i = np.arange(n, dtype=np.uint64)
    seed = np.uint32(seed)
    with np.errstate(over='ignore'):
        lo = (i & np.uint64(0xffffffff)).astype(np.uint32) * np.uint32(2654435761) + seed
        hi = (i >> np.uint64(32)).astype(np.uint32) + seed * np.uint32(31)
        r = hash32(lo) ^ hash32(hi)
    if dtype == DT_INT8:
        return ((r % np.uint32(255)).astype(np.int32) - 127).astype(np.int8)
    if dtype == DT_FP8:
        return ((r & np.uint32(0x80)) | ((r >> np.uint32(8)) & np.uint32(0x3f))).astype(np.uint8)
    u = ((r >> np.uint32(8)).astype(F32) * F32(1.0 / 8388608.0)).astype(F32)
    v = ((u - F32(1.0)).astype(F32) * F32(scale)).astype(F32)
    return v.astype(np.float16) if dtype == DT_HALF else v
