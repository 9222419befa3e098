"""The decode GEMV (csrc/kernels/gemv*.hip) in numpy float64 - TEST INFRASTRUCTURE ONLY (see llama_oracle.py header).

    y[m, n] = epi( scale(n, m) * sum_k pro(x)[m, k] * W[n, k] )

with the rounding points the kernel declares (kernels.h GemvParams / Prologue / Epilogue, gemv_impl.h): every stage is evaluated
in float64 and rounded only where the kernel rounds.  fp16 values travel as float64 arrays that hold fp16-representable numbers.
SmoothQuant is the exception: its sum is an exact integer and its scaling `float32(acc) * (float32 s_col * float32 s_row)` is
evaluated in float32, as the kernel (and llama_oracle.sq_gemm) does - that path reproduces the kernel bit for bit.

Numbering of weight types, prologues, epilogues and output types: kernels.h."""
import numpy as np

F64, F32 = np.float64, np.float32
W_FP16, W_INT8_WOQ, W_INT4_WOQ, W_INT8_SQ = 0, 1, 2, 3
PRO_NONE, PRO_RMSNORM, PRO_RMSNORM_QSTATIC, PRO_RMSNORM_QDYN, PRO_QSTATIC, PRO_QDYN = 0, 1, 2, 3, 4, 5
EPI_NONE, EPI_RESIDUAL, EPI_SWIGLU, EPI_SWIGLU_QSTATIC = 0, 1, 2, 3
DT_FLOAT, DT_HALF, DT_INT8, DT_INT32 = 0, 1, 2, 3


def f16(x):
    """round to IEEE fp16 (nearest-even), carried as float64"""
    with np.errstate(over='ignore'):
        return np.asarray(x, dtype=F64).astype(np.float16).astype(F64)


def rni_sat(x, lo, hi):
    """round-half-even, saturate, NaN -> 0 (cvt.rni.sat)"""
    x = np.asarray(x, dtype=F64)
    return np.clip(np.where(np.isnan(x), 0.0, np.rint(x)), lo, hi)


def ulp16(a):
    """the fp16 spacing at |a| (the subnormal spacing 2^-24 below 2^-14)"""
    a = np.maximum(np.abs(np.asarray(a, dtype=F64)), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(a)) - 10)


# ---------------------------------------------------------------------------------------------- prologue
def rmsnorm(x16, gamma16, eps=1e-6):
    """inv = 1 / sqrt(mean(x^2) + eps); n = f16(x * inv); x' = f16(n * gamma)"""
    x = np.asarray(x16, dtype=F64)
    inv = 1.0 / np.sqrt((x * x).mean(axis=-1, keepdims=True) + F64(eps))
    return f16(f16(x * inv) * np.asarray(gamma16, dtype=F64))


def quant_static(xp16, act_scale):
    """q = sat(rni(x' * act_scale))"""
    return rni_sat(np.asarray(xp16, dtype=F64) * F64(F32(act_scale)), -128, 127).astype(np.int8)


def quant_per_token(xp16):
    """amax = max(|x'|, f16(1e-6)); q = sat(rni(x' * 127 / amax)); row scale amax / 127.  Returns (q, scale float64 [M], amax)"""
    x = np.asarray(xp16, dtype=F64)
    amax = np.maximum(np.abs(x).max(axis=-1), f16(1e-6))
    q = rni_sat(x * (127.0 / amax[:, None]), -128, 127).astype(np.int8)
    return q, amax / 127.0, amax


def prologue(x16, pro, gamma16=None, eps=1e-6, act_scale=None):
    """pro(x) of an fp16 input: dict(xp = x' (fp16 values, or int8 behind a quantiser), row_scale = amax / 127 per row or None,
    amax).  PRO_NONE returns x itself."""
    x = np.asarray(x16, dtype=F64)
    if pro in (PRO_RMSNORM, PRO_RMSNORM_QSTATIC, PRO_RMSNORM_QDYN):
        x = rmsnorm(x, gamma16, eps)
    if pro in (PRO_RMSNORM_QSTATIC, PRO_QSTATIC):
        return dict(xp=quant_static(x, act_scale), row_scale=None, amax=None)
    if pro in (PRO_RMSNORM_QDYN, PRO_QDYN):
        q, s, amax = quant_per_token(x)
        return dict(xp=q, row_scale=s, amax=amax)
    return dict(xp=x, row_scale=None, amax=None)


# ---------------------------------------------------------------------------------------------- dot
def dot_exact(xp, w_int_or_f16_nk):
    """sum_k x'[m, k] * W[n, k] in float64: exact products (fp16 x fp16, fp16 x small integer, s8 x s8) - the integer sums of
    SmoothQuant stay below 2^53 and are exact."""
    xp, w = np.asarray(xp), np.asarray(w_int_or_f16_nk)
    if xp.dtype == np.int8 and w.dtype == np.int8:
        # s8 x s8 through sgemm in slices of 1024 terms: |sum| <= 1024 * 128 * 128 = 2^24 is exact in float32 (a float64 copy of
        # a 30 MB weight matrix is what this avoids)
        acc = np.zeros((xp.shape[0], w.shape[0]), F64)
        for k0 in range(0, xp.shape[1], 1024):
            acc += xp[:, k0:k0 + 1024].astype(F32) @ w[:, k0:k0 + 1024].astype(F32).T
        return acc
    return xp.astype(F64) @ w.astype(F64).T


def sq_scale(acc, s_col, s_row):
    """float32(acc) * (float32 s_col[n] * float32 s_row[m]) in float32 (epilogue_per_row_per_col_scale: product of the scales
    first).  acc [M, N] exact integers; s_col [N] or [1]; s_row [M] or [1]."""
    sc = np.asarray(s_col, dtype=F32).reshape(1, -1)
    sr = np.asarray(s_row, dtype=F32).reshape(-1, 1)
    return (np.asarray(acc).astype(F32) * (sc * sr).astype(F32)).astype(F32)


# ---------------------------------------------------------------------------------------------- epilogue
def silu_mul_fp16(g, u):
    """g16 = f16(g); u16 = f16(u); a = f16(g16 / (1 + exp(-g16))); f16(a * u16)"""
    g16, u16 = f16(g), f16(u)
    return f16(f16(g16 / (1.0 + np.exp(-g16))) * u16)


def epilogue(v, epi, out_dtype=DT_HALF, residual16=None, epi_scale=None, u=None):
    """v (and u for SwiGLU): the scaled sums [M, N] - float64 (fp16 / weight-only weights) or the float32 of sq_scale."""
    if epi == EPI_RESIDUAL:
        return f16(f16(v) + np.asarray(residual16, dtype=F64))
    if epi in (EPI_SWIGLU, EPI_SWIGLU_QSTATIC):
        o = silu_mul_fp16(v, u)
        return o if epi == EPI_SWIGLU else rni_sat(o * F64(F32(epi_scale)), -128, 127).astype(np.int8)
    if out_dtype == DT_HALF:
        return f16(v)
    if out_dtype == DT_FLOAT:
        return np.asarray(v, dtype=F64)
    return rni_sat(v, -2147483648, 2147483647).astype(np.int32)


def gemv(xp, w, wtype, epi=EPI_NONE, out_dtype=DT_HALF, scale_col=None, scale_row=None, residual16=None, epi_scale=None):
    """The dot and the epilogue on a prologue result `xp` [M, K].  `w`: the weight values [N, K] (SwiGLU: the stacked [2N, K]
    rows gate | up) - fp16 values, or the integers of the quantised types.  scale_col: fp16 [rows] (weight-only), float32 [rows]
    or [1] (SmoothQuant); scale_row: float32 [M] or [1] (SmoothQuant).  Returns dict(y, v[, u]): v / u are the scaled sums before
    the epilogue's first rounding (gate / up for SwiGLU)."""
    acc = dot_exact(xp, w)
    swiglu = epi in (EPI_SWIGLU, EPI_SWIGLU_QSTATIC)
    rows = acc.shape[1]
    if wtype == W_INT8_SQ:
        sc = np.asarray(scale_col, dtype=F32).reshape(-1)
        sr = np.ones(1, F32) if scale_row is None else scale_row
        if swiglu:
            n = rows // 2
            g = sq_scale(acc[:, :n], sc[:n] if sc.size > 1 else sc, sr)
            u = sq_scale(acc[:, n:], sc[n:] if sc.size > 1 else sc, sr)
        else:
            g, u = sq_scale(acc, sc, sr), None
    else:
        if wtype != W_FP16:
            acc = acc * np.asarray(scale_col, dtype=F64).reshape(1, -1)
        g, u = (acc[:, :rows // 2], acc[:, rows // 2:]) if swiglu else (acc, None)
    out = dict(y=epilogue(g, epi, out_dtype, residual16, epi_scale, u), v=np.asarray(g, dtype=F64))
    if swiglu:
        out['u'] = np.asarray(u, dtype=F64)
    return out
