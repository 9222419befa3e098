"""The prefill GEMMs (csrc/kernels/gemm*.hip) in numpy float64 - TEST INFRASTRUCTURE ONLY (see llama_oracle.py header).

    C[m, n] = epi( scale(n, m) * sum_k A[m, k] * W[n, k] )

A thin layer over gemv_oracle.py, whose dot_exact / sq_scale / epilogue / f16 / rni_sat / ulp16 hold for any M.  What the GEMMs
add (kernels.h GemmParams):
  silu_gate : C = f16(f16(silu(gate16)) * f16(v))          - the gate is an fp16 INPUT here, the product is what goes through f16
  dual      : two SmoothQuant GEMMs to fp16, SwiGLU in fp16, the static quantiser (tllm_gemm_swiglu_quant)
SmoothQuant sums are exact integers and their scaling is evaluated in float32 as the kernels do: bit for bit."""
import numpy as np

from oracle import gemv_oracle as GO

F64, F32 = np.float64, np.float32
EPI_NONE, EPI_RESIDUAL, EPI_GATE = 'none', 'res', 'gate'


def silu(g, exp=np.exp):
    g = np.asarray(g, dtype=F64)
    return g / (1.0 + exp(-g))


def scaled_sums(a, w, wtype, scale_col=None, scale_row=None):
    """v [M, N]: the value in front of the epilogue's first rounding - float32 (SmoothQuant, the kernel's own arithmetic) or
    float64 (fp16 weights; weight-only integers x their fp16 scale per output channel)"""
    acc = GO.dot_exact(a, w)
    if wtype == GO.W_INT8_SQ:
        return GO.sq_scale(acc, scale_col, np.ones(1, F32) if scale_row is None else scale_row)
    if wtype != GO.W_FP16:
        acc = acc * np.asarray(scale_col, dtype=F64).reshape(1, -1)
    return acc


def gemm(a, w, wtype, epi=EPI_NONE, out_dtype=GO.DT_HALF, scale_col=None, scale_row=None, residual16=None, gate16=None):
    """dict(y, v).  a [M, K]: int8 (SmoothQuant) or fp16 values; w [N, K]: fp16 values or the integers of the quantised types."""
    v = scaled_sums(a, w, wtype, scale_col, scale_row)
    if epi == EPI_GATE:
        y = GO.f16(GO.f16(silu(np.asarray(gate16, dtype=F64))) * GO.f16(v))
    elif epi == EPI_RESIDUAL:
        y = GO.epilogue(v, GO.EPI_RESIDUAL, GO.DT_HALF, residual16)
    else:
        y = GO.epilogue(v, GO.EPI_NONE, out_dtype)
    return dict(y=y, v=np.asarray(v, dtype=F64))


def dual_swiglu_quant(a, w_gate, w_up, s_gate, s_up, s_row, qscale, exp=np.exp):
    """int8 [M, N] = sat(rni(f16(f16(silu(g16)) * u16) * qscale)),  g16 = f16(sq(A W_gate^T)), u16 = f16(sq(A W_up^T)) - the
    rounding points of GEMM + GEMM + SwiGLU + static quantiser run one after the other.  `exp`: the exponential (np.exp in
    float64; a float32 one to measure how far a single-precision exp can move the result)."""
    g16 = GO.f16(GO.sq_scale(GO.dot_exact(a, w_gate), s_gate, s_row))
    u16 = GO.f16(GO.sq_scale(GO.dot_exact(a, w_up), s_up, s_row))
    a16 = GO.f16(silu(g16, exp))
    return GO.rni_sat(GO.f16(a16 * u16) * F64(F32(qscale)), -128, 127).astype(np.int8)


def exp_f32(x):
    """exp evaluated in float32 (correctly rounded to float32 by numpy), carried as float64"""
    return np.exp(np.asarray(x, dtype=F32)).astype(F64)
