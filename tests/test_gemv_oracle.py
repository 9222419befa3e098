"""No GPU: oracle/gemv_oracle.py (float64, the decode GEMV's rounding points) pinned to the oracle functions the rest of the suite
already rests on (oracle/llama_oracle.py, float32 with the same rounding points) - exact where both are exact, within a rounding of
the float32 evaluation elsewhere - and to the host-side weight layout of the product."""
import numpy as np
import pytest

from oracle import gemv_oracle as GO
from oracle import llama_oracle as O
from oracle.quant_oracle import process_woq_layout


def rng(seed):
    return np.random.default_rng(seed)


def _ord16(a):
    b = np.asarray(a, dtype=np.float16).view(np.int16).astype(np.int32)
    return np.where(b < 0, -(b & 0x7FFF), b)


@pytest.mark.parametrize('k', [64, 4096, 11008])
def test_prologues_against_the_float32_oracle(k):
    r = rng(k)
    x = (1.7 * r.standard_normal((8, k))).astype(np.float16)
    gamma = r.uniform(0.5, 1.5, k).astype(np.float16)
    # RMSNorm: the float32 evaluation rounds inv and x * inv once more before the fp16 rounding - at most 2 ulp, almost never
    mine, theirs = GO.rmsnorm(x, gamma), O.rmsnorm(x, gamma)
    d = np.abs(_ord16(mine) - _ord16(theirs))
    assert d.max() <= 2 and (d == 0).mean() >= 0.999, (d.max(), (d == 0).mean())
    # quantisers on the SAME fp16 input: identical up to a product that lands on a tie in one of the two precisions
    y = theirs
    q_s = GO.quant_static(y, 37.0)
    assert np.array_equal(q_s, O.quantize_tensor(y, 37.0))
    q, s, amax = GO.quant_per_token(y)
    q_o, s_o = O.quantize_per_token(y)
    assert np.array_equal(amax, np.abs(y).max(-1)) and np.array_equal(s.astype(np.float32), s_o[:, 0])
    dq = np.abs(q.astype(np.int32) - q_o.astype(np.int32))
    assert dq.max() <= 1 and (dq == 0).mean() >= 0.999
    # the fused forms
    p = GO.prologue(x, GO.PRO_RMSNORM_QSTATIC, gamma, 1e-6, 37.0)
    q_o, _ = O.rmsnorm_quant(x, gamma, 1e-6, 37.0)
    dq = np.abs(p['xp'].astype(np.int32) - q_o.astype(np.int32))
    assert dq.max() <= 1 and (dq == 0).mean() >= 0.99
    p = GO.prologue(x, GO.PRO_RMSNORM_QDYN, gamma)
    q_o, s_o = O.rmsnorm_quant(x, gamma)
    dq = np.abs(p['xp'].astype(np.int32) - q_o.astype(np.int32))
    assert dq.max() <= 1 and (dq == 0).mean() >= 0.99
    np.testing.assert_allclose(p['row_scale'], s_o[:, 0], rtol=2.0 ** -9)  # amax itself may sit 2 fp16 ulp apart
    assert GO.prologue(x, GO.PRO_NONE)['xp'].dtype == np.float64 and np.array_equal(GO.prologue(x, GO.PRO_NONE)['xp'], x)
    # the per-token floor: a row of zeros quantises against f16(1e-6)
    q, s, amax = GO.quant_per_token(np.zeros((1, 8), np.float16))
    assert amax[0] == np.float64(np.float16(1e-6)) and not q.any()


@pytest.mark.parametrize('out,name', [(GO.DT_HALF, 'float16'), (GO.DT_FLOAT, 'float32'), (GO.DT_INT32, 'int32')])
@pytest.mark.parametrize('per_channel,per_token', [(1, 1), (0, 0), (1, 0)])
def test_smoothquant_is_sq_gemm_bit_for_bit(out, name, per_channel, per_token):
    r = rng(7 + out)
    m, n, k = 5, 37, 1500
    a = r.integers(-128, 128, (m, k)).astype(np.int8)
    w = r.integers(-128, 128, (n, k)).astype(np.int8)
    sa = (r.integers(1, 13, m if per_token else 1) * 1e-2).astype(np.float32)
    sb = (r.integers(1, 13, n if per_channel else 1) * 1e-2).astype(np.float32)
    ref = O.sq_gemm(a, w, sa, sb, name)
    got = GO.gemv(a, w, GO.W_INT8_SQ, GO.EPI_NONE, out, sb, sa)['y']
    assert np.array_equal(got.astype(ref.dtype), ref)
    assert np.array_equal(GO.dot_exact(a, w), a.astype(np.int64) @ w.astype(np.int64).T)
    # residual: fp16(fp16(v) + residual), and the SwiGLU forms on the stacked rows
    res = r.standard_normal((m, n)).astype(np.float16)
    got = GO.gemv(a, w, GO.W_INT8_SQ, GO.EPI_RESIDUAL, GO.DT_HALF, sb, sa, res)['y']
    assert np.array_equal(got, O.f16(O.sq_gemm(a, w, sa, sb) + res.astype(np.float32)))
    if out == GO.DT_HALF:
        sb2 = (r.uniform(0.5, 1.5, 2 * n if per_channel else 1) * 2e-6).astype(np.float32)
        w2 = np.concatenate([w, r.integers(-128, 128, (n, k)).astype(np.int8)])
        o = GO.gemv(a, w2, GO.W_INT8_SQ, GO.EPI_SWIGLU, GO.DT_HALF, sb2, sa)
        g = O.sq_gemm(a, w2[:n], sa, sb2[:n] if per_channel else sb2)
        u = O.sq_gemm(a, w2[n:], sa, sb2[n:] if per_channel else sb2)
        d = np.abs(_ord16(o['y']) - _ord16(O.swiglu(g, u)))  # float32 exp against float64 exp
        assert d.max() <= 1 and (d == 0).mean() >= 0.99
        oq = GO.gemv(a, w2, GO.W_INT8_SQ, GO.EPI_SWIGLU_QSTATIC, GO.DT_INT8, sb2, sa, epi_scale=21.0)['y']
        assert oq.dtype == np.int8 and np.array_equal(oq, O.quantize_tensor(o['y'], 21.0))


@pytest.mark.parametrize('bits', [8, 4])
def test_weight_only_and_fp16_against_the_float32_oracle(bits):
    r = rng(bits)
    m, n, k = 3, 40, 2056
    x = (1.7 * r.standard_normal((m, k))).astype(np.float16)
    w = (1.7 * r.uniform(-1, 1, (n, k)) / np.sqrt(k)).astype(np.float16)
    q_kn, s = O.woq_quantize(w.T.astype(np.float32), bits)
    wt = GO.W_INT8_WOQ if bits == 8 else GO.W_INT4_WOQ
    o = GO.gemv(x, q_kn.T, wt, scale_col=s.astype(np.float16))
    ref = O.woq_matmul(x, q_kn, s)  # float32 accumulation: a fraction of an ulp from the exact sum, then the same one rounding
    assert np.abs(o['y'] - ref).max() <= GO.ulp16(np.abs(ref).max())
    assert (o['y'] == ref).mean() >= 0.95
    assert np.abs(o['y'] - o['v']).max() <= 0.5 * GO.ulp16(np.abs(o['v']).max())
    o = GO.gemv(x, w, GO.W_FP16)
    ref = O.gemm_fp16(x, w)
    assert np.abs(o['y'] - ref).max() <= GO.ulp16(np.abs(ref).max()) and (o['y'] == ref).mean() >= 0.95
    assert np.array_equal(GO.gemv(x, w, GO.W_FP16, out_dtype=GO.DT_FLOAT)['y'], o['v'])
    # SwiGLU on the stacked rows [gate | up]
    o = GO.gemv(x, w, GO.W_FP16, GO.EPI_SWIGLU)
    assert o['y'].shape == (m, n // 2)
    ref = O.swiglu(O.gemm_fp16(x, w[:n // 2]), O.gemm_fp16(x, w[n // 2:]))
    assert np.abs(_ord16(o['y']) - _ord16(ref)).max() <= 4  # a 1-ulp difference of gate or up carried through
    assert np.array_equal(GO.silu_mul_fp16(o['v'], o['u']), o['y'])
    # the processed layout the GPU test uploads holds exactly these integers: int8 bytes q + 128, int4 nibbles q + 8 in the
    # order e0 e2 e4 e6 e1 e3 e5 e7 of every 32-bit word (weight_layout.h)
    p = process_woq_layout(q_kn, bits).view(np.uint8)
    if bits == 8:
        assert np.array_equal(p[:, :k].astype(np.int16) - 128, q_kn.T) and (p[:, k:] == 128).all()
    else:
        words = p.view(np.uint32)
        back = np.stack([(words >> (4 * pos)) & 0xF for pos in (0, 4, 1, 5, 2, 6, 3, 7)], axis=-1).reshape(n, -1).astype(np.int16) - 8
        assert np.array_equal(back[:, :k], q_kn.T) and not back[:, k:].any()


def test_ulp16_and_the_saturating_rounding():
    assert GO.ulp16(1.0) == 2.0 ** -10 and GO.ulp16(1.999) == 2.0 ** -10 and GO.ulp16(2.0) == 2.0 ** -9 and GO.ulp16(0.0) == 2.0 ** -24
    assert list(GO.rni_sat([0.5, 1.5, 2.5, -0.5, -1.5, 300.0, -300.0, np.nan], -128, 127)) == [0, 2, 2, 0, -2, 127, -128, 0]
    assert np.array_equal(GO.f16([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 70000.0]), [1.0, 1.0 + 2.0 ** -9, np.inf])
