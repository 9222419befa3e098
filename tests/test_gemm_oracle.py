"""No GPU: oracle/gemm_oracle.py (the reference of tests/test_gpu_gemm_instances.py) against the oracles the project already
trusts - llama_oracle.sq_gemm / gemm_fp16 / woq_matmul, gemv_oracle.gemv at M <= 8 - and the share of the dual SwiGLU GEMM's
98 % allowance that the reference itself uses up."""
import numpy as np
import pytest

import gemm_cases as GC
from oracle import gemm_oracle as GM
from oracle import gemv_oracle as GO
from oracle import llama_oracle as O


def _ord16(a):
    b = np.asarray(a, dtype=np.float16).view(np.int16).astype(np.int32)
    return np.where(b < 0, -(b & 0x7FFF), b)


@pytest.fixture(scope='module')
def ops():
    r = np.random.default_rng(7)
    M, N, K = 37, 53, 192
    d = dict(M=M, N=N, K=K)
    d['a8'] = r.integers(-127, 128, (M, K), dtype=np.int8)
    d['w8'] = r.integers(-127, 128, (N, K), dtype=np.int8)
    d['sr'] = r.uniform(0.01, 0.03, M).astype(np.float32)
    d['sc'] = (r.uniform(0.5, 1.5, N) / (np.sqrt(K) * 73 * 73 * 0.02)).astype(np.float32)
    d['a16'] = (1.7 * r.standard_normal((M, K))).astype(np.float16)
    d['w16'] = (1.7 * r.uniform(-1, 1, (N, K)) / np.sqrt(K)).astype(np.float16)
    d['other'] = r.standard_normal((M, N)).astype(np.float16)
    return d


def test_smoothquant_is_llama_oracle_sq_gemm_bit_for_bit(ops):
    for pc, pt in ((1, 1), (0, 1), (1, 0), (0, 0)):
        sc, sr = (ops['sc'] if pc else ops['sc'][:1]), (ops['sr'] if pt else ops['sr'][:1])
        for dt, name, np_t in ((GO.DT_HALF, 'float16', np.float16), (GO.DT_FLOAT, 'float32', np.float32), (GO.DT_INT32, 'int32', np.int32)):
            s = 1000.0 if dt == GO.DT_INT32 else 1.0
            got = GM.gemm(ops['a8'], ops['w8'], GO.W_INT8_SQ, out_dtype=dt, scale_col=sc * np.float32(s), scale_row=sr)['y']
            ref = O.sq_gemm(ops['a8'], ops['w8'], sr, sc * np.float32(s), name)
            assert np.array_equal(got.astype(np_t), np.asarray(ref).astype(np_t)), (pc, pt, name)
    # residual: one more fp16 rounding of an exact fp16 + fp16 sum
    y = GM.gemm(ops['a8'], ops['w8'], GO.W_INT8_SQ, GM.EPI_RESIDUAL, scale_col=ops['sc'], scale_row=ops['sr'], residual16=ops['other'])['y']
    base = O.sq_gemm(ops['a8'], ops['w8'], ops['sr'], ops['sc'], 'float16')
    want = (np.asarray(base, dtype=np.float64) + ops['other'].astype(np.float64)).astype(np.float16)
    assert np.array_equal(y.astype(np.float16), want)


def test_fp16_and_weight_only_are_the_float32_oracles_to_a_rounding_flip(ops):
    """gemm_fp16 / woq_matmul accumulate in float32: the float64 sums round to the same fp16 but for rare ties"""
    got = GM.gemm(ops['a16'], ops['w16'], GO.W_FP16)['y']
    d = np.abs(_ord16(got) - _ord16(O.gemm_fp16(ops['a16'], ops['w16'])))
    assert d.max() <= 1 and (d == 0).mean() >= 0.99
    for bits, wt in ((8, GO.W_INT8_WOQ), (4, GO.W_INT4_WOQ)):
        q_kn, s = O.woq_quantize(ops['w16'].T.astype(np.float32), bits)
        got = GM.gemm(ops['a16'], q_kn.T, wt, scale_col=s.astype(np.float16))['y']
        d = np.abs(_ord16(got) - _ord16(O.woq_matmul(ops['a16'], q_kn, s)))
        assert d.max() <= 1 and (d == 0).mean() >= 0.99, bits
    # the gate: f16(f16(silu(gate)) * f16(v)) is llama_oracle.swiglu(gate, f16(v)) but for its float32 exponential
    v16 = GO.f16(GM.scaled_sums(ops['a16'], ops['w16'], GO.W_FP16))
    got = GM.gemm(ops['a16'], ops['w16'], GO.W_FP16, GM.EPI_GATE, gate16=ops['other'])['y']
    d = np.abs(_ord16(got) - _ord16(O.swiglu(ops['other'], v16.astype(np.float16))))
    assert d.max() <= 1 and (d == 0).mean() >= 0.99


def test_at_eight_rows_it_is_the_gemv_oracle(ops):
    """the two oracles meet at M <= 8 (what the GEMV slabs of launch_gemm rely on): every weight type, plain / residual, all outputs"""
    a8, a16, res = ops['a8'][:8], ops['a16'][:8], ops['other'][:8]
    for dt in (GO.DT_HALF, GO.DT_FLOAT, GO.DT_INT32):
        g = GM.gemm(a8, ops['w8'], GO.W_INT8_SQ, out_dtype=dt, scale_col=ops['sc'], scale_row=ops['sr'][:8])
        v = GO.gemv(a8, ops['w8'], GO.W_INT8_SQ, GO.EPI_NONE, dt, ops['sc'], ops['sr'][:8])
        assert np.array_equal(g['y'], v['y']) and np.array_equal(g['v'], v['v'])
    q_kn, s = O.woq_quantize(ops['w16'].T.astype(np.float32), 4)
    for wt, w, sc in ((GO.W_FP16, ops['w16'], None), (GO.W_INT4_WOQ, q_kn.T, s.astype(np.float16))):
        for epi_m, epi_v in ((GM.EPI_NONE, GO.EPI_NONE), (GM.EPI_RESIDUAL, GO.EPI_RESIDUAL)):
            g = GM.gemm(a16, w, wt, epi_m, scale_col=sc, residual16=res)
            v = GO.gemv(a16.astype(np.float64), w, wt, epi_v, GO.DT_HALF, sc, None, res)
            assert np.array_equal(g['y'], v['y']) and np.array_equal(g['v'], v['v'])


def test_the_dual_form_is_the_unfused_chain_and_a_float32_exp_moves_few_outputs():
    """(1) the dual oracle is sq_gemm -> sq_gemm -> swiglu -> static quantiser written out with the project's own pieces;
    (2) for the inputs of every dual case of the GPU test, evaluating the oracle with a float32 exponential instead of the float64
    one changes well under 2 % of the outputs (asserted: at most 0.2 %, never by more than 1 LSB) - so the 98 %-identical cap of
    the GPU test is not used up by the reference, and a kernel that loses a fiftieth of its outputs cannot hide behind exp()."""
    from test_gpu_gemm_instances import inputs
    seen = 0
    for c in GC.CASES:
        if c.kernel != GC.DUAL or GC.instance(c)[0] == 'refused':
            continue
        seen += 1
        d = inputs(c)
        N = c.N
        args = (d['a'], d['w'][:N], d['w'][N:], d['scale_col'][:N], d['scale_col'][N:], d['scale_row'], d['qscale'])
        q64 = GM.dual_swiglu_quant(*args)
        q32 = GM.dual_swiglu_quant(*args, exp=GM.exp_f32)
        diff = np.abs(q64.astype(np.int32) - q32.astype(np.int32))
        frac = float((diff != 0).mean())
        print(f'{GC.case_id(c)}: float32 exp changes {100 * frac:.4f} % of {diff.size} outputs, by at most {diff.max()}; '
              f'{100 * float((np.abs(q64) == 127).mean()):.2f} % at +-127')
        assert diff.max() <= 1 and frac <= 0.002, (GC.case_id(c), frac)
        assert (np.abs(q64.astype(np.int32)) >= 127).mean() < 0.05, 'the inputs saturate the quantiser: too little left to compare'
        g16 = O.sq_gemm(d['a'], d['w'][:N], d['scale_row'], d['scale_col'][:N], 'float16')
        u16 = O.sq_gemm(d['a'], d['w'][N:], d['scale_row'], d['scale_col'][N:], 'float16')
        chain = np.clip(np.rint(np.asarray(O.swiglu(g16, u16), dtype=np.float64) * np.float64(d['qscale'])), -128, 127).astype(np.int8)
        dc = np.abs(chain.astype(np.int32) - q64.astype(np.int32))
        assert dc.max() <= 1 and (dc != 0).mean() <= 0.002, GC.case_id(c)
    assert seen >= 8
