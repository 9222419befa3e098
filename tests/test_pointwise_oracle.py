"""No GPU: oracle/pointwise_oracle.py against the float32 oracle the plugin tests use (llama_oracle.py), on the inputs of
tests/pointwise_cases.py, and a float32 emulation of the kernels' summation order against every cap that
tests/test_gpu_pointwise_instances.py sets - so the inputs alone do not break a cap.

The emulation is not exact (it does not restate the backend's fused multiply-adds or its rsqrt): per-thread partial sums over
ascending k, a pairwise tree over the 64 lanes of a wave, the four waves in order."""
import numpy as np
import pytest

import pointwise_cases as PC
from oracle import llama_oracle as O
from oracle import pointwise_oracle as PO

F32 = np.float32
RUN = [c for c in PC.RMS_CASES if c.expect > 0]
_memo = {}


def inputs(c):
    """one set of operands and one float64 reference per case, shared by the tests below and never modified"""
    k = PC.rms_id(c)
    if k not in _memo:
        d = PC.rms_inputs(c)
        y, s = PO.norm(d['x'], d['gamma'], d['eps'], d['residual'] if c.residual else None, d['beta'], bool(c.ln), bool(c.diff_sq))
        _memo[k] = (d, y, s)
    return _memo[k]


def _assert_stage_a(got, ref, what):
    worst, differ, cap = PC.within_ulp16(got, ref)
    assert worst <= 2.0 and differ <= cap, (what, worst, differ, cap)
    return worst, differ


# ---------------------------------------------------------------------------------------------- against llama_oracle
@pytest.mark.parametrize('c', RUN, ids=PC.rms_id)
def test_the_norm_oracle_reproduces_the_float32_oracle(c):
    d, y, s = inputs(c)
    x = d['x'].astype(F32) if s is None else s.astype(F32)
    if c.ln:
        for static in (None, d['scale']):
            q32, s32 = O.layernorm_quant(x, d['gamma'].astype(F32), d['beta'].astype(F32), d['eps'], static, bool(c.diff_sq))
            if static is None:
                q, sc, _ = PO.quant_per_token(y)
                np.testing.assert_allclose(sc, s32.reshape(-1), rtol=2.0 ** -9)  # amax within 2 fp16 ulp
            else:
                q = PO.quant_static(y, static)
            dq = np.abs(q.astype(np.int32) - q32.astype(np.int32))
            assert dq.max() <= 1 and (dq != 0).sum() <= max(2, dq.size // 50), (dq.max(), (dq != 0).sum())
        return
    _assert_stage_a(O.rmsnorm(x, d['gamma'].astype(F32), d['eps']), y, 'rmsnorm')
    q32, _ = O.rmsnorm_quant(x, d['gamma'].astype(F32), d['eps'], d['scale'])
    dq = np.abs(PO.quant_static(y, d['scale']).astype(np.int32) - q32.astype(np.int32))
    assert dq.max() <= 1 and (dq != 0).sum() <= max(2, dq.size // 50)
    # the float32 restatement of the per-token tail IS llama_oracle's quantiser: bit for bit on the same y
    y16 = y.astype(np.float16)
    q, sc, _ = PO.quant_per_token_f32(y16)
    q0, s0 = O.quantize_per_token(y16.astype(F32))
    assert np.array_equal(q, q0) and np.array_equal(sc, s0.reshape(-1))
    assert np.array_equal(PO.quant_static_f32(y16, d['scale']), O.quantize_tensor(y16.astype(F32), d['scale']))
    # and the float64 tail agrees with the float32 one except where float32 rounding moves a product across a tie (fp16 y over an
    # fp16 amax lands on exact halves often): 1 LSB, the Stage-A cap on how many
    dq = np.abs(q.astype(np.int32) - PO.quant_per_token(y)[0].astype(np.int32))
    assert dq.max() <= 1 and (dq != 0).sum() <= max(2, dq.size // 100)


def test_the_swiglu_oracle_reproduces_the_float32_oracle():
    a, b = PC.ew_inputs(33024, 7)
    ref = PO.swiglu(a, b)
    with np.errstate(over='ignore', invalid='ignore'):
        got = O.swiglu(a.astype(F32), b.astype(F32))
    worst, differ, cap = PC.within_ulp16(got, ref)
    assert worst <= 2.0 and differ <= cap, (worst, differ)
    # the pinned elements: g = +-0 -> 0, g = -65504 -> 0, NaN -> NaN, 65504 * 1 stays, 60000 * 60000 -> inf
    assert ref[0] == 0 and ref[1] == 0 and ref[3] == 0 and ref[8] == 0 and ref[11] == 0 and np.isnan(ref[7]) and np.isnan(ref[15])
    assert ref[2] == 65504.0 and ref[10] == -49120.0 and ref[16] == np.inf
    q = PO.swiglu_quant(a, b, 21.0)
    assert q[7] == 0 and q[16] == 127 and q[2] == 127 and q[10] == -128


def test_the_small_oracles():
    a, b = PC.ew_inputs(64, 3)
    s = PO.add(a, b)
    assert s[16] == np.inf and s[17] == -np.inf and np.isnan(s[7]) and s[2] == 65504.0 and s[4] == -19.0
    assert np.array_equal(PO.exclusive_scan([3, 0, 5]), np.array([0, 3, 3, 8], np.int32)) and PO.exclusive_scan([]).tolist() == [0]
    t = np.arange(12, dtype=np.float16).reshape(4, 3) + 1
    e = PO.embedding(np.array([3, -1, 4, 0, 2 ** 31 - 1], np.int32), t)
    assert e.tolist() == [[10, 11, 12], [0, 0, 0], [0, 0, 0], [1, 2, 3], [0, 0, 0]]
    h = np.arange(2 * 3 * 2, dtype=np.float16).reshape(2, 3, 2)
    assert PO.gather_last_token(h, [0, 9]).tolist() == [[0, 1], [10, 11]] and PO.gather_last_token(h, [2, -3]).tolist() == [[2, 3], [6, 7]]
    assert PO.gather_rows(t, [2, 2, 0]).tolist() == [[7, 8, 9], [7, 8, 9], [1, 2, 3]]


def test_fill_random_oracle_properties():
    n = 4096
    f8 = PO.fill_random(PO.DT_FP8, n, 77)
    assert ((f8 & 0x7f) <= 0x3f).all() and not np.isin(f8, [0x7f, 0xff]).any() and len(np.unique(f8)) > 100
    i8 = PO.fill_random(PO.DT_INT8, n, 77)
    assert i8.min() >= -127 and len(np.unique(i8)) > 200
    for dt in (PO.DT_HALF, PO.DT_FLOAT):
        v = PO.fill_random(dt, n, 77, 0.5).astype(np.float64)
        assert np.abs(v).max() <= 0.5 and abs(v.mean()) < 0.05 and v.std() > 0.2
    # hash32 by hand on one word, and the seed matters
    x = 1
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    assert int(PO.hash32(np.uint32(1))) == x
    assert not np.array_equal(PO.fill_random(PO.DT_INT8, n, 77), PO.fill_random(PO.DT_INT8, n, 78))


# ---------------------------------------------------------------------------------------------- the kernels' summation order
def _block_sum(per_thread):
    """[M, 256] float32 -> [M]: a pairwise tree over each wave's 64 lanes, then 0 + w0 + w1 + w2 + w3"""
    v = per_thread.astype(F32).reshape(per_thread.shape[0], 4, 64)
    while v.shape[-1] > 1:
        v = (v[..., 0::2] + v[..., 1::2]).astype(F32)
    t = np.zeros(per_thread.shape[0], F32)
    for w in range(4):
        t = (t + v[:, w, 0]).astype(F32)
    return t


def _per_thread(vals, vec):
    """[M, N] float32 terms -> [M, 256] partial sums: thread t owns k = (t + 256 j) * vec + i, summed over ascending k"""
    M, N = vals.shape
    per = -(-N // (256 * vec)) * vec
    pad = np.zeros((M, per // vec * 256 * vec), F32)
    pad[:, :N] = vals
    owned = pad.reshape(M, per // vec, 256, vec).transpose(0, 2, 1, 3).reshape(M, 256, per)
    acc = np.zeros((M, 256), F32)
    for i in range(per):
        acc = (acc + owned[:, :, i]).astype(F32)
    return acc


def emulate(c, d, s64):
    x = (d['x'] if s64 is None else s64).astype(F32)
    N = F32(c.N)
    vec = 8 if c.expect != PC.K_LDS1 else 1
    g = d['gamma'].astype(F32)
    if not c.ln:
        ss = _block_sum(_per_thread((x * x).astype(F32), vec))
        inv = (F32(1.0) / np.sqrt((ss / N).astype(F32) + d['eps'], dtype=F32)).astype(F32)
        n16 = (x * inv[:, None]).astype(F32).astype(np.float16)
        return (n16.astype(F32) * g).astype(F32).astype(np.float16)
    mean = (_block_sum(_per_thread(x, vec)) / N).astype(F32)
    if c.diff_sq:
        var = ((_block_sum(_per_thread((x * x).astype(F32), vec)) / N).astype(F32) - (mean * mean).astype(F32)).astype(F32)
    else:
        dd = (x - mean[:, None]).astype(F32)
        var = (_block_sum(_per_thread((dd * dd).astype(F32), 1)) / N).astype(F32)
    inv = (F32(1.0) / np.sqrt(np.maximum(var, F32(0)) + d['eps'], dtype=F32)).astype(F32)
    y = ((((x - mean[:, None]).astype(F32) * inv[:, None]).astype(F32) * g).astype(F32) + d['beta'].astype(F32)).astype(F32)
    return y.astype(np.float16)


@pytest.mark.parametrize('c', RUN, ids=PC.rms_id)
def test_a_float32_emulation_of_the_kernel_stays_inside_every_cap(c):
    d, y, s = inputs(c)
    got = emulate(c, d, s)
    worst, differ = _assert_stage_a(got, y, 'y')
    print(f'[{PC.rms_id(c)}] emulated {PC.KERNEL_NAME[c.expect]}: worst {worst:.2f} ulp, {differ} of {got.size} differ')
    if s is not None:  # sum_out: the float32 add of two fp16 values rounded to fp16 is the single rounding
        s32 = (d['x'].astype(F32) + d['residual'].astype(F32)).astype(F32).astype(np.float16)
        assert np.array_equal(s32, s.astype(np.float16))
    # Stage B's caps: the float32 tail on the emulated y against the float64 oracle's scales (rtol 2^-22 on amax / 127 needs the
    # same amax: compare where the emulated row maximum is the oracle's)
    q, sc, amax = PO.quant_per_token_f32(got)
    _, sc64, amax64 = PO.quant_per_token(got)
    np.testing.assert_allclose(sc.astype(np.float64), sc64, rtol=2.0 ** -22)


def test_the_emulation_at_the_sizes_the_caps_were_set_with():
    """x ~ 1.7 N(0, 1), gamma in [0.5, 1.5], M = 3 at N in {8 .. 11008}: the record behind max(2, 1 %) at 2 ulp"""
    r = np.random.default_rng(20240)
    for n in (8, 64, 100, 257, 2040, 4096, 5120, 8200, 11008):
        c = PC.RCase('emu', n, expect=PC.rule(n))
        d = dict(x=(1.7 * r.standard_normal((3, n))).astype(np.float16), gamma=r.uniform(0.5, 1.5, n).astype(np.float16), eps=F32(1e-6))
        y, _ = PO.add_rmsnorm(d['x'], d['gamma'], 1e-6)
        _assert_stage_a(emulate(c, d, None), y, n)
