"""Every kernel of kernels/pointwise.hip through its flat entry (tllm_rmsnorm with the kernel forced or chosen, tllm_swiglu,
tllm_swiglu_quant, tllm_add, tllm_quantize_tensor, tllm_embedding, the gathers, the scan, the fills) against the float64 oracle
(oracle/pointwise_oracle.py) at the smallest shapes that reach the kernel, the partly filled last vector, the scalar forms and
the second trip of the grid-stride loops - the case table is tests/pointwise_cases.py, held against the dispatch by
tests/test_pointwise_instance_table.py.

RMSNorm / LayerNorm in two stages, so that a rounding flip in the norm does not blur the quantiser:
  A. y against the oracle: 2 fp16 ulp at the oracle's value, at most max(2, 1 %) of the elements differing; sum_out bit-exact;
  B. q and dyn_scale_out against the float32 restatement of the tail fed with the kernel's own y: bit-exact (each step of the
     tail is a single IEEE operation); dyn_scale_out against the float64 amax / 127 of that y: rtol 2^-22.
Every launch: run twice (bit-identical), every output buffer with an extra row and 64 bytes of 0xFF in front and behind, the
inputs read back unmodified."""
import ctypes

import numpy as np
import pytest
import torch

import pointwise_cases as PC
from helpers import RmsnormParams
from oracle import pointwise_oracle as PO
from tensorrt_llm.plugin import capi

pytestmark = pytest.mark.gpu
PAD = 64
_vp, _i32, _i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64


@pytest.fixture(scope='module')
def pw(lib):
    sig = dict(tllm_rmsnorm=[ctypes.POINTER(RmsnormParams), _i32, _vp], tllm_rmsnorm_kernel=[ctypes.POINTER(RmsnormParams)],
               tllm_swiglu=[_vp, _vp, _vp, _i64, _vp], tllm_swiglu_quant=[_vp, _vp, _vp, _i64, _vp, _vp],
               tllm_add=[_vp, _vp, _vp, _i64, _vp], tllm_quantize_tensor=[_vp, _vp, _i32, _i64, _vp, _vp],
               tllm_quantize_per_token=[_vp, _vp, _i32, _i64, _i64, _vp, _vp], tllm_embedding=[_vp, _vp, _vp, _i64, _i32, _i32, _vp],
               tllm_gather_last_token=[_vp, _vp, _vp, _i32, _i32, _i32, _vp], tllm_gather_rows=[_vp, _vp, _vp, _i32, _i32, _vp],
               tllm_exclusive_scan_i32=[_vp, _vp, _i32, _vp], tllm_fill_i32=[_vp, _i32, _i64, _vp],
               tllm_fill_random=[_vp, _i32, _i64, ctypes.c_uint32, ctypes.c_float, _vp])
    for name, args in sig.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = _i32
    return lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Buf:
    """a device buffer | 64 x 0xFF | off x 0xFF | payload | 64 x 0xFF |: `data` (any numpy array) is the payload, or nbytes of
    0xFF (an output).  ptr is the payload's address: 16-byte aligned + off."""

    def __init__(self, data=None, nbytes=0, off=0):
        raw = np.ascontiguousarray(data).view(np.uint8).reshape(-1) if data is not None else np.full(nbytes, 0xFF, np.uint8)
        self.off, self.n = off, raw.size
        self.host = np.full(PAD + off + raw.size + PAD, 0xFF, np.uint8)
        self.host[PAD + off:PAD + off + raw.size] = raw
        self.t = torch.from_numpy(self.host.copy()).cuda()
        self.ptr = self.t.data_ptr() + PAD + off
        assert self.t.data_ptr() % 256 == 0

    def read(self, dtype=np.uint8):
        """(payload as dtype, guards intact)"""
        b = self.t.cpu().numpy()
        lo = PAD + self.off
        return b[lo:lo + self.n].copy().view(dtype), bool((b[:lo] == 0xFF).all() and (b[lo + self.n:] == 0xFF).all())

    def unchanged(self):
        return np.array_equal(self.t.cpu().numpy(), self.host)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _all_ff(a):
    return bool((_bits(a) == 0xFF).all())


# ---------------------------------------------------------------------------------------------- RMSNorm / LayerNorm
_rms_memo = {}


def rms_data(c):
    """operands and the float64 reference of a case: computed once, shared, never modified"""
    k = PC.rms_id(c)
    if k not in _rms_memo:
        d = PC.rms_inputs(c)
        y, s = PO.norm(d['x'], d['gamma'], d['eps'], d['residual'] if c.residual else None, d['beta'], bool(c.ln), bool(c.diff_sq))
        d['y_ref'], d['sum_ref'] = y, s
        _rms_memo[k] = d
    return _rms_memo[k]


def run_rms(lib, c, d, out, kernel=None):
    """one launch of case `c` asking for the outputs `out`; returns dict(rc, y, q, dyn, sum): the WHOLE payloads (M + 1 rows) as
    numpy, after checking the guards and that the inputs read back unmodified"""
    M, N, rows = c.M, c.N, max(c.M, 0) + 1

    def spare_row(a):  # fp16 [M, N] -> M + 1 rows, the last one 0xFF bytes (NaN): never read
        full = np.full((rows, N), 0xFFFF, np.uint16).view(np.float16)
        full[:rows - 1] = a[:rows - 1]
        return full

    x = Buf(spare_row(d['x']), off=2 * c.x_off)
    gamma, beta = Buf(d['gamma']), Buf(d['beta'])
    res = Buf(spare_row(d['residual']))
    scale = Buf(np.array([d['scale']], np.float32))
    y, so = Buf(nbytes=rows * N * 2), Buf(nbytes=rows * N * 2)
    q, dyn = Buf(nbytes=rows * N, off=c.q_off), Buf(nbytes=rows * 4)
    p = RmsnormParams()
    p.M, p.N, p.eps = M, N, float(d['eps'])
    p.x, p.gamma = x.ptr, gamma.ptr
    if c.residual:
        p.residual = res.ptr
        p.sum_out = None if c.drop == 'sum_out' else so.ptr
    if 'y' in out:
        p.y = y.ptr
    if 'q' in out:
        p.q = q.ptr
        if c.drop != 'scale':
            if out.endswith('s'):
                p.static_scale = scale.ptr
            else:
                p.dyn_scale_out = dyn.ptr
    p.layernorm, p.use_diff_of_squares = c.ln, c.diff_sq
    if c.ln and c.drop != 'beta':
        p.beta = beta.ptr
    rc = lib.tllm_rmsnorm(ctypes.byref(p), c.kernel if kernel is None else kernel, _stream())
    torch.cuda.synchronize()
    r = dict(rc=rc, chosen=lib.tllm_rmsnorm_kernel(ctypes.byref(p)))  # the launcher's own choice on these very pointers
    for name, b, dt in (('y', y, np.float16), ('sum', so, np.float16), ('q', q, np.int8), ('dyn', dyn, np.float32)):
        a, ok = b.read(dt)
        assert ok, f'{name}: bytes around the buffer were written'
        r[name] = a.reshape(rows, -1) if name != 'dyn' else a
    for name, b in (('x', x), ('gamma', gamma), ('beta', beta), ('residual', res), ('static_scale', scale)):
        assert b.unchanged(), f'{name} was modified'
    return r


def _same(r1, r2):
    return all(np.array_equal(_bits(r1[k]), _bits(r2[k])) for k in ('y', 'sum', 'q', 'dyn')) and r1['rc'] == r2['rc']


def check_rms(lib, c, d, out, tag):
    M = c.M
    r = run_rms(lib, c, d, out)
    assert _same(r, run_rms(lib, c, d, out)), 'two runs differ'
    if c.kernel == 0:
        assert r['chosen'] == c.expect, f'the launcher picks {PC.KERNEL_NAME.get(r["chosen"])}, the case names {PC.KERNEL_NAME[c.expect]}'
    if c.expect <= 0:
        assert r['rc'] == (0 if c.expect == 0 else -1), (r['rc'], capi.last_error())
        if c.expect < 0:
            assert capi.last_error(), 'a refusal without an error string'
            print(f'{tag} refused: {capi.last_error()}')
        assert all(_all_ff(r[k]) for k in ('y', 'sum', 'q', 'dyn')), 'a refused / empty call wrote to a buffer'
        return
    assert r['rc'] == 0, capi.last_error()
    # ---- what was not asked for stays untouched; rows >= M of what was
    for k, asked in (('y', 'y' in out), ('sum', bool(c.residual)), ('q', 'q' in out)):
        assert _all_ff(r[k][M:] if asked else r[k]), f'{k}: {"rows >= M" if asked else "not requested but"} written'
    assert _all_ff(r['dyn'][M:] if out.endswith('qd') else r['dyn']), 'dyn_scale_out written where it should not be'
    # ---- stage A
    if c.residual:
        assert np.array_equal(_bits(r['sum'][:M]), _bits(d['sum_ref'].astype(np.float16))), 'sum_out is not f16(x + residual)'
    if 'y' in out:
        worst, differ, cap = PC.within_ulp16(r['y'][:M], d['y_ref'])
        print(f'{tag} A: y worst {worst:.2f} fp16 ulp, {differ} of {r["y"][:M].size} differ (cap {cap})')
        assert worst <= 2.0 and differ <= cap, (worst, differ, cap)
    if 'q' not in out:
        return
    # ---- stage B: the tail on the kernel's own y
    if 'y' in out:
        yk = r['y'][:M]
    else:
        both = run_rms(lib, c, d, 'y' + out)
        assert both['rc'] == 0, capi.last_error()
        yk = both['y'][:M]
        assert np.array_equal(r['q'][:M], both['q'][:M]), 'q alone differs from the q of the y + q call'
        assert np.array_equal(_bits(r['dyn']), _bits(both['dyn'])), 'dyn_scale_out alone differs from that of the y + q call'
    dev_y, dev_q, dev_s, dev_scale = Buf(yk), Buf(nbytes=yk.size), Buf(nbytes=M * 4), Buf(np.array([d['scale']], np.float32))
    if out.endswith('s'):
        want = PO.quant_static_f32(yk, d['scale'])
        bad = int((r['q'][:M] != want).sum())
        print(f'{tag} B: static q: {bad} of {want.size} differ from the float32 restatement (must be bit-exact)')
        assert bad == 0
        assert lib.tllm_quantize_tensor(dev_q.ptr, dev_y.ptr, PC.DT_HALF, yk.size, dev_scale.ptr, _stream()) == 0, capi.last_error()
        torch.cuda.synchronize()
        assert np.array_equal(dev_q.read(np.int8)[0].reshape(M, -1), r['q'][:M]), 'q static != QuantizeTensor(y)'
    else:
        want, ws, _ = PO.quant_per_token_f32(yk)
        bad = int((r['q'][:M] != want).sum())
        sbad = int((_bits(r['dyn'][:M]) != _bits(ws)).reshape(M, 4).any(-1).sum())
        print(f'{tag} B: dynamic q: {bad} of {want.size} and {sbad} of {M} scales differ from the float32 restatement (must be bit-exact)')
        assert bad == 0 and sbad == 0
        _, s64, _ = PO.quant_per_token(yk)
        np.testing.assert_allclose(r['dyn'][:M].astype(np.float64), s64, rtol=2.0 ** -22, atol=0)
        assert lib.tllm_quantize_per_token(dev_q.ptr, dev_y.ptr, PC.DT_HALF, M, c.N, dev_s.ptr, _stream()) == 0, capi.last_error()
        torch.cuda.synchronize()
        assert np.array_equal(dev_q.read(np.int8)[0].reshape(M, -1), r['q'][:M]), 'q dynamic != QuantizePerToken(y)'
        assert np.array_equal(_bits(dev_s.read(np.float32)[0]), _bits(r['dyn'][:M])), 'dynamic scales != QuantizePerToken(y)'
    assert dev_q.read()[1] and dev_s.read()[1] and dev_y.unchanged()


@pytest.mark.parametrize('c', PC.RMS_CASES, ids=PC.rms_id)
def test_rmsnorm_instance_against_the_float64_oracle(c, pw):
    d = rms_data(c)
    for out in c.outs:
        check_rms(pw, c, d, out, f'[{PC.rms_id(c)} {out} {PC.KERNEL_NAME[c.expect]}]')


REG_ROWS = [c for c in PC.RMS_CASES if c.kernel == 0 and c.expect in (PC.REG1, PC.REG2, PC.REG4)]


@pytest.mark.parametrize('c', REG_ROWS, ids=PC.rms_id)
def test_the_register_kernel_and_the_lds_kernel_are_bit_identical(c, pw):
    """the claim in the comment above rmsnorm_reg_kernel: same arithmetic in the same order as rmsnorm_kernel<8>"""
    d = rms_data(c)
    for out in ('yqs', 'yqd'):
        a, b = run_rms(pw, c, d, out, kernel=PC.K_REG), run_rms(pw, c, d, out, kernel=PC.K_LDS8)
        assert a['rc'] == 0 and b['rc'] == 0, capi.last_error()
        for k in ('y', 'q', 'dyn', 'sum'):
            n = int((_bits(a[k]) != _bits(b[k])).sum())
            assert n == 0, f'{k}: {n} bytes differ between rmsnorm_reg_kernel and rmsnorm_kernel<8> ({out}, N = {c.N})'


# ---------------------------------------------------------------------------------------------- swiglu, swiglu_quant, add
EW_SCALE = np.float32(21.0)
_ew_memo = {}


def ew_data(op, n):
    k = (op, n)
    if k not in _ew_memo:
        a, b = PC.ew_inputs(n, PC.crc(f'ew-{n}'))
        ref = {'swiglu': PO.swiglu, 'add': PO.add}[op](a, b) if op != 'swiglu_quant' else PO.swiglu_quant(a, b, EW_SCALE)
        _ew_memo[k] = (a, b, ref)
    return _ew_memo[k]


def run_ew(lib, op, a, b, off='', inplace=0):
    """returns the output payload (fp16, or int8 for swiglu_quant); guards and inputs checked"""
    n = a.size
    quant = op == 'swiglu_quant'
    A, B = Buf(a, off=2 if off == 'a' else 0), Buf(b, off=2 if off == 'b' else 0)
    Y = A if inplace else Buf(nbytes=n * (1 if quant else 2), off=(4 if quant else 2) if off == 'y' else 0)
    S = Buf(np.array([EW_SCALE], np.float32))
    if quant:
        rc = lib.tllm_swiglu_quant(Y.ptr, A.ptr, B.ptr, n, S.ptr, _stream())
    else:
        rc = getattr(lib, 'tllm_' + op)(Y.ptr, A.ptr, B.ptr, n, _stream())
    torch.cuda.synchronize()
    assert rc == 0, capi.last_error()
    y, ok = Y.read(np.int8 if quant else np.float16)
    assert ok, 'bytes around the output were written'
    assert (inplace or A.unchanged()) and B.unchanged() and S.unchanged(), 'an input was modified'
    return y


def _nan_pins(n):
    return [i for i in (7, 15) if i < n]


@pytest.mark.parametrize('c', PC.EW_CASES, ids=PC.ew_id)
def test_elementwise_instance_against_the_float64_oracle(c, pw):
    a, b, ref = ew_data(c.op, c.n)
    tag = f'[{PC.ew_id(c)} VEC={PC.ew_vec(c)}]'
    y = run_ew(pw, c.op, a, b, c.off, c.inplace)
    assert np.array_equal(_bits(y), _bits(run_ew(pw, c.op, a, b, c.off, c.inplace))), 'two runs differ'
    if c.op == 'add':
        want = ref.astype(np.float16)
        # bit for bit, the sign of zero and the infinities included (a NaN's payload is not compared: NaN in -> NaN out)
        bad = int(((y.view(np.uint16) != want.view(np.uint16)) & ~(np.isnan(want) & np.isnan(y))).sum())
        print(f'{tag} add: {bad} of {c.n} differ from f16(a + b) (must be bit-exact)')
        assert bad == 0
    elif c.op == 'swiglu':
        worst, differ, cap = PC.within_ulp16(y, ref)
        print(f'{tag} swiglu: worst {worst:.2f} fp16 ulp, {differ} of {c.n} differ (cap {cap})')
        assert worst <= 2.0 and differ <= cap, (worst, differ, cap)
        # the pinned elements are exact: g = +-0 -> 0, g = -65504 -> -0 or 0, NaN in -> NaN out
        for i in (0, 1, 3, 8, 9, 11):
            if i < c.n:
                assert y[i] == 0, (i, y[i])
        assert all(np.isnan(y[i]) for i in _nan_pins(c.n))
    else:
        dq = np.abs(y.astype(np.int32) - ref.astype(np.int32))
        differ, cap = int((dq != 0).sum()), max(2, c.n // 100)
        print(f'{tag} swiglu_quant: worst {dq.max()} LSB, {differ} of {c.n} differ (cap {cap})')
        assert dq.max() <= 1 and differ <= cap
        assert all(y[i] == 0 for i in _nan_pins(c.n)), 'NaN must quantise to 0'
        # == quantize_tensor(swiglu(a, b), s), bit for bit
        h = run_ew(pw, 'swiglu', a, b)
        H, Q, S = Buf(h), Buf(nbytes=c.n), Buf(np.array([EW_SCALE], np.float32))
        assert pw.tllm_quantize_tensor(Q.ptr, H.ptr, PC.DT_HALF, c.n, S.ptr, _stream()) == 0, capi.last_error()
        torch.cuda.synchronize()
        assert np.array_equal(Q.read(np.int8)[0], y), 'swiglu_quant != quantize_tensor(swiglu)'
        assert np.array_equal(y, PO.quant_static_f32(h, EW_SCALE)), 'swiglu_quant != the float32 restatement on the kernel\'s swiglu'
    if c.off or c.inplace:
        # the scalar form (a pointer off 16 bytes) / the in-place call against the aligned out-of-place one: the same bits
        assert np.array_equal(_bits(y), _bits(run_ew(pw, c.op, a, b))), 'VEC = 1 / in place differs from the aligned VEC = 8 run'


# ---------------------------------------------------------------------------------------------- quantize_tensor
@pytest.mark.parametrize('dtype', ['float16', 'float32'])
def test_quantize_tensor_second_grid_stride_trip(dtype, pw):
    n = PC.QT_N
    r = np.random.default_rng(PC.crc(f'qt-{dtype}'))
    x = (50.0 * r.standard_normal(n)).astype(np.float32)
    x[:12] = [0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 127.5, -128.5, 200, -200, 126.5, np.nan]
    x = x.astype(dtype)
    for scale in (np.float32(1.0), np.float32(0.37)):
        X, Q, S = Buf(x), Buf(nbytes=n), Buf(np.array([scale], np.float32))
        outs = []
        for _ in range(2):
            assert pw.tllm_quantize_tensor(Q.ptr, X.ptr, PC.DT_HALF if dtype == 'float16' else PC.DT_FLOAT, n, S.ptr, _stream()) == 0
            torch.cuda.synchronize()
            q, ok = Q.read(np.int8)
            assert ok and X.unchanged() and S.unchanged()
            outs.append(q)
        assert np.array_equal(outs[0], outs[1])
        assert np.array_equal(outs[0], PO.quant_static_f32(x, scale))


# ---------------------------------------------------------------------------------------------- embedding and the gathers
@pytest.mark.parametrize('tokens,hidden,vocab,off', PC.EMB_CASES)
def test_embedding(tokens, hidden, vocab, off, pw):
    r = np.random.default_rng(PC.crc(f'emb-{tokens}-{hidden}-{vocab}'))
    table = r.standard_normal((vocab, hidden)).astype(np.float16)
    ids = PC.emb_ids(tokens, vocab)
    T, I, Y = Buf(table, off=2 * off), Buf(ids), Buf(nbytes=(tokens + 1) * hidden * 2)
    outs = []
    for _ in range(2):
        assert pw.tllm_embedding(Y.ptr, I.ptr, T.ptr, tokens, hidden, vocab, _stream()) == 0, capi.last_error()
        torch.cuda.synchronize()
        y, ok = Y.read(np.float16)
        assert ok and T.unchanged() and I.unchanged()
        outs.append(y.reshape(tokens + 1, hidden))
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
    assert _all_ff(outs[0][tokens:]), 'row >= tokens written'
    assert np.array_equal(_bits(outs[0][:tokens]), _bits(PO.embedding(ids, table)))


@pytest.mark.parametrize('batch,seq,hs', PC.GLT_CASES)
def test_gather_last_token(batch, seq, hs, pw):
    r = np.random.default_rng(PC.crc(f'glt-{batch}-{seq}-{hs}'))
    hid = r.standard_normal((batch, seq, hs)).astype(np.float16)
    ids = PC.glt_ids(batch, seq, hs)
    H, I, Y = Buf(hid), Buf(ids), Buf(nbytes=(batch + 1) * hs * 2)
    outs = []
    for _ in range(2):
        assert pw.tllm_gather_last_token(Y.ptr, H.ptr, I.ptr, batch, seq, hs, _stream()) == 0, capi.last_error()
        torch.cuda.synchronize()
        y, ok = Y.read(np.float16)
        assert ok and H.unchanged() and I.unchanged()
        outs.append(y.reshape(batch + 1, hs))
    assert np.array_equal(_bits(outs[0]), _bits(outs[1])) and _all_ff(outs[0][batch:])
    assert np.array_equal(_bits(outs[0][:batch]), _bits(PO.gather_last_token(hid, ids)))


@pytest.mark.parametrize('hs', PC.GR_CASES)
def test_gather_rows(hs, pw):
    r = np.random.default_rng(PC.crc(f'gr-{hs}'))
    hid = r.standard_normal((6, hs)).astype(np.float16)
    rows, batch = PC.GR_ROWS, len(PC.GR_ROWS)
    H, I, Y = Buf(hid), Buf(rows), Buf(nbytes=(batch + 1) * hs * 2)
    outs = []
    for _ in range(2):
        assert pw.tllm_gather_rows(Y.ptr, H.ptr, I.ptr, batch, hs, _stream()) == 0, capi.last_error()
        torch.cuda.synchronize()
        y, ok = Y.read(np.float16)
        assert ok and H.unchanged() and I.unchanged()
        outs.append(y.reshape(batch + 1, hs))
    assert np.array_equal(_bits(outs[0]), _bits(outs[1])) and _all_ff(outs[0][batch:])
    assert np.array_equal(_bits(outs[0][:batch]), _bits(PO.gather_rows(hid, rows)))


# ---------------------------------------------------------------------------------------------- the scan and the fills
@pytest.mark.parametrize('n', PC.SCAN_N)
def test_exclusive_scan_i32(n, pw):
    lens = np.random.default_rng(PC.crc(f'scan-{n}')).integers(0, 2049, n).astype(np.int32)
    L, C = Buf(lens), Buf(nbytes=(n + 1) * 4)
    outs = []
    for _ in range(2):
        assert pw.tllm_exclusive_scan_i32(C.ptr, L.ptr, n, _stream()) == 0, capi.last_error()
        torch.cuda.synchronize()
        cu, ok = C.read(np.int32)
        assert ok and L.unchanged()
        outs.append(cu)
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], PO.exclusive_scan(lens))


def test_fill_i32_second_grid_stride_trip(pw):
    n = PC.QT_N
    D = Buf(nbytes=n * 4)
    for v in (-7, 0x01020304):
        assert pw.tllm_fill_i32(D.ptr, v, n, _stream()) == 0, capi.last_error()
        torch.cuda.synchronize()
        d, ok = D.read(np.int32)
        assert ok and (d == v).all()


@pytest.mark.parametrize('dtype', PC.FILL_DTYPES)
def test_fill_random_is_the_oracle_bit_for_bit(dtype, pw):
    n = PC.QT_N
    np_dt = {PC.DT_HALF: np.float16, PC.DT_FLOAT: np.float32, PC.DT_INT8: np.int8, PC.DT_FP8: np.uint8}[dtype]
    D = Buf(nbytes=n * np.dtype(np_dt).itemsize)
    outs = []
    for _ in range(2):
        assert pw.tllm_fill_random(D.ptr, dtype, n, 1234567, 0.75, _stream()) == 0, capi.last_error()
        torch.cuda.synchronize()
        d, ok = D.read(np_dt)
        assert ok
        outs.append(d)
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
    bad = int((_bits(outs[0]) != _bits(PO.fill_random(dtype, n, 1234567, 0.75))).sum())
    assert bad == 0, f'{bad} bytes differ from the oracle'
    if dtype == PC.DT_FP8:
        assert not np.isin(outs[0], [0x7f, 0xff]).any() and ((outs[0] & 0x7f) <= 0x3f).all()
