"""Every instance of the decode GEMV (kernels/gemv.hip launch_gemv: the skinny vector-ALU kernel of gemv_impl.h in every
(weight type, prologue, epilogue, row bucket, activation bucket) form, the K-split one-shot kernel, the matrix-pipe kernel and the
LDS slab split) through tllm_gemv against the float64 oracle (oracle/gemv_oracle.py), at the smallest shapes that reach the
instance - the case table is tests/gemv_cases.py, held against the dispatch by tests/test_gemv_instance_table.py.

Two stages, so that a rounding flip in the prologue does not blur the dot and the epilogue:
  A. x_pro_out against the oracle's x' (2 fp16 ulp / 1 LSB, 99 % identical), dyn_scale_out against amax / 127;
  B. y against the oracle fed with the kernel's own x_pro_out (x itself for the copy prologue): SmoothQuant bit-exact
     (SwiGLU: 2 ulp / 1 LSB - __expf is its only inexact step), fp16 / weight-only weights in fp16 ulps at the row's largest
     value (bounds next to each assert).
Every case: run twice (bit-identical), every buffer allocated for 8 rows with 0xFF sentinels (rows >= M, columns >= N, padding),
the residual unmodified; `inplace` cases once more with residual == y."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import gemv_cases as GC
from helpers import GemvParams
from oracle import gemv_oracle as GO
from oracle import llama_oracle as O
from oracle.quant_oracle import process_woq_layout
from tensorrt_llm.plugin import capi

pytestmark = pytest.mark.gpu

ROWS = 8  # every row-indexed buffer is allocated for 8 rows
_NP_OF = {GC.DT_FLOAT: np.float32, GC.DT_HALF: np.float16, GC.DT_INT8: np.int8, GC.DT_INT32: np.int32}


@pytest.fixture(scope='module')
def gemv(lib):
    lib.tllm_gemv.argtypes = [ctypes.POINTER(GemvParams), ctypes.c_void_p]
    lib.tllm_gemv.restype = ctypes.c_int32
    lib.tllm_gemv_set_mfma_rows.argtypes = [ctypes.c_int32]
    lib.tllm_gemv_set_mfma_rows.restype = None
    lib.tllm_gemv_set_blocks_per_cu.argtypes = [ctypes.c_int32]
    lib.tllm_gemv_set_blocks_per_cu.restype = None
    return lib


def _padded(a, ld, dtype=None):
    """[rows, n] -> [ROWS or rows, ld] bytes-0xFF-filled array holding `a` in its top-left corner"""
    a = np.ascontiguousarray(a, dtype=dtype)
    out = np.full((a.shape[0], ld * a.itemsize), 0xFF, np.uint8).view(a.dtype)
    out[:, :a.shape[1]] = a
    return out


def inputs(c):
    """numpy operands of a case, seeded by its id.  x ~ 1.7 N(0, 1) (dc: 3 + N(0, 1)), gamma in [0.5, 1.5], weights
    1.7 U(-1, 1) / sqrt(K) (SmoothQuant: random int8 with scales to match), so that the outputs are O(1)."""
    r = np.random.default_rng(zlib.crc32(GC.case_id(c).encode()))
    sq = c.wt == GC.W_INT8_SQ
    rows = 2 * c.N if GC.is_swiglu(c) else c.N
    ldx, ldy, ldw = GC.strides(c)
    d = dict(rows=rows, ldx=ldx, ldy=ldy, ldw=ldw)
    if sq and c.pro == GC.PRO_NONE:
        x = r.integers(-127, 128, (ROWS, c.K)).astype(np.int8)
    else:
        x = ((3.0 + r.standard_normal((ROWS, c.K))) if c.dc else 1.7 * r.standard_normal((ROWS, c.K))).astype(np.float16)
    d['x'] = x[:c.M]
    xb = _padded(x, ldx)
    xb[c.M:] = np.full((), 0xFF, np.uint8).view(np.int8) if x.dtype == np.int8 else np.float16(np.nan)  # rows >= M are never read
    d['x_buf'] = xb
    d['gamma'] = r.uniform(0.5, 1.5, c.K).astype(np.float16)
    if sq:
        w = r.integers(-127, 128, (rows, c.K)).astype(np.int8)
        full = np.zeros((rows, GC.row_bytes(c.wt, c.K)), np.int8)  # the layout pads a row with zeros up to Kp
        full[:, :c.K] = w
        d['w'], d['w_buf'] = w, _padded(full, ldw)
        # |acc| ~ sqrt(K) * 73 * 45 (s8 operands of rms 73 and ~45): column x row scales bring it to O(1)
        srow = (0.013 * (1.0 + 0.17 * np.arange(ROWS))).astype(np.float32)
        d['scale_row'] = srow[:c.M] if c.per_token else srow[:1]
        d['scale_row_buf'] = srow if c.per_token else srow[:1]
        sc = (r.uniform(0.5, 1.5, rows) / (np.sqrt(c.K) * 73 * 45 * 0.013)).astype(np.float32)
        d['scale_col'] = sc if c.per_channel else sc[:1]
        d['act_scale'] = np.float32(37.0 if GC.pro_kind(c.pro) == GC.PK_NORM else 21.0)
        d['epi_scale'] = np.float32(21.0)
    else:
        w = (1.7 * r.uniform(-1, 1, (rows, c.K)) / np.sqrt(c.K)).astype(np.float16)
        if c.wt == GC.W_FP16:
            d['w'], d['w_buf'] = w, _padded(w.view(np.uint8), ldw)
        else:
            bits = 8 if c.wt == GC.W_INT8_WOQ else 4
            q_kn, s = O.woq_quantize(w.T.astype(np.float32), bits)
            processed = process_woq_layout(q_kn, bits)
            if bits == 8 or rows % 2 == 0:  # the product's own host-side layout (it packs int4 columns in pairs)
                p2, s2, _ = capi.symmetric_quantize_last_axis(np.ascontiguousarray(w.T), bits)
                assert np.array_equal(p2, processed) and np.array_equal(s2.astype(np.float32), s)
            d['w'], d['w_buf'], d['scale_col'] = np.ascontiguousarray(q_kn.T), _padded(processed.view(np.uint8), ldw), s.astype(np.float16)
    if c.strided and c.wt != GC.W_FP16:
        # the Kp - K tail of a row too (K is a multiple of 8: whole bytes of either integer width); it faces zeroed activations
        d['w_buf'].view(np.uint8)[:, (c.K if c.wt != GC.W_INT4_WOQ else c.K // 2):] = 0xFF
    res = r.standard_normal((ROWS, c.N)).astype(np.float16)
    d['residual'], d['residual_buf'] = res[:c.M], _padded(res, ldy)
    return d


class Device:
    """the operands of a case on the GPU; launch() returns (rc, y, x_pro_out, dyn_scale_out) as numpy arrays of the WHOLE
    buffers (8 rows, padding included)"""

    def __init__(self, c, d):
        self.c, self.d = c, d
        cu = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
        self.x, self.w, self.gamma = cu(d['x_buf']), cu(d['w_buf']), cu(d['gamma'])
        self.res = cu(d['residual_buf'])
        self.scale_col = cu(d['scale_col']) if 'scale_col' in d else None
        self.scale_row = cu(d['scale_row_buf']) if 'scale_row_buf' in d else None
        self.act = cu(np.array([d['act_scale']], np.float32)) if 'act_scale' in d else None
        self.epi_q = cu(np.array([d['epi_scale']], np.float32)) if 'epi_scale' in d else None

    def launch(self, lib, side, inplace=False, mfma_rows=None):
        c, d = self.c, self.d
        sq = c.wt == GC.W_INT8_SQ
        odt = GC.out_dtype(c)
        ysz = np.dtype(_NP_OF[odt]).itemsize
        y = torch.full((ROWS * d['ldy'] * ysz, ), 0xFF, dtype=torch.uint8, device='cuda')
        if inplace:
            y.copy_(self.res)
        xpro = torch.full((ROWS * c.K * (1 if sq else 2), ), 0xFF, dtype=torch.uint8, device='cuda')
        dyn = torch.full((ROWS * 4, ), 0xFF, dtype=torch.uint8, device='cuda')
        ptr = lambda t: t.data_ptr() if t is not None else None
        q = GemvParams(c.wt, c.pro, c.epi, odt, c.M, c.N, c.K, self.x.data_ptr(), d['ldx'], self.w.data_ptr(), d['ldw'],
                       ptr(self.scale_col), ptr(self.scale_row), c.per_channel, c.per_token,
                       self.gamma.data_ptr() if GC.pro_kind(c.pro) == GC.PK_NORM else None, 1e-6,
                       ptr(self.act) if c.pro in (GC.PRO_RMSNORM_QSTATIC, GC.PRO_QSTATIC) else None,
                       dyn.data_ptr() if side else None, xpro.data_ptr() if side else None,
                       (y.data_ptr() if inplace else self.res.data_ptr()) if c.epi == GC.EPI_RESIDUAL else None,
                       ptr(self.epi_q) if c.epi == GC.EPI_SWIGLU_QSTATIC else None, y.data_ptr(), d['ldy'])
        try:
            lib.tllm_gemv_set_mfma_rows(c.mfma_rows if mfma_rows is None else mfma_rows)
            lib.tllm_gemv_set_blocks_per_cu(c.blocks_per_cu)
            rc = lib.tllm_gemv(ctypes.byref(q), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        finally:
            lib.tllm_gemv_set_mfma_rows(-1)
            lib.tllm_gemv_set_blocks_per_cu(0)
        return (rc, y.cpu().numpy().view(_NP_OF[odt]).reshape(ROWS, d['ldy']),
                xpro.cpu().numpy().view(np.int8 if sq else np.float16).reshape(ROWS, c.K), dyn.cpu().numpy().view(np.float32))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _untouched(a):
    return bool((_bits(a) == 0xFF).all())


def _ord16(a):
    """fp16 values -> integers whose difference counts representable values in between"""
    b = np.asarray(a, dtype=np.float16).view(np.int16).astype(np.int32)
    return np.where(b < 0, -(b & 0x7FFF), b)


def stage_a(c, d, xpro, dyn, tag):
    """the prologue's side outputs against the oracle's x'"""
    ref = GO.prologue(d['x'], c.pro, d['gamma'], 1e-6, d.get('act_scale'))
    got = xpro[:c.M]
    if c.wt == GC.W_INT8_SQ:
        diff = np.abs(got.astype(np.int32) - ref['xp'].astype(np.int32))
        unit, lim = 'LSB', 1
    else:
        diff = np.abs(_ord16(got) - _ord16(ref['xp']))
        unit, lim = 'fp16 ulp', 2
    same = float((diff == 0).mean())
    print(f'{tag} A: x_pro_out worst {diff.max()} {unit}, {100 * same:.3f} % identical')
    assert diff.max() <= lim and same >= 0.99, (diff.max(), same)
    assert _untouched(xpro[c.M:]), 'x_pro_out rows >= M written'
    if c.pro in (GC.PRO_RMSNORM_QDYN, GC.PRO_QDYN):
        # dyn_scale_out[m] = float32(a / 127) to 1 fp32 ulp for an fp16 a within 2 fp16 ulp of the oracle's amax
        for m in range(c.M):
            a0 = np.float16(ref['amax'][m])
            cands = [a0]
            for step_to in (np.float16(np.inf), np.float16(0)):
                a = a0
                for _ in range(2):
                    a = np.nextafter(a, step_to)
                    cands.append(a)
            want = [np.float32(np.float64(a) / 127.0) for a in cands]
            err = min(abs(np.float64(dyn[m]) - np.float64(w)) / np.float64(np.spacing(w)) for w in want)
            assert err <= 1.0, (m, dyn[m], ref['amax'][m] / 127.0)
        assert _untouched(dyn[c.M:]), 'dyn_scale_out rows >= M written'
    else:
        assert _untouched(dyn), 'dyn_scale_out written without a per-token quantiser'


def stage_b(c, d, y, xp, row_scale, tag):
    """y against the oracle's dot + epilogue on the prologue result `xp`; returns the worst error in the case's unit"""
    sq = c.wt == GC.W_INT8_SQ
    odt = GC.out_dtype(c)
    got = y[:c.M, :c.N]
    ref = GO.gemv(xp, d['w'], c.wt, c.epi, odt, d.get('scale_col'), row_scale, d['residual'], d.get('epi_scale'))
    v = ref['v']
    if sq and not GC.is_swiglu(c):
        want = ref['y'].astype(_NP_OF[odt])
        bad = int((_bits(got) != _bits(want)).reshape(c.M, c.N, -1).any(-1).sum())
        print(f'{tag} B: SmoothQuant {GC.EPI_NAME[c.epi]} -> {GC.DT_NAME[odt]}: {bad} of {got.size} outputs differ (must be bit-exact)')
        assert bad == 0
        return 0.0
    if sq:
        if odt == GC.DT_INT8:
            diff, unit, lim, frac = np.abs(got.astype(np.int32) - ref['y'].astype(np.int32)), 'LSB', 1, 0.98
        else:
            diff, unit, lim, frac = np.abs(_ord16(got) - _ord16(ref['y'])), 'fp16 ulp', 2, 0.99
        same = float((diff == 0).mean())
        print(f'{tag} B: SmoothQuant SwiGLU worst {diff.max()} {unit}, {100 * same:.3f} % identical')
        assert diff.max() <= lim and same >= frac, (diff.max(), same)
        return float(diff.max())
    g64 = got.astype(np.float64)
    rowmax = lambda a: np.abs(a).max(axis=1, keepdims=True)
    if GC.is_swiglu(c):
        # first-order propagation of 1 ulp on gate and up (silu' <= 1.1) + the epilogue's own fp16 roundings
        g, u = v, ref['u']
        silu = g / (1.0 + np.exp(-g))
        exact = silu * u
        bound = 1.1 * np.abs(u) * GO.ulp16(rowmax(g)) + np.abs(silu) * GO.ulp16(rowmax(u)) + 2.0 * GO.ulp16(exact)
        unit = 'of the SwiGLU bound'
    elif c.epi == GC.EPI_RESIDUAL:
        exact = v + d['residual'].astype(np.float64)
        bound = 1.0 * GO.ulp16(rowmax(v)) + 0.5 * GO.ulp16(rowmax(exact)) + 0 * exact
        unit = 'of 1 ulp(max |v|) + 0.5 ulp(max |y|)'
    else:
        exact = v
        bound = (1.0 if odt == GC.DT_HALF else 0.5) * GO.ulp16(rowmax(v)) + 0 * exact
        unit = f'of {1.0 if odt == GC.DT_HALF else 0.5} fp16 ulp(max |y| of the row)'
    assert np.isfinite(g64).all(), f'{int((~np.isfinite(g64)).sum())} non-finite outputs'
    worst = float((np.abs(g64 - exact) / bound).max())
    print(f'{tag} B: worst error {worst:.3f} {unit}; max |y| = {np.abs(exact).max():.2f}')
    assert worst <= 1.0, worst
    return worst


@pytest.mark.parametrize('c', GC.CASES, ids=GC.case_id)
def test_gemv_instance_against_the_float64_oracle(c, gemv):
    tag = f'[{GC.case_id(c)}]'
    inst = GC.instance(c)
    d = inputs(c)
    dev = Device(c, d)
    side = GC.has_side(c)
    rc, y, xpro, dyn = dev.launch(gemv, side)
    if inst[0] == 'refused':
        assert rc != 0, f'{tag} expected a refusal ({inst[1]})'
        assert _untouched(y) and _untouched(xpro) and _untouched(dyn)
        print(f'{tag} refused: {capi.last_error()}')
        return
    assert rc == 0, capi.last_error()
    print(f'{tag} instance {inst}')
    # ---- determinism
    rc2, y2, xpro2, dyn2 = dev.launch(gemv, side)
    assert rc2 == 0
    assert np.array_equal(_bits(y), _bits(y2)) and np.array_equal(_bits(xpro), _bits(xpro2)) and np.array_equal(_bits(dyn), _bits(dyn2)), \
        'two runs differ'
    # ---- sentinels: rows >= M, columns >= N; the operands as they were
    assert _untouched(y[c.M:]), 'y rows >= M written'
    assert _untouched(y[:, c.N:]), 'y columns >= N written'
    assert np.array_equal(dev.res.cpu().numpy(), _bits(d['residual_buf']).reshape(-1)), 'the residual was modified'
    assert np.array_equal(dev.x.cpu().numpy(), _bits(d['x_buf']).reshape(-1)), 'x was modified'
    # ---- stage A
    row_scale = d.get('scale_row')
    if c.pro == GC.PRO_NONE:
        xp = d['x']
        assert _untouched(xpro) and _untouched(dyn), 'side outputs written by the copy prologue'
    else:
        if side:
            xa, da = xpro, dyn
        else:
            # no side outputs in this call (the matrix pipe does not write them): x' from the vector-ALU kernel on the same
            # operands - the matrix-pipe kernel states the same prologue, stage B holds it to that
            assert _untouched(xpro) and _untouched(dyn)
            rca, _, xa, da = dev.launch(gemv, True, mfma_rows=0)
            assert rca == 0, capi.last_error()
        stage_a(c, d, xa, da, tag)
        xp = xa[:c.M]
        if c.pro in (GC.PRO_RMSNORM_QDYN, GC.PRO_QDYN):
            row_scale = da[:c.M]
    # ---- stage B
    stage_b(c, d, y, xp, row_scale, tag)
    # ---- residual == y (the session's own usage)
    if c.inplace:
        assert c.epi == GC.EPI_RESIDUAL
        rci, yi, _, _ = dev.launch(gemv, side, inplace=True)
        assert rci == 0, capi.last_error()
        assert np.array_equal(_bits(yi[:c.M, :c.N]), _bits(y[:c.M, :c.N])), 'in-place residual differs from the out-of-place run'
        assert np.array_equal(_bits(yi[c.M:, :c.N]), _bits(d['residual_buf'][c.M:, :c.N])), 'in place: rows >= M written'
        assert _untouched(yi[:, c.N:]), 'in place: y columns >= N written'
