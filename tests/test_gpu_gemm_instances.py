"""Every kernel id of the prefill GEMMs (kernels/gemm_glds.hip, gemm_sqp.hip, gemm_woq.hip, gemm_mfma.hip, the GEMV slabs) and
every branch of launch_gemm's fall-back chain against the float64 oracle (oracle/gemm_oracle.py), at the smallest shapes that
reach the edge - the case table is tests/gemm_cases.py, held against the host code by tests/test_gemm_instance_table.py.

The kernel is chosen through tllm_gemm_kernel (exactly this kernel or a refusal), so a case cannot pass on another kernel's
result; where the mirror (evaluated at this device's CU count) predicts a refusal, the return code 1 and an untouched c are
asserted.  Every case: operands in padded buffers whose every byte outside the problem is 0xFF (NaN in fp16, -1 in int8): PAD
rows beyond M / N, and lda / ldw / ldc beyond the row where the case says so; c pre-filled with 0xFF; run twice (bit-identical);
rows >= M and columns >= N of c untouched; operands, residual and gate unmodified; `inplace` cases once more with residual == c.

Bounds.  SmoothQuant (all but the dual form and the pointwise SwiGLU pass): bit-exact.  fp16 / weight-only weights, in the units
of tests/test_gpu_gemv_instances.py: 1.0 fp16 ulp at the row's largest |v| (0.5 for float32 output); residual 1 ulp(max |v|) +
0.5 ulp(max |y|); gate |silu(g)| ulp16(max |v|) + 2 ulp16(exact).  Dual SwiGLU + quantiser: at most 1 LSB, at least 98 %
identical (tests/test_gemm_oracle.py shows the reference alone stays far inside that)."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import gemm_cases as GC
from oracle import gemm_oracle as GM
from oracle import gemv_oracle as GO
from oracle import llama_oracle as O
from oracle.quant_oracle import process_woq_layout
from tensorrt_llm.plugin import capi

pytestmark = pytest.mark.gpu

PAD = 3  # rows beyond M (activations, c, residual, gate) and beyond N (weights), all 0xFF
_NP_OF = {GC.DT_FLOAT: np.float32, GC.DT_HALF: np.float16, GC.DT_INT8: np.int8, GC.DT_INT32: np.int32}
WORST = {}  # family -> (worst error in the bound's units, case id)


class GemmParams(ctypes.Structure):
    """tllm_gemm_params_t (include/tllm_runtime_api.h)"""
    _fields_ = [('wtype', ctypes.c_int32), ('out_dtype', ctypes.c_int32), ('M', ctypes.c_int32), ('N', ctypes.c_int32),
                ('K', ctypes.c_int32), ('a', ctypes.c_void_p), ('lda', ctypes.c_int64), ('w', ctypes.c_void_p),
                ('ldw', ctypes.c_int64), ('scale_col', ctypes.c_void_p), ('scale_row', ctypes.c_void_p),
                ('per_channel', ctypes.c_int32), ('per_token', ctypes.c_int32), ('c', ctypes.c_void_p), ('ldc', ctypes.c_int64)]


@pytest.fixture(scope='module')
def gemm(lib):
    P, V, I = ctypes.POINTER(GemmParams), ctypes.c_void_p, ctypes.c_int32
    for name, args in (('tllm_gemm', [P, V]), ('tllm_gemm_epi', [P, V, V, V]), ('tllm_gemm_kernel', [P, V, V, I, V]),
                       ('tllm_gemm_static_cfg', [P]), ('tllm_gemm_swiglu_quant', [P, V, V, V, V]), ('tllm_gemm_tactics_import', [ctypes.c_char_p])):
        getattr(lib, name).argtypes, getattr(lib, name).restype = args, I
    lib.tllm_gemm_set_tile_cfg.argtypes, lib.tllm_gemm_set_tile_cfg.restype = [I], None
    lib.tllm_gemm_tactics_clear.restype = None
    yield lib
    lib.tllm_gemm_set_tile_cfg(0)
    lib.tllm_gemm_tactics_clear()
    for fam in sorted(WORST):
        print(f'worst error of family {fam}: {WORST[fam][0]:.3f} of its bound ({WORST[fam][1]})')


@pytest.fixture(scope='module')
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _padded(a, ld_bytes):
    """[rows, n] -> [rows + PAD, ld_bytes] uint8, 0xFF everywhere but the top-left corner"""
    a = np.ascontiguousarray(a)
    b = a.view(np.uint8).reshape(a.shape[0], -1)
    out = np.full((a.shape[0] + PAD, ld_bytes), 0xFF, np.uint8)
    out[:a.shape[0], :b.shape[1]] = b
    return out


def inputs(c):
    """numpy operands of a case, seeded by its id: activations 1.7 N(0, 1), weights 1.7 U(-1, 1) / sqrt(K) (SmoothQuant: random
    int8 with scales to match), so that the outputs are O(1)"""
    r = np.random.default_rng(zlib.crc32(GC.case_id(c).encode()))
    sq = c.wt == GC.W_INT8_SQ
    lda, ldw, ldc = GC.strides(c)
    M, N, K = c.M, c.N, c.K
    d = dict(lda=lda, ldw=ldw, ldc=ldc)
    nan32 = np.full(PAD, 0xFFFFFFFF, np.uint32).view(np.float32)
    if sq:
        a = r.integers(-127, 128, (M, K), dtype=np.int8)
        d['a'], d['a_buf'] = a, _padded(a, lda)
        nw = 2 if c.kernel == GC.DUAL else 1
        w = r.integers(-127, 128, (nw * N, K), dtype=np.int8)
        d['w'] = w
        d['w_bufs'] = [_padded(w[i * N:(i + 1) * N], ldw) for i in range(nw)]
        base = 0.013
        srow = (base * (1.0 + 0.17 * (np.arange(M) % 8))).astype(np.float32)
        big = 1000.0 if c.out == GC.DT_INT32 else 1.0  # integers worth comparing
        sc = (big * r.uniform(0.5, 1.5, nw * N) / (np.sqrt(K) * 73 * 73 * 1.6 * base)).astype(np.float32)  # |acc| ~ sqrt(K) 73^2, mean row scale 1.6 base
        d['scale_row'] = srow if c.per_token else srow[:1]
        d['scale_col'] = sc if c.per_channel else sc[:1]
        d['scale_row_buf'] = np.concatenate([d['scale_row'], nan32])
        d['scale_col_bufs'] = [np.concatenate([sc[i * N:(i + 1) * N] if c.per_channel else sc[:1], nan32]) for i in range(nw)]
        d['qscale'] = np.float32(21.0)
    else:
        a = (1.7 * r.standard_normal((M, K))).astype(np.float16)
        d['a'], d['a_buf'] = a, _padded(a, 2 * lda)
        w = (1.7 * r.uniform(-1, 1, (N, K)) / np.sqrt(K)).astype(np.float16)
        if c.wt == GC.W_FP16:
            d['w'], d['w_bufs'] = w, [_padded(w, ldw)]
        else:
            bits = 8 if c.wt == GC.W_INT8_WOQ else 4
            q_kn, s = O.woq_quantize(w.T.astype(np.float32), bits)
            d['w'], d['w_bufs'] = np.ascontiguousarray(q_kn.T), [_padded(process_woq_layout(q_kn, bits), ldw)]
            d['scale_col'] = s.astype(np.float16)
            d['scale_col_bufs'] = [np.concatenate([d['scale_col'], np.full(PAD, np.nan, np.float16)])]
    d['other'] = r.standard_normal((M, N)).astype(np.float16)  # the residual / the gate
    d['other_buf'] = _padded(d['other'], 2 * ldc)
    return d


class Device:
    def __init__(self, c, d):
        self.c, self.d = c, d
        cu = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
        self.a, self.w = cu(d['a_buf']), [cu(b) for b in d['w_bufs']]
        self.other = cu(d['other_buf'])
        self.scale_col = [cu(b) for b in d['scale_col_bufs']] if 'scale_col_bufs' in d else [None]
        self.scale_row = cu(d['scale_row_buf']) if 'scale_row_buf' in d else None
        self.qscale = cu(np.array([d['qscale']], np.float32)) if 'qscale' in d else None
        self.csz = np.dtype(_NP_OF[c.out]).itemsize

    def operands_intact(self):
        d = self.d
        return (np.array_equal(self.a.cpu().numpy(), d['a_buf'].reshape(-1)) and np.array_equal(self.other.cpu().numpy(), d['other_buf'].reshape(-1))
                and all(np.array_equal(w.cpu().numpy(), b.reshape(-1)) for w, b in zip(self.w, d['w_bufs'])))

    def params(self, cbuf):
        c, d = self.c, self.d
        ptr = lambda t: t.data_ptr() if t is not None else None
        return GemmParams(c.wt, c.out, c.M, c.N, c.K, self.a.data_ptr(), d['lda'], self.w[0].data_ptr(), d['ldw'], ptr(self.scale_col[0]),
                          ptr(self.scale_row), c.per_channel, c.per_token, cbuf.data_ptr(), d['ldc'])

    def launch(self, lib, inplace=False, kernel=None):
        """(rc, the WHOLE c buffer [M + PAD, ldc])"""
        c, d = self.c, self.d
        rows = c.M + PAD
        cbuf = torch.full((rows * d['ldc'] * self.csz, ), 0xFF, dtype=torch.uint8, device='cuda')
        if inplace:
            cbuf.copy_(self.other)
        q = self.params(cbuf)
        other = cbuf.data_ptr() if inplace else self.other.data_ptr()
        res = other if c.epi == GC.EPI_RES else None
        gate = other if c.epi == GC.EPI_GATE else None
        stream = torch.cuda.current_stream().cuda_stream
        kernel = c.kernel if kernel is None else kernel
        rc = 0
        try:
            if kernel <= 0 and c.force:
                lib.tllm_gemm_set_tile_cfg(c.force)
            if kernel == 0 and c.table:
                assert lib.tllm_gemm_tactics_import(f'{c.wt}:{c.M}:{c.N}:{c.K}:{c.table}:1.00;'.encode()) == 0, capi.last_error()
            for _ in range(1 if inplace else c.repeat):  # (in place every launch adds the residual again)
                if kernel == GC.DUAL:
                    rc |= lib.tllm_gemm_swiglu_quant(ctypes.byref(q), self.w[1].data_ptr(), self.scale_col[1].data_ptr(), self.qscale.data_ptr(), stream)
                elif kernel == 0 and c.epi == GC.EPI_NONE:
                    rc |= lib.tllm_gemm(ctypes.byref(q), stream)
                elif kernel == 0:
                    rc |= lib.tllm_gemm_epi(ctypes.byref(q), res, gate, stream)
                else:
                    rc |= lib.tllm_gemm_kernel(ctypes.byref(q), res, gate, kernel, stream)
            try:
                torch.cuda.synchronize()
            except RuntimeError as e:  # a HIP error leaves the context unusable: nothing more is launched on it
                pytest.exit(f'{GC.case_id(c)}: the device reported {e}', returncode=4)
        finally:
            lib.tllm_gemm_set_tile_cfg(0)
            lib.tllm_gemm_tactics_clear()
        return rc, cbuf.cpu().numpy().view(_NP_OF[c.out]).reshape(rows, d['ldc'])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _untouched(a):
    return bool((_bits(a) == 0xFF).all())


def family(c, inst):
    k = GC.key(inst)
    return f'{k[0]}/{GC.WT_NAME[c.wt]}' if k[0] != 'dual' else 'dual'


def compare(c, d, got, inst, tag):
    """c[:M, :N] against the oracle; returns the worst error in the unit of the case's bound"""
    sq = c.wt == GC.W_INT8_SQ
    if c.kernel == GC.DUAL:
        N = c.N
        sc = d['scale_col']
        ref = GM.dual_swiglu_quant(d['a'], d['w'][:N], d['w'][N:], sc[:N] if c.per_channel else sc, sc[N:] if c.per_channel else sc,
                                   d['scale_row'], d['qscale'])
        diff = np.abs(got.astype(np.int32) - ref.astype(np.int32))
        same = float((diff == 0).mean())
        print(f'{tag} dual SwiGLU + quantiser: worst {diff.max()} LSB, {100 * same:.3f} % identical; max |q| = {np.abs(ref).max()}')
        assert diff.max() <= 1 and same >= 0.98, (int(diff.max()), same)
        return float(diff.max())
    epi = {GC.EPI_NONE: GM.EPI_NONE, GC.EPI_RES: GM.EPI_RESIDUAL, GC.EPI_GATE: GM.EPI_GATE}[c.epi]
    ref = GM.gemm(d['a'], d['w'], c.wt, epi, c.out, d.get('scale_col'), d.get('scale_row'), d['other'], d['other'])
    v = ref['v']
    if sq and c.epi != GC.EPI_GATE:
        want = ref['y'].astype(_NP_OF[c.out])
        bad = int((_bits(got) != _bits(want)).reshape(c.M, c.N, -1).any(-1).sum())
        print(f'{tag} SmoothQuant {c.epi} -> {GC.DT_NAME[c.out]}: {bad} of {got.size} outputs differ (must be bit-exact); max |y| = {np.abs(want.astype(np.float64)).max():.2f}')
        assert bad == 0
        return 0.0
    g64 = got.astype(np.float64)
    rowmax = lambda x: np.abs(x).max(axis=1, keepdims=True)
    if c.epi == GC.EPI_GATE:
        # the gate is an exact input: 1 ulp on v through the product, and the epilogue's own fp16 roundings
        s = GM.silu(d['other'].astype(np.float64))
        exact = s * v
        bound = np.abs(s) * GO.ulp16(rowmax(v)) + 2.0 * GO.ulp16(exact)
        unit = 'of |silu(g)| ulp16(max |v|) + 2 ulp16(exact)'
    elif c.epi == GC.EPI_RES:
        exact = v + d['other'].astype(np.float64)
        bound = 1.0 * GO.ulp16(rowmax(v)) + 0.5 * GO.ulp16(rowmax(exact)) + 0 * exact
        unit = 'of 1 ulp(max |v|) + 0.5 ulp(max |y|)'
    else:
        exact = v
        f = 1.0 if c.out == GC.DT_HALF else 0.5
        bound = f * GO.ulp16(rowmax(v)) + 0 * exact
        unit = f'of {f} fp16 ulp(max |y| of the row)'
    assert np.isfinite(g64).all(), f'{int((~np.isfinite(g64)).sum())} non-finite outputs'
    worst = float((np.abs(g64 - exact) / bound).max())
    print(f'{tag} worst error {worst:.3f} {unit}; max |y| = {np.abs(exact).max():.2f}')
    assert worst <= 1.0, worst
    return worst


@pytest.mark.parametrize('c', GC.CASES, ids=GC.case_id)
def test_gemm_instance_against_the_float64_oracle(c, gemm, cus):
    tag = f'[{GC.case_id(c)}]'
    inst = GC.instance(c, cus)
    d = inputs(c)
    dev = Device(c, d)
    if c.kernel >= 0 and c.wt in (GC.W_INT8_SQ, GC.W_FP16):
        q = dev.params(dev.other)  # (no launch: the c pointer only has to be aligned)
        assert gemm.tllm_gemm_static_cfg(ctypes.byref(q)) == GC.static_cfg(c, cus), 'gemm_static_cfg and its mirror disagree'
    rc, y = dev.launch(gemm)
    if inst[0] == 'refused':
        assert (rc == 1) if c.kernel > 0 else (rc != 0), f'{tag} expected a refusal ({inst[1]}), rc = {rc}'
        assert _untouched(y), 'a refused call wrote c'
        print(f'{tag} refused ({inst[1]}): {capi.last_error()}')
        return
    assert rc == 0, (f'{tag} the mirror says {inst} at {cus} CUs, the library refuses: {capi.last_error()}'
                     + (' - the occupancy query answers fewer workgroups per CU than this split-K form is built for' if inst[0] == 'splitk' else ''))
    # ---- determinism, sentinels, operands
    rc2, y2 = dev.launch(gemm)
    assert rc2 == 0 and np.array_equal(_bits(y), _bits(y2)), 'two runs differ'
    assert _untouched(y[c.M:]), 'c rows >= M written'
    assert _untouched(y[:, c.N:]), 'c columns >= N written'
    assert dev.operands_intact(), 'an operand (a, w, residual / gate) was modified'
    # ---- the oracle
    worst = compare(c, d, y[:c.M, :c.N], inst, tag)
    fam = family(c, inst)
    print(f'{tag} ran {inst}' + (f', (tiles_m, tiles, workgroups) = {GC.persist_walk(c, cus)}' if inst[0] == 'persist' else '')
          + f'; worst {worst:.3f}')
    if worst >= WORST.get(fam, (-1.0, ''))[0]:
        WORST[fam] = (worst, GC.case_id(c))
    # ---- a table entry that serves: the very kernel tllm_gemm_kernel runs under that id
    if c.kernel == 0 and c.table and inst[0] in ('table:lockstep', 'table:phased'):
        rck, yk = dev.launch(gemm, kernel=c.table)
        assert rck == 0 and np.array_equal(_bits(yk), _bits(y)), 'the table entry did not run the kernel it names'
    # ---- residual == c (the session's own usage)
    if c.inplace:
        assert c.epi == GC.EPI_RES
        rci, yi = dev.launch(gemm, inplace=True)
        want = d['other_buf'].view(np.float16).reshape(y.shape).copy()
        if GC.instance(c, cus, inplace=True)[0] == 'refused':
            assert rci != 0 and np.array_equal(_bits(yi), _bits(want)), 'a refused in-place call wrote c'
            print(f'{tag} in place refused: {capi.last_error()}')
            return
        assert rci == 0, capi.last_error()
        want[:c.M, :c.N] = y[:c.M, :c.N]
        assert np.array_equal(_bits(yi), _bits(want)), 'in place: differs from the out-of-place run, or wrote outside the problem'


def test_weight_only_tile_shapes_agree_bit_for_bit(gemm, cus):
    """the six tile shapes of gemm_woq.hip accumulate every output over K in the same order: identical bits"""
    for wt in (GC.W_INT8_WOQ, GC.W_INT4_WOQ):
        c0 = GC.Case('woq-tiles', wt, 300, 456, 704, kernel=101, strided=1)
        d = inputs(c0)
        outs = []
        for tile in GC.WOQ:
            rc, y = Device(c0._replace(kernel=100 + tile), d).launch(gemm)
            assert rc == 0, capi.last_error()
            outs.append(y)
        assert all(np.array_equal(_bits(o), _bits(outs[0])) for o in outs[1:])
