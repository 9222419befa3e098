"""tllm_gemm_stream_f16 (kernels/gemm_stream_f16.hip) against the float64 oracle (oracle/gemv_oracle.py) within the bounds
tests/test_gpu_gemm_instances.py holds fp16 weights to, at the smallest shapes that reach each decision of the kernel and its plan.
Buffers are padded with 0xFF (fp16 NaN in rows >= M of A, rows >= N of W and behind K in a strided row); every case runs twice."""
import ctypes
import zlib
from collections import namedtuple

import numpy as np
import pytest
import torch

from oracle import gemv_oracle as GO
from tensorrt_llm.plugin import capi
from test_gpu_stream_gemm import ROWS, _bits, _padded

pytestmark = pytest.mark.gpu
DT_FLOAT, DT_HALF = 0, 1

# N 'big': 64 * CUs + 40 - a workgroup walks a second quad, the last group is partial.  K 64: half a ring block of 128; 448: not a
# multiple of it.  cus 4 (the planner's hook) with K 8768 at M = 16 / K 2368, N 200 at M = 64: several slices with a remainder in
# the last, 18 and more blocks through a wave's ring of 4 slots; K 2368 at M = 64 on the device's own CU count: 4 slices.
Case = namedtuple('Case', 'M N K epi strided cus')
CASES = [Case(*s) for s in [(9, 16, 64, 'f16', 0, 0), (16, 40, 64, 'f32', 0, 0), (17, 16, 448, 'res', 0, 0), (33, 40, 448, 'gate', 0, 0),
                            (48, 16, 448, 'inplace', 0, 0), (64, 'big', 64, 'f16', 0, 0), (16, 16, 8768, 'f16', 0, 4),
                            (64, 200, 2368, 'gate', 0, 4), (64, 40, 2368, 'res', 0, 0), (17, 40, 448, 'f16', 1, 0)]]
case_id = lambda c: '-'.join(str(v) for v in c)


class Problem:
    """operands of a case on the host and the device; run() returns (rc, the whole C buffer [ROWS, ldc])"""
    def __init__(self, c):
        r = np.random.default_rng(zlib.crc32(case_id(c).encode()))
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        self.c, self.N = c, (64 * cus + 40 if c.N == 'big' else c.N)
        M, N, K = c.M, self.N, c.K
        pad = (32, 64, 8) if c.strided else (0, 0, 0)
        self.lda, ldw_el, self.ldc = K + pad[0], K + pad[1], N + pad[2]
        self.ldw = 2 * ldw_el  # bytes, as tllm_gemm takes it
        self.odt, self.np_out = (DT_FLOAT, np.float32) if c.epi == 'f32' else (DT_HALF, np.float16)
        self.x = r.standard_normal((M, K)).astype(np.float16)
        self.w = (r.standard_normal((N, K)) / np.sqrt(K)).astype(np.float16)  # outputs of O(1)
        self.other = r.standard_normal((M, N)).astype(np.float16)  # the residual or the gate
        self.host = dict(a=_padded(self.x, ROWS, self.lda), w=_padded(self.w, N + 3, ldw_el), other=_padded(self.other, ROWS, self.ldc))
        cu = lambda a: torch.from_numpy(_bits(a).reshape(-1).copy()).cuda()
        self.dev = {k: cu(v) for k, v in self.host.items()}
        self.lib = capi.load_library()
        nbytes = ctypes.c_int64()
        p = capi.GemmParams(wtype=0, M=M, N=N, K=K)
        assert self.lib.tllm_gemm_stream_f16_layout(ctypes.byref(p), c.cus or cus, ctypes.byref(nbytes), *[None] * 6) == 0
        self.ws = torch.full((nbytes.value, ), 0xFF, dtype=torch.uint8, device='cuda')

    def run(self, inplace=False, **over):
        c = self.c
        cbuf = torch.full((ROWS * self.ldc * np.dtype(self.np_out).itemsize, ), 0xFF, dtype=torch.uint8, device='cuda')
        if inplace:
            cbuf.copy_(self.dev['other'])
        a = dict(wtype=0, out_dtype=self.odt, M=c.M, N=self.N, K=c.K, a=self.dev['a'].data_ptr(), lda=self.lda,
                 w=self.dev['w'].data_ptr(), ldw=self.ldw, c=cbuf.data_ptr(), ldc=self.ldc, ws=self.ws.data_ptr(),
                 ws_bytes=self.ws.numel(), epi=c.epi)
        a.update(over)
        ws, ws_bytes, epi = a.pop('ws'), a.pop('ws_bytes'), a.pop('epi')
        other = (cbuf if inplace else self.dev['other']).data_ptr()
        st, p = torch.cuda.current_stream().cuda_stream, ctypes.byref(capi.GemmParams(**a))
        try:
            self.lib.tllm_gemm_stream_set_cus(c.cus)
            rc = self.lib.tllm_gemm_stream_f16(p, other if epi in ('res', 'inplace') else None, other if epi == 'gate' else None,
                                               ws, ws_bytes, st)
            torch.cuda.synchronize()
        finally:
            self.lib.tllm_gemm_stream_set_cus(0)
        return rc, cbuf.cpu().numpy().view(self.np_out).reshape(ROWS, self.ldc)

    def error(self, got):
        """the worst error of got [M, N] in the unit of the epilogue's bound (tests/test_gpu_gemm_instances.py compare())"""
        epi, o = self.c.epi, self.other.astype(np.float64)
        v = GO.gemv(self.x, self.w, GO.W_FP16, GO.EPI_NONE, self.odt)['v']
        rowmax = lambda x: np.abs(x).max(axis=1, keepdims=True)
        if epi == 'gate':
            s = o / (1.0 + np.exp(-o))
            exact, bound = s * v, np.abs(s) * GO.ulp16(rowmax(v)) + 2.0 * GO.ulp16(s * v)
        elif epi in ('res', 'inplace'):
            exact, bound = v + o, 1.0 * GO.ulp16(rowmax(v)) + 0.5 * GO.ulp16(rowmax(v + o)) + 0 * v
        else:
            exact, bound = v, (1.0 if epi == 'f16' else 0.5) * GO.ulp16(rowmax(v)) + 0 * v
        assert np.isfinite(got).all(), 'non-finite outputs'
        return float((np.abs(got.astype(np.float64) - exact) / bound).max())


@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_stream_gemm_f16_against_the_oracle(c):
    pb = Problem(c)
    inplace = c.epi == 'inplace'
    rc, y = pb.run(inplace)
    assert rc == 0, capi.last_error()
    rc2, y2 = pb.run(inplace)
    assert rc2 == 0 and np.array_equal(_bits(y), _bits(y2)), 'two runs differ'
    worst = pb.error(y[:c.M, :pb.N])
    print(f'[{case_id(c)}] worst error {worst:.3f} of the bound of family {"res" if inplace else c.epi}')
    assert worst <= 1.0
    # rows >= M keep what the buffer held: the residual (in place) or 0xFF
    assert np.array_equal(_bits(y[c.M:]), _bits(pb.host['other'][c.M:]) if inplace else np.full_like(_bits(y[c.M:]), 0xFF)), 'rows >= M written'
    assert (_bits(y[:, pb.N:]) == 0xFF).all(), 'columns >= N written'
    for k in ('a', 'w', 'other'):
        assert np.array_equal(pb.dev[k].cpu().numpy(), _bits(pb.host[k]).reshape(-1)), f'{k} was modified'


REFUSALS = {'wtype=1': (lambda pb: dict(wtype=1), 'not fp16'), 'M=8': (lambda pb: dict(M=8), '9 .. 64'),
            'M=65': (lambda pb: dict(M=65), '9 .. 64'), 'K=96': (lambda pb: dict(K=96), 'multiple of 64'),
            'A misaligned': (lambda pb: dict(a=pb.dev['a'].data_ptr() + 2), 'aligned'),
            'workspace too small': (lambda pb: dict(ws_bytes=pb.ws.numel() - 1), 'workspace'),
            'residual with fp32 output': (lambda pb: dict(epi='res', out_dtype=DT_FLOAT), 'fp16 output')}


@pytest.mark.parametrize('name', REFUSALS)
def test_stream_gemm_f16_refuses(name):
    over, needle = REFUSALS[name]
    pb = Problem(Case(16, 40, 448, 'f16', 1, 0))
    rc, y = pb.run(**over(pb))
    assert rc != 0 and needle in capi.last_error(), capi.last_error()
    assert (_bits(y) == 0xFF).all(), 'C written by a refused call'
