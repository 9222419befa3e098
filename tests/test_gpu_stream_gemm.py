"""tllm_gemm_stream (kernels/gemm_stream_sq.hip) against the exact-integer oracle (oracle/gemv_oracle.py): bit-exact on every output,
at the smallest shapes that reach each decision of the kernel and its plan.  Operands as tests/test_gpu_gemv_instances.py draws
them; row-indexed buffers hold 64 rows of 0xFF, rows >= M of A stay 0xFF; every case runs twice."""
import ctypes
import zlib
from collections import namedtuple

import numpy as np
import pytest
import torch

from oracle import gemv_oracle as GO
from tensorrt_llm.plugin import capi

pytestmark = pytest.mark.gpu
ROWS = 64
W_INT8_SQ, DT_FLOAT, DT_HALF = 3, 0, 1

# N 'big': 64 * CUs + 40 - a workgroup walks a second quad of row groups, the last group is partial (K small).
# K 448: not a multiple of the 256-byte DMA block.  cus 4 (the planner's hook) with K 8768 at M <= 16 / K 2368, N 200 at M = 64:
# 4 / 3 K-slices with a remainder in the last (1856 / 320 bytes, both with a partial block) and 9 / 12 blocks through a wave's
# ring of four slots - it wraps twice.  K 2368 at M = 64 on the device's own CU count: 3 slices.
Case = namedtuple('Case', 'M N K pc pt epi strided cus')
CASES = [Case(*c) for c in [
    (9, 16, 64, 0, 0, 'f16', 0, 0), (16, 40, 64, 1, 0, 'f16', 0, 0), (16, 16, 64, 1, 1, 'f32', 0, 0), (48, 16, 64, 0, 1, 'f16', 0, 0),
    (33, 16, 64, 1, 0, 'inplace', 0, 0), (17, 16, 448, 0, 1, 'f16', 0, 0), (33, 40, 448, 1, 1, 'f32', 0, 0),
    (48, 40, 448, 1, 1, 'res', 0, 0), (64, 16, 448, 1, 0, 'inplace', 0, 0), (9, 40, 448, 0, 1, 'f16', 0, 0),
    (64, 'big', 64, 1, 1, 'f16', 0, 0), (17, 'big', 64, 0, 0, 'res', 0, 0),
    (16, 16, 8768, 1, 1, 'f16', 0, 4), (9, 40, 8768, 1, 0, 'inplace', 0, 4),
    (64, 200, 2368, 1, 1, 'f16', 0, 4), (48, 200, 2368, 0, 1, 'f32', 0, 4), (33, 200, 2368, 1, 1, 'res', 0, 4),
    (64, 40, 2368, 1, 1, 'f16', 0, 0), (17, 40, 2368, 0, 0, 'f16', 1, 0), (64, 40, 448, 1, 1, 'res', 1, 0)]]
case_id = lambda c: '-'.join(str(v) for v in c)


def _padded(a, rows, ld):
    out = np.full((rows, ld * a.itemsize), 0xFF, np.uint8).view(a.dtype)
    out[:a.shape[0], :a.shape[1]] = a
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


class Problem:
    """operands of a case on the host and the device; run() returns (rc, the whole C buffer [ROWS, ldc])"""

    def __init__(self, c):
        r = np.random.default_rng(zlib.crc32(case_id(c).encode()))
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        self.c, self.N = c, (64 * cus + 40 if c.N == 'big' else c.N)
        M, N, K = c.M, self.N, c.K
        self.lda, self.ldw, self.ldc = (K + 32, K + 64, N + 8) if c.strided else (K, K, N)
        self.odt = DT_FLOAT if c.epi == 'f32' else DT_HALF
        self.np_out = np.float32 if c.epi == 'f32' else np.float16
        self.x = r.integers(-127, 128, (M, K)).astype(np.int8)
        self.w = r.integers(-127, 128, (N, K)).astype(np.int8)
        # |acc| ~ sqrt(K) * 73 * 73: column x row scales bring the outputs to O(1)
        srow = (0.013 * (1.0 + 0.17 * np.arange(ROWS))).astype(np.float32)
        self.srow = srow[:M] if c.pt else srow[:1]
        sc = (r.uniform(0.5, 1.5, N) / (np.sqrt(K) * 73 * 73 * 0.013)).astype(np.float32)
        self.scol = sc if c.pc else sc[:1]
        self.res = r.standard_normal((M, N)).astype(np.float16)
        self.host = dict(a=_padded(self.x, ROWS, self.lda), w=_padded(self.w, N, self.ldw), res=_padded(self.res, ROWS, self.ldc))
        cu = lambda a: torch.from_numpy(_bits(a).reshape(-1).copy()).cuda()
        self.dev = {k: cu(v) for k, v in self.host.items()}
        self.dev.update(scol=cu(self.scol), srow=cu(srow if c.pt else srow[:1]))
        self.lib = capi.load_library()
        nbytes = ctypes.c_int64()
        p = capi.GemmParams(wtype=W_INT8_SQ, M=M, N=N, K=K)
        assert self.lib.tllm_gemm_stream_layout(ctypes.byref(p), c.cus or cus, ctypes.byref(nbytes), *[None] * 6) == 0
        self.ws = torch.full((nbytes.value, ), 0xFF, dtype=torch.uint8, device='cuda')

    def want(self):
        ref = GO.gemv(self.x, self.w, W_INT8_SQ, GO.EPI_RESIDUAL if self.c.epi in ('res', 'inplace') else GO.EPI_NONE, self.odt,
                      self.scol, self.srow, self.res)
        return ref['y'].astype(self.np_out)

    def run(self, inplace=False, **over):
        c = self.c
        cbuf = torch.full((ROWS * self.ldc * np.dtype(self.np_out).itemsize, ), 0xFF, dtype=torch.uint8, device='cuda')
        if inplace:
            cbuf.copy_(self.dev['res'])
        a = dict(wtype=W_INT8_SQ, out_dtype=self.odt, M=c.M, N=self.N, K=c.K, a=self.dev['a'].data_ptr(), lda=self.lda,
                 w=self.dev['w'].data_ptr(), ldw=self.ldw, scale_col=self.dev['scol'].data_ptr(), scale_row=self.dev['srow'].data_ptr(),
                 per_channel=c.pc, per_token=c.pt, c=cbuf.data_ptr(), ldc=self.ldc, ws=self.ws.data_ptr(), ws_bytes=self.ws.numel())
        a.update(over)
        ws, ws_bytes = a.pop('ws'), a.pop('ws_bytes')
        res = None if c.epi in ('f16', 'f32') else (cbuf if inplace else self.dev['res']).data_ptr()
        try:
            self.lib.tllm_gemm_stream_set_cus(c.cus)
            rc = self.lib.tllm_gemm_stream(ctypes.byref(capi.GemmParams(**a)), res, ws, ws_bytes, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        finally:
            self.lib.tllm_gemm_stream_set_cus(0)
        return rc, cbuf.cpu().numpy().view(self.np_out).reshape(ROWS, self.ldc)


@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_stream_gemm_is_bit_exact_against_the_oracle(c):
    pb = Problem(c)
    inplace = c.epi == 'inplace'
    rc, y = pb.run(inplace)
    assert rc == 0, capi.last_error()
    rc2, y2 = pb.run(inplace)
    assert rc2 == 0 and np.array_equal(_bits(y), _bits(y2)), 'two runs differ'
    got, want = y[:c.M, :pb.N], pb.want()
    bad = int((_bits(got) != _bits(want)).reshape(c.M, pb.N, -1).any(-1).sum())
    print(f'[{case_id(c)}] {bad} of {got.size} outputs differ (must be bit-exact)')
    assert bad == 0
    if inplace:  # the buffer held the residual: rows >= M keep it
        assert np.array_equal(_bits(y[c.M:]), _bits(pb.host['res'][c.M:])), 'rows >= M written'
    else:
        assert (_bits(y[c.M:]) == 0xFF).all(), 'rows >= M written'
    assert (_bits(y[:, pb.N:]) == 0xFF).all(), 'columns >= N written'
    for k in ('a', 'w', 'res'):
        assert np.array_equal(pb.dev[k].cpu().numpy(), _bits(pb.host[k]).reshape(-1)), f'{k} was modified'


REFUSALS = [(dict(wtype=0), 'SmoothQuant'), (dict(M=8), '9 .. 64'), (dict(M=65), '9 .. 64'), (dict(K=96), 'multiple of 64'),
            (dict(a_off=1), 'aligned'), (dict(lda=456), 'lda'), (dict(ldw=456), 'ldw'), (dict(ldc=42), 'ldc'),
            (dict(ws=None), 'workspace'), (dict(ws_off=4), 'workspace'), (dict(ws_bytes_off=-1), 'workspace')]


@pytest.mark.parametrize('over,needle', REFUSALS, ids=lambda v: '-'.join(v) if isinstance(v, dict) else v)
def test_stream_gemm_refuses(over, needle):
    pb = Problem(Case(16, 40, 448, 1, 1, 'f16', 1, 0))  # strided: room for the odd strides
    over = dict(over)
    if 'a_off' in over:
        over['a'] = pb.dev['a'].data_ptr() + over.pop('a_off')
    if 'ws_off' in over:
        over['ws'] = pb.ws.data_ptr() + over.pop('ws_off')
    if 'ws_bytes_off' in over:
        over['ws_bytes'] = pb.ws.numel() + over.pop('ws_bytes_off')
    rc, y = pb.run(**over)
    assert rc != 0 and needle in capi.last_error(), capi.last_error()
    assert (_bits(y) == 0xFF).all(), 'C written by a refused call'
