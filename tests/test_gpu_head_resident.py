"""The lm_head launch's row boundary between the two cache policies (kernels.h GemvParams::resident_rows; gemv_impl.h, the head
family): rows below it load with the allocating policy, rows from it on stream non-temporally, chosen per row pair by a scalar
branch between two load sequences.  A policy is a hint: the boundary must not change one bit of the result.

The head instance (fp16 weights, RMSNorm prologue, fp32 output, one row) through tllm_gemv_head at N in {5, 37, 260} x K in
{264, 4096} - less than one tile per row and two tiles per row, N odd, several row groups per wave slot - with resident_rows in
{0, 1, 3, N - 1, N, N + 7}: odd boundaries, a boundary inside a row pair, a boundary beyond N.  Every operand is an interior view of
a 0xFF-filled allocation with ldw = row bytes + 48, ldx > K, ldy > N (tests/test_gpu_entry_path.py): a load sequence that builds an
address from the wrong base or stride reads NaN bits.  Held to oracle/gemv_oracle.py at the bound of tests/test_gpu_gemv_instances.py
for this family (0.5 fp16 ulp of the row's largest value); the six outputs are bit-identical to each other and to tllm_gemv's."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import gemv_cases as GC
import test_gpu_gemv_instances as TG
from helpers import GemvParams
from oracle import gemv_oracle as GO
from tensorrt_llm.plugin import capi
from test_gpu_entry_path import View, _rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def head(lib):
    lib.tllm_gemv.argtypes = [ctypes.POINTER(GemvParams), ctypes.c_void_p]
    lib.tllm_gemv.restype = ctypes.c_int32
    lib.tllm_gemv_head.argtypes = [ctypes.POINTER(GemvParams), ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    lib.tllm_gemv_head.restype = ctypes.c_int32
    return lib


@pytest.mark.parametrize('K', [264, 4096])
@pytest.mark.parametrize('N', [5, 37, 260])
def test_the_row_boundary_does_not_change_the_logits(N, K, head):
    c = GC.Case('head', GC.W_FP16, GC.PRO_RMSNORM, GC.EPI_NONE, 1, N, K, out=GC.DT_FLOAT)
    assert GC.instance(c) == ('valu', GC.W_FP16, GC.PK_NORM, GC.EK_PLAIN, 1, GC.NXV_SMALL, GC.U)
    tag = f'[head N {N} K {K}]'
    r = np.random.default_rng(zlib.crc32(tag.encode()))
    ldw, ldx, ldy = 2 * K + 48, K + 16, N + 8
    x = (1.7 * r.standard_normal((1, K))).astype(np.float16)
    gamma = r.uniform(0.5, 1.5, K).astype(np.float16)
    w = (1.7 * r.uniform(-1, 1, (N, K)) / np.sqrt(K)).astype(np.float16)
    d = dict(x=x, gamma=gamma, w=w, residual=np.zeros((1, N), np.float16))
    V = dict(x=View(_rows(x, ldx)), w=View(_rows(w.view(np.uint8), ldw)), gamma=View(gamma))
    stream = torch.cuda.current_stream().cuda_stream

    def launch(resident_rows):
        y = View(np.full((1, ldy * 4), 0xFF, np.uint8))
        xpro = View(np.full(K * 2, 0xFF, np.uint8))
        q = GemvParams(c.wt, c.pro, c.epi, GC.DT_FLOAT, 1, N, K, V['x'].ptr, ldx, V['w'].ptr, ldw, None, None, 1, 0, V['gamma'].ptr,
                       1e-6, None, None, xpro.ptr, None, None, y.ptr, ldy)
        rc = (head.tllm_gemv(ctypes.byref(q), stream) if resident_rows is None
              else head.tllm_gemv_head(ctypes.byref(q), resident_rows, None, stream))
        torch.cuda.synchronize()
        assert rc == 0, capi.last_error()
        for k, v in list(V.items()) + [('y', y), ('xpro', xpro)]:
            front, mid, back = v.read()
            assert (front == 0xFF).all() and (back == 0xFF).all(), f'{k}: bytes outside the view written'
            if k in V:
                assert np.array_equal(mid, v.host), f'{k} was modified'
        out = y.read()[1].view(np.float32).reshape(1, ldy)
        assert TG._untouched(out[:, N:]), 'y columns >= N written'
        return out, xpro.read()[1].view(np.float16).reshape(1, K)

    base, xp = launch(None)  # tllm_gemv: the launch every other caller makes
    ref = GO.prologue(x, c.pro, gamma, 1e-6, None)
    diff = np.abs(TG._ord16(xp) - TG._ord16(ref['xp']))
    assert diff.max() <= 2 and float((diff == 0).mean()) >= 0.99
    worst = TG.stage_b(c, d, base, xp, None, tag)
    print(f'{tag} tllm_gemv: worst error {worst:.3f} of the bound')
    for rr in (0, 1, 3, N - 1, N, N + 7):
        got, xp_rr = launch(rr)
        same = np.array_equal(got.view(np.uint32)[:, :N], base.view(np.uint32)[:, :N])
        print(f'{tag} resident_rows {rr}: logits {"bit-identical" if same else "DIFFER"}')
        assert same, rr
        assert np.array_equal(xp_rr.view(np.uint16), xp.view(np.uint16))


def test_the_options_are_refused_outside_the_head_family(head):
    """a call that sets resident_rows on another weight type or on several rows is an error, never a launch that ignores it"""
    N, K = 8, 64
    x = torch.zeros((2, K), dtype=torch.float16, device='cuda')
    w = torch.zeros((N, K), dtype=torch.float16, device='cuda')
    w8 = torch.zeros((N, K), dtype=torch.int8, device='cuda')
    sc = torch.ones(N, dtype=torch.float32, device='cuda')
    y = torch.full((2, N), 7.0, dtype=torch.float32, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream
    two_rows = GemvParams(GC.W_FP16, GC.PRO_NONE, GC.EPI_NONE, GC.DT_FLOAT, 2, N, K, x.data_ptr(), K, w.data_ptr(), 2 * K, None, None,
                          1, 0, None, 1e-6, None, None, None, None, None, y.data_ptr(), N)
    int8_w = GemvParams(GC.W_INT8_SQ, GC.PRO_NONE, GC.EPI_NONE, GC.DT_FLOAT, 1, N, K, w8.data_ptr(), K, w8.data_ptr(), K, sc.data_ptr(),
                        sc.data_ptr(), 1, 0, None, 1e-6, None, None, None, None, None, y.data_ptr(), N)
    for q in (two_rows, int8_w):
        assert head.tllm_gemv_head(ctypes.byref(q), 4, None, stream) != 0
        assert 'lm_head' in capi.last_error()
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
