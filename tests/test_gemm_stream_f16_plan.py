"""tllm_gemm_stream_f16_layout (no GPU): the plan of kernels/gemm_stream_f16.hip - K-slices in multiples of the ring block of 128
k-elements, row groups, LDS, workspace - over the 7B projections, the 7B lm_head and the shapes of the GPU test."""
import ctypes

import pytest

from tensorrt_llm.plugin import capi
from test_gemm_stream_plan import SHAPES_7B

HEAD_7B = (32000, 4096)


def layout(M, N, K, cus):
    lib = capi.load_library()
    p = capi.GemmParams(wtype=0, M=M, N=N, K=K)
    ws = ctypes.c_int64()
    v = [ctypes.c_int32() for _ in range(6)]
    rc = lib.tllm_gemm_stream_f16_layout(ctypes.byref(p), cus, ctypes.byref(ws), *[ctypes.byref(x) for x in v])
    names = ('k_slices', 'k_slice', 'row_groups', 'groups_per_workgroup', 'grid_x', 'lds_bytes')
    return rc, dict(zip(names, (int(x.value) for x in v)), workspace_bytes=int(ws.value))


@pytest.mark.parametrize('M', [9, 16, 33, 48, 64])
@pytest.mark.parametrize('N,K,cus', [(n, k, 256) for n, k in SHAPES_7B + [HEAD_7B]] + [(16, 64, 256), (40, 448, 304), (16424, 64, 256),
                                                                                      (16, 8768, 4), (200, 2368, 4), (40, 2368, 256)])
def test_the_plan(M, N, K, cus):
    rc, p = layout(M, N, K, cus)
    assert rc == 0, capi.last_error()
    T = (M + 15) // 16
    ks, S = p['k_slice'], p['k_slices']
    # the slices tile K without a gap or an empty slice, in multiples of the ring block (K itself below it)
    assert ks > 0 and (S - 1) * ks < K <= S * ks and (ks % 128 == 0 or ks == K == 64)
    G = p['row_groups']
    assert (G - 1) * 16 < N <= G * 16
    assert p['grid_x'] >= 1 and p['groups_per_workgroup'] % 4 == 0 and p['grid_x'] * p['groups_per_workgroup'] >= G
    assert (p['grid_x'] - 1) * 4 < G  # no workgroup without a quad
    # four rings of 16 KB and the fp16 panel (the slice rounded up to the block of 128 elements)
    assert p['lds_bytes'] == 4 * 16384 + 16 * T * 2 * ((ks + 127) // 128 * 128) <= 160 * 1024
    assert p['workspace_bytes'] == S * G * T * 1024
    assert p['grid_x'] * S <= max(cus, S)


def test_the_head_takes_as_few_slices_as_its_panel_allows():
    # 262 MB of weights: a slice more is 4 bytes x bucket x 32000, written and read back - the plan stays at the panel's minimum
    for M, slices in ((16, 2), (32, 3), (48, 4), (64, 6)):
        rc, p = layout(M, *HEAD_7B, 256)
        assert rc == 0 and p['k_slices'] == slices
    assert layout(64, *HEAD_7B, 256)[1]['workspace_bytes'] == 49152000  # the figure of the header comment


@pytest.mark.parametrize('M,K', [(8, 4096), (65, 4096), (16, 96)])
def test_the_plan_refuses(M, K):
    rc, _ = layout(M, 4096, K, 256)
    assert rc != 0 and ('9 .. 64' in capi.last_error() or 'multiple of 64' in capi.last_error())
