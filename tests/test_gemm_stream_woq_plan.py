"""tllm_gemm_stream_layout with the weight-only types (no GPU): the plan of kernels/gemm_stream_woq.hip - K-slices in k-elements,
row groups, LDS, workspace."""
import ctypes

import pytest

from tensorrt_llm.plugin import capi
from test_gemm_stream_plan import SHAPES_7B


def layout(wtype, M, N, K, cus):
    lib = capi.load_library()
    p = capi.GemmParams(wtype=wtype, M=M, N=N, K=K)
    ws = ctypes.c_int64()
    v = [ctypes.c_int32() for _ in range(6)]
    assert lib.tllm_gemm_stream_layout(ctypes.byref(p), cus, ctypes.byref(ws), *[ctypes.byref(x) for x in v]) == 0, capi.last_error()
    names = ('k_slices', 'k_slice', 'row_groups', 'groups_per_workgroup', 'grid_x', 'lds_bytes')
    return dict(zip(names, (int(x.value) for x in v)), workspace_bytes=int(ws.value))


@pytest.mark.parametrize('wtype', [1, 2])
@pytest.mark.parametrize('M', [9, 16, 17, 33, 48, 64])
@pytest.mark.parametrize('N,K,cus', [(n, k, 256) for n, k in SHAPES_7B] + [(16, 64, 256), (40, 448, 304), (16424, 64, 256),
                                                                           (16, 8768, 4), (200, 2368, 4), (40, 2368, 256)])
def test_the_plan(wtype, M, N, K, cus):
    p = layout(wtype, M, N, K, cus)
    T = (M + 15) // 16
    ks, S = p['k_slice'], p['k_slices']
    assert ks % 64 == 0 and ks > 0 and (S - 1) * ks < K <= S * ks
    assert all((min(K, (s + 1) * ks) - s * ks) % 64 == 0 for s in range(S))
    G = p['row_groups']
    assert (G - 1) * 16 < N <= G * 16
    seen = []
    for x in range(p['grid_x']):
        mine = [g for q in range(x, (G + 3) // 4, p['grid_x']) for g in range(4 * q, min(4 * q + 4, G))]
        assert 0 < len(mine) <= p['groups_per_workgroup']
        seen += mine
    assert sorted(seen) == list(range(G))
    # four rings of 16 KB and the fp16 panel (the slice rounded up to the block of 256 elements)
    assert p['lds_bytes'] == 4 * 16384 + 16 * T * 2 * ((ks + 255) // 256 * 256) <= 160 * 1024
    assert p['workspace_bytes'] == S * G * T * 1024
    assert p['grid_x'] * S <= max(cus, S)
