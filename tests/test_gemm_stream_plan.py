"""tllm_gemm_stream_layout (no GPU): the plan of the weight-streaming SmoothQuant GEMM - K-slices, row groups, LDS, workspace."""
import ctypes

import pytest

from tensorrt_llm.plugin import capi


def layout(M, N, K, cus):
    lib = capi.load_library()
    p = capi.GemmParams(wtype=3, M=M, N=N, K=K)
    ws = ctypes.c_int64()
    v = [ctypes.c_int32() for _ in range(6)]
    rc = lib.tllm_gemm_stream_layout(ctypes.byref(p), cus, ctypes.byref(ws), *[ctypes.byref(x) for x in v])
    if rc:
        raise RuntimeError(capi.last_error())
    names = ('k_slices', 'k_slice', 'row_groups', 'groups_per_workgroup', 'grid_x', 'lds_bytes')
    return dict(zip(names, (int(x.value) for x in v)), workspace_bytes=int(ws.value))


SHAPES_7B = [(12288, 4096), (4096, 4096), (11008, 4096), (4096, 11008)]


@pytest.mark.parametrize('M', [9, 16, 17, 33, 48, 64])
@pytest.mark.parametrize('N,K,cus', [(n, k, 256) for n, k in SHAPES_7B] + [(16, 64, 256), (40, 192, 304), (16424, 64, 256),
                                                                           (16, 8768, 4), (296, 2368, 64), (4096, 11008, 0)])
def test_the_plan(M, N, K, cus):
    p = layout(M, N, K, cus)
    T = (M + 15) // 16
    # the K-slices tile [0, K) exactly once, in multiples of 64
    ks, S = p['k_slice'], p['k_slices']
    assert ks % 64 == 0 and ks > 0 and (S - 1) * ks < K <= S * ks
    assert all((min(K, (s + 1) * ks) - s * ks) % 64 == 0 for s in range(S))
    # the row groups cover [0, N) exactly once: workgroup x walks the quads x, x + grid_x, ..
    G = p['row_groups']
    assert (G - 1) * 16 < N <= G * 16
    seen = []
    for x in range(p['grid_x']):
        mine = [g for q in range(x, (G + 3) // 4, p['grid_x']) for g in range(4 * q, min(4 * q + 4, G))]
        assert 0 < len(mine) <= p['groups_per_workgroup']
        seen += mine
    assert sorted(seen) == list(range(G))
    # the panel (rows of the bucket, the slice rounded up to the DMA block, 16 bytes of pitch) and the rings fit the LDS
    assert p['lds_bytes'] == 4 * 4 * 4096 + 16 * T * ((ks + 255) // 256 * 256 + 16) <= 160 * 1024
    assert p['workspace_bytes'] == S * G * T * 1024
    # one workgroup per CU at the most
    assert p['grid_x'] * S <= max(cus or 256, S)
