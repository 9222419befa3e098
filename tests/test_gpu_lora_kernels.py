"""The two LoRA launches (csrc/kernels/lora.hip) through tllm_lora_shrink / tllm_lora_expand against tensorrt_llm/runtime/lora_ref.py
in float64: K in {64, 264, 4096, 11008}, r in {8, 16, 64}, M in {1, 3, 8, 9, 40} (both regimes: M <= 8 and beyond), one, two and
three segments (256, 64, 64 among them), column counts that are no multiple of a workgroup's 2048 / r columns, both prologues,
three adapters mixed over the rows with rows of none between them.

The x rows of the rows of none are NaN, their t and y rows sentinels: nothing of them may move and no NaN may reach another row.

Bounds (the form of tests/test_gpu_gemv_instances.py):
  t   |t - t_ref| <= K 2^-24 sum_k |A||xh|: K fp32 roundings of partial sums that never exceed sum |A||xh| (v_dot2 products are
      exact).  Under the RMSNorm prologue xh is within 2 fp16 ulp of the float64 oracle's (as that file holds the GEMV's prologue
      to), which adds sum_k |A_k| 2 ulp16(xh_k).
  y   within 0.5 fp16 ulp of the exact y + s B t_ref, plus the propagated bound of t, s sum_j |B_nj| tb_j.  That much is the
      bound as the feature's specification words it.  Two derived terms WIDEN it here, by about 1e-6 relative against the 1e-3 of
      the ulp term: d also counts the expand's own fp32 evaluation - r + 2 roundings at 2^-24 of values no larger than
      |y| + s sum_j |B_nj||t_j| - and the ulp is taken at |exact| + d, not at |exact|.  Without them the bound is unsound at a
      rounding tie and at a binade edge: a result that is off by one fp32 rounding may legitimately round to the other fp16
      neighbour."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import gemv_oracle as GO
from tensorrt_llm.plugin import capi
from tensorrt_llm.runtime import lora_ref as LR

pytestmark = pytest.mark.gpu
PRO_NONE, PRO_RMSNORM = 0, 1
NADAPT = 3


class ShrinkParams(ctypes.Structure):
    """tllm_lora_shrink_params_t"""
    _fields_ = [('M', ctypes.c_int32), ('K', ctypes.c_int32), ('R', ctypes.c_int32), ('pro', ctypes.c_int32), ('x', ctypes.c_void_p),
                ('ldx', ctypes.c_int64), ('gamma', ctypes.c_void_p), ('eps', ctypes.c_float), ('row_adapter', ctypes.c_void_p),
                ('table', ctypes.c_void_p), ('num_adapters', ctypes.c_int32), ('t', ctypes.c_void_p)]


class ExpandParams(ctypes.Structure):
    """tllm_lora_expand_params_t"""
    _fields_ = [('M', ctypes.c_int32), ('r', ctypes.c_int32), ('nseg', ctypes.c_int32), ('seg_n', ctypes.c_int32 * 3),
                ('seg_y', ctypes.c_void_p * 3), ('seg_ldy', ctypes.c_int64 * 3), ('t', ctypes.c_void_p), ('row_adapter', ctypes.c_void_p),
                ('table', ctypes.c_void_p), ('num_adapters', ctypes.c_int32)]


@pytest.fixture(scope='module')
def lib():
    lib = capi.load_library()
    lib.tllm_lora_shrink.argtypes = [ctypes.POINTER(ShrinkParams), ctypes.c_void_p]
    lib.tllm_lora_shrink.restype = ctypes.c_int32
    lib.tllm_lora_expand.argtypes = [ctypes.POINTER(ExpandParams), ctypes.c_void_p]
    lib.tllm_lora_expand.restype = ctypes.c_int32
    return lib


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def table(As, Bs, scales):
    """device records {a, b, scale, reserved} of 24 bytes"""
    rec = np.zeros(len(As), np.dtype([('a', np.uint64), ('b', np.uint64), ('scale', np.float32), ('reserved', np.int32)]))
    for i, (a, b, s) in enumerate(zip(As, Bs, scales)):
        rec[i] = (a.data_ptr(), b.data_ptr(), s, 0)
    assert rec.itemsize == 24
    return dev(rec.view(np.uint8))


# (M, K, r, segments, prologue)
CASES = [
    (1, 64, 8, (40, ), PRO_NONE),
    (3, 264, 16, (72, 57), PRO_RMSNORM),
    (8, 4096, 16, (256, 64, 64), PRO_RMSNORM),
    (8, 11008, 8, (4100, ), PRO_NONE),
    (9, 11008, 64, (200, ), PRO_NONE),
    (9, 64, 8, (256, 64, 64), PRO_RMSNORM),
    (40, 4096, 8, (256, 64, 64), PRO_NONE),
    (40, 264, 64, (130, 70), PRO_RMSNORM),
    (3, 4096, 64, (33, ), PRO_NONE),
]


def row_map(M, seed):
    """three adapters mixed over the rows, every third row or so on none; at least one row on an adapter"""
    r = np.random.default_rng(seed)
    rows = r.integers(-1, NADAPT, M).astype(np.int32)
    rows[r.integers(0, M)] = r.integers(0, NADAPT)
    if M >= 3:
        rows[(np.flatnonzero(rows >= 0)[0] + 1) % M] = -1
    return rows


@pytest.mark.parametrize('M,K,r,segs,pro', CASES, ids=[f'M{c[0]}-K{c[1]}-r{c[2]}-seg{len(c[3])}-pro{c[4]}' for c in CASES])
def test_shrink_and_expand_against_the_float64_restatement(lib, M, K, r, segs, pro):
    rng = np.random.default_rng(M * 131 + K + r)
    nseg, N, R = len(segs), sum(segs), len(segs) * r
    rows = row_map(M, M + K)
    on = rows >= 0
    x = (1.3 * rng.standard_normal((M, K))).astype(np.float16)
    gamma = rng.uniform(0.5, 1.5, K).astype(np.float16)
    As = [(rng.standard_normal((R, K)) / np.sqrt(K)).astype(np.float16) for _ in range(NADAPT)]
    Bs = [(rng.standard_normal((N, r)) * 0.05).astype(np.float16) for _ in range(NADAPT)]
    scales = [2.0, 0.5, 1.25]
    y0 = rng.standard_normal((M, N)).astype(np.float16)
    # ---- reference
    xh = np.asarray(GO.rmsnorm(x, gamma, 1e-6), np.float16) if pro == PRO_RMSNORM else x
    t_ref = LR.shrink(xh, As, rows)
    # ---- device: NaN x rows, sentinel t and y rows where no adapter is selected
    xd = x.copy()
    xd[~on] = np.nan
    y_in = y0.copy()
    y_in[~on] = np.float16(-7.5)
    ldy = N + 8  # an interior view: the columns behind N must not move either
    ybuf = np.full((M, ldy), np.float16(3.25))
    ybuf[:, :N] = y_in
    t_in = np.full((M, R), np.float32(12345.0))
    d_x, d_g, d_rows = dev(xd), dev(gamma), dev(rows)
    d_A, d_B = [dev(a) for a in As], [dev(b) for b in Bs]
    d_tab = table(d_A, d_B, scales)
    st = torch.cuda.current_stream().cuda_stream

    def launch():
        d_t, d_y = dev(t_in), dev(ybuf)
        sp = ShrinkParams(M=M, K=K, R=R, pro=pro, x=d_x.data_ptr(), ldx=K, gamma=d_g.data_ptr(), eps=1e-6,
                          row_adapter=d_rows.data_ptr(), table=d_tab.data_ptr(), num_adapters=NADAPT, t=d_t.data_ptr())
        assert lib.tllm_lora_shrink(ctypes.byref(sp), st) == 0, capi.last_error()
        ep = ExpandParams(M=M, r=r, nseg=nseg, t=d_t.data_ptr(), row_adapter=d_rows.data_ptr(), table=d_tab.data_ptr(),
                          num_adapters=NADAPT)
        off = 0
        for g, n in enumerate(segs):
            ep.seg_n[g], ep.seg_y[g], ep.seg_ldy[g] = n, d_y.data_ptr() + 2 * off, ldy
            off += n
        assert lib.tllm_lora_expand(ctypes.byref(ep), st) == 0, capi.last_error()
        torch.cuda.synchronize()
        return d_t.cpu().numpy(), d_y.cpu().numpy()

    t_got, y_got = launch()
    # ---- rows of none: nothing moved
    np.testing.assert_array_equal(t_got[~on], t_in[~on])
    np.testing.assert_array_equal(y_got[~on].view(np.uint16), ybuf[~on].view(np.uint16))
    np.testing.assert_array_equal(y_got[:, N:].view(np.uint16), ybuf[:, N:].view(np.uint16))
    assert np.isfinite(t_got[on]).all() and np.isfinite(y_got[on]).all()
    # ---- t
    tb = np.zeros((M, R))
    for m in np.flatnonzero(on):
        a = np.abs(As[rows[m]].astype(np.float64))
        tb[m] = K * 2.0 ** -24 * (a @ np.abs(xh[m].astype(np.float64)))
        if pro == PRO_RMSNORM:
            tb[m] += a @ (2 * GO.ulp16(xh[m]))
    worst_t = float((np.abs(t_got[on] - t_ref[on]) / np.maximum(tb[on], 1e-30)).max())
    print(f'shrink: worst error {worst_t:.3f} of the bound')
    assert worst_t <= 1.0
    # ---- y
    exact = y_in.astype(np.float64) + LR.delta(t_ref, Bs, scales, list(segs), rows)
    seg = LR.segment_of(list(segs))
    cols = seg[:, None] * r + np.arange(r)[None, :]
    bound = np.zeros((M, N))
    for m in np.flatnonzero(on):
        b, s = np.abs(Bs[rows[m]].astype(np.float64)), scales[rows[m]]
        prop = s * np.einsum('nj,nj->n', b, tb[m][cols])
        mag = np.abs(y_in[m].astype(np.float64)) + s * np.einsum('nj,nj->n', b, np.abs(t_ref[m])[cols])
        d = prop + (r + 2) * 2.0 ** -24 * mag
        bound[m] = 0.5 * GO.ulp16(np.abs(exact[m]) + d) + d
    worst_y = float((np.abs(y_got[on][:, :N].astype(np.float64) - exact[on]) / bound[on]).max())
    print(f'expand: worst error {worst_y:.3f} of the bound')
    assert worst_y <= 1.0
    # ---- a second launch on the same inputs: the same bits
    t2, y2 = launch()
    np.testing.assert_array_equal(t2.view(np.uint32), t_got.view(np.uint32))
    np.testing.assert_array_equal(y2.view(np.uint16), y_got.view(np.uint16))


def test_launchers_refuse_what_they_cannot_run(lib):
    x = torch.zeros(8, 64, dtype=torch.float16, device='cuda')
    rows = torch.zeros(8, dtype=torch.int32, device='cuda')
    t = torch.zeros(8, 8, dtype=torch.float32, device='cuda')
    A, B = torch.zeros(8, 64, dtype=torch.float16, device='cuda'), torch.zeros(40, 8, dtype=torch.float16, device='cuda')
    tab = table([A], [B], [1.0])
    ok = dict(M=8, K=64, R=8, pro=PRO_NONE, x=x.data_ptr(), ldx=64, eps=1e-6, row_adapter=rows.data_ptr(), table=tab.data_ptr(),
              num_adapters=1, t=t.data_ptr())
    for bad in (dict(K=60), dict(num_adapters=9), dict(pro=2), dict(pro=PRO_RMSNORM), dict(M=0), dict(ldx=60)):
        assert lib.tllm_lora_shrink(ctypes.byref(ShrinkParams(**dict(ok, **bad))), None) != 0 and capi.last_error()
    ep = ExpandParams(M=8, r=12, nseg=1, t=t.data_ptr(), row_adapter=rows.data_ptr(), table=tab.data_ptr(), num_adapters=1)
    ep.seg_n[0], ep.seg_y[0], ep.seg_ldy[0] = 40, x.data_ptr(), 64
    assert lib.tllm_lora_expand(ctypes.byref(ep), None) != 0 and 'r 12' in capi.last_error()
    torch.cuda.synchronize()
