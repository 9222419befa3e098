"""tllm_attention_decode_grouped (csrc/kernels/mmha_gqa_mfma.hip: the query heads of a K/V head as MFMA columns) against
tensorrt_llm/runtime/gqa_ref.py::decode, the float64-backed oracle the head-mapped kernel is held to - with the inputs, the bounds
and the checks of tests/test_gpu_gqa_attention.py: context atol 2e-3, nothing but slot L of the cache changed, V bytes exact, K within
check_appended_rows.  B = 2 with the padded, masked second prompt of decode_case."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import as_f32
from tensorrt_llm.plugin import capi
from test_gpu_gqa_attention import Call, check_appended_rows, decode_case, decode_reference, dev_i32

pytestmark = pytest.mark.gpu

KINDS = ['fp16', 'int8', 'fp8']
# G = 2 at head size 64; G = 4; G = 3 (padding columns); a full tile; two column tiles
SHAPES = [(4, 2, 64), (8, 2, 128), (6, 2, 128), (16, 1, 128), (32, 1, 128)]


def grouped_call(lib, kind, H, Hkv, Dh, L, case, **kw):
    B, smax, max_in, in_len, masked, cache_np, qkv = case
    c = Call(lib, kind, B, H, Hkv, Dh, smax, max_input_len=max_in, **kw)
    c.p.timestep = L
    c.set('qkv', qkv)
    cache = c.set('kv_cache', torch.from_numpy(cache_np.copy()).cuda())
    c.set('sequence_length', dev_i32([L] * B))
    c.set('input_lengths', dev_i32(in_len))
    c.set('masked_tokens', dev_i32(masked))
    out = c.set('out', torch.full((B, H * Dh), 7.0, dtype=torch.float16, device='cuda'))
    return c, cache, out


def run_grouped(lib, c):
    ws = torch.empty(lib.tllm_attention_workspace_size(ctypes.byref(c.p), 0), dtype=torch.uint8, device='cuda')
    c.p.workspace = ws.data_ptr()
    rc = lib.tllm_attention_decode_grouped(ctypes.byref(c.p), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def check_grouped(lib, kind, H, Hkv, Dh, L, seed, **force):
    case = decode_case(kind, H, Hkv, Dh, L, seed)
    _, _, max_in, in_len, masked, cache_np, qkv = case
    ref, ref_cache = decode_reference(kind, qkv, cache_np, L, in_len, max_in, masked, H, Hkv, Dh)
    c, cache, out = grouped_call(lib, kind, H, Hkv, Dh, L, case, **force)
    lay = c.layout()
    assert run_grouped(lib, c) == 0, capi.last_error()
    what = f'{kind} H={H} Hkv={Hkv} Dh={Dh} L={L} layout={lay}'
    print(f'{what}: max |ctx - ref| = {np.abs(as_f32(out) - ref).max():.3e}')
    np.testing.assert_allclose(as_f32(out), ref, atol=2e-3, rtol=0, err_msg=what)
    check_appended_rows(kind, cache.cpu().numpy(), ref_cache, cache_np, L, what)
    return lay


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('H,Hkv,Dh', SHAPES)
@pytest.mark.parametrize('L', [1, 17, 63, 64, 65, 1023])
def test_grouped_decode_vs_gqa_ref(lib, kind, H, Hkv, Dh, L):
    check_grouped(lib, kind, H, Hkv, Dh, L, 100 + L)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('edge', [-1, 0, 1])
def test_grouped_decode_at_a_split_boundary(lib, kind, edge):
    """The new token in the last slot of a split, the first slot of the next one (a split that holds the new token alone) and one
    further: the split that owns slot L appends, once per K/V head."""
    H, Hkv, Dh = 8, 2, 128
    tchunk, nsplit, _, merged = Call(lib, kind, 2, H, Hkv, Dh, 1152).layout()
    assert nsplit > 2 and merged == 1
    check_grouped(lib, kind, H, Hkv, Dh, tchunk + edge, 500 + edge)


@pytest.mark.parametrize('kind', KINDS)
def test_grouped_decode_on_the_combine_path(lib, kind):
    """L = 4000 with the finest split (more splits than the in-launch merge takes: partial launch + combine launch; seed 100 + L as
    test_gpu_gqa_attention.test_decode_on_the_combine_path argues), and the combine launch forced at L = 300."""
    lay = check_grouped(lib, kind, 8, 2, 128, 4000, 100 + 4000, rows_per_group=4)
    assert lay[1] > 16 and lay[3] == 0, lay
    lay = check_grouped(lib, kind, 8, 2, 128, 300, 701, combine_launch=1)
    assert lay[1] <= 16 and lay[3] == 0, lay


@pytest.mark.parametrize('H,Hkv,Dh,kw,field', [
    (8, 8, 128, {}, 'num_kv_heads'),
    (8, 2, 32, {}, 'head_size'),
    (8, 2, 128, dict(beam_width=2), 'beam_width'),
    (8, 2, 128, dict(tokens_per_block=16, max_blocks_per_seq=72), 'block_pointers'),
], ids=['G1', 'Dh32', 'beam2', 'paged'])
def test_what_the_grouped_kernel_does_not_serve_is_refused_by_name(lib, H, Hkv, Dh, kw, field):
    case = decode_case('fp16', H, Hkv, Dh, 17, 5)
    c, cache, out = grouped_call(lib, 'fp16', H, Hkv, Dh, 17, case, **kw)
    if field == 'beam_width':
        c.set('cache_indirection', dev_i32(np.zeros((2, case[1]), np.int32)))
    if field == 'block_pointers':
        c.set('block_pointers', torch.full((2, 2, 72), cache.data_ptr(), dtype=torch.int64, device='cuda'))
    assert run_grouped(lib, c) != 0
    assert field in capi.last_error(), capi.last_error()
    assert torch.equal(out, torch.full_like(out, 7.0)) and np.array_equal(cache.cpu().numpy(), case[5])
