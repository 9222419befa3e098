"""Grouped-query attention on the GPU: the session-free entry points tllm_attention_decode / tllm_attention_context
(include/tllm_runtime_api.h) against tensorrt_llm/runtime/gqa_ref.py - the multi-head oracle on expanded inputs.

Tolerances are the project's own, taken from the reference's plugin test where tests/test_gpu_plugins.py takes them: decode output
atol 2e-3, context output atol 5e-3; the appended K within 1 fp16 ulp (atol 2e-4, rtol 2e-3) / 1 int8 LSB / 1 E4M3 code with at
least 98 % of the bytes equal (RoPE uses fma); V bytes exact against kv_store / kv_store_fp8 (no RoPE precedes them); nothing but
slot L of the cache may change in a generation step.  Every query tile in {1, 2, 4, 8} that divides the group is forced, and the
launcher's default is run as well; a forced tile that does not divide the group is an error and launches nothing."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import HostTensor, as_f32, f32, h, i8, i32, make_plugin, run_plugin
from oracle import llama_oracle as O
from tensorrt_llm.plugin import capi
from tensorrt_llm.runtime import gqa_ref as G
from tensorrt_llm.runtime import kv_fp8_ref as F8

pytestmark = pytest.mark.gpu

KV_SCALE = 0.05  # values ~N(0, 1): +-6 sigma covered by 127 * 0.05
KINDS = {'fp16': (capi.HALF, np.float16, torch.float16), 'int8': (capi.INT8, np.int8, torch.int8),
         'fp8': (capi.FP8, np.uint8, torch.uint8)}


def store(kind, x):
    if kind == 'fp16':
        return np.asarray(x, np.float32).astype(np.float16)
    if kind == 'int8':
        return O.rni_sat_i8(np.asarray(x, np.float32) * np.float32(1.0 / KV_SCALE))
    return F8.kv_store_fp8(x, 1.0 / KV_SCALE)


def scales_of(kind):
    return None if kind == 'fp16' else (1.0 / KV_SCALE, KV_SCALE)


def tiles_of(group):
    return [t for t in (1, 2, 4, 8) if group % t == 0]


def dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


class Call:
    """One tllm_attention_params_t with the tensors it points to kept alive."""

    def __init__(self, lib, kind, B, H, Hkv, Dh, smax, **kw):
        self.lib = lib
        self.keep = []
        self.p = capi.AttentionParams(batch=B, num_heads=H, num_kv_heads=Hkv, head_size=Dh, rotary_dim=Dh, neox=1, q_scaling=1.0,
                                      kv_cache_type=KINDS[kind][0], max_seq_len=smax, timestep=-1, **kw)
        sc = scales_of(kind)
        if sc:
            self.set('kv_scale_orig_quant', torch.tensor([sc[0]], dtype=torch.float32, device='cuda'))
            self.set('kv_scale_quant_orig', torch.tensor([sc[1]], dtype=torch.float32, device='cuda'))

    def set(self, name, tensor):
        self.keep.append(tensor)
        setattr(self.p, name, tensor.data_ptr())
        return tensor

    def layout(self):
        a = [ctypes.c_int32() for _ in range(4)]
        rc = self.lib.tllm_attention_decode_layout(ctypes.byref(self.p), *[ctypes.byref(x) for x in a])
        assert rc == 0, capi.last_error()
        return [x.value for x in a]  # tchunk, nsplit, q_tile, in_launch_merge

    def run(self, is_context=False):
        ws = torch.empty(max(self.lib.tllm_attention_workspace_size(ctypes.byref(self.p), 1 if is_context else 0), 16),
                         dtype=torch.uint8, device='cuda')
        self.p.workspace = ws.data_ptr()
        fn = self.lib.tllm_attention_context if is_context else self.lib.tllm_attention_decode
        rc = fn(ctypes.byref(self.p), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc


def decode_case(kind, H, Hkv, Dh, L, seed, smax=None, B=2):
    """The padded second prompt of test_mmha_decode_vs_oracle, on an [B, 2, Hkv, Smax, Dh] cache (B = 1: the first prompt alone)."""
    r = np.random.default_rng(seed)
    if smax is None:
        smax = 1152 if L < 1152 else (2048 if L < 2048 else 4096)
    max_in = max(L - 3, 1) if L > 4 else L
    in_len = [max_in, max(max_in // 2, 1)][:B]
    masked = np.zeros((B, smax), dtype=np.int32)
    masked[1:, in_len[-1]:max_in] = 1
    past = r.standard_normal((B, 2, Hkv, smax, Dh)).astype(np.float32)
    past[:, :, :, L:] = 0
    cache_np = store(kind, past)
    qkv = h(r.standard_normal((B, (H + 2 * Hkv) * Dh)))
    return B, smax, max_in, in_len, masked, cache_np, qkv


def decode_reference(kind, qkv, cache_np, L, in_len, max_in, masked, H, Hkv, Dh):
    ref_cache = cache_np.copy()
    sc = scales_of(kind)
    ref = G.decode(as_f32(qkv), ref_cache, [L] * qkv.shape[0], in_len, max_in, L, H, Hkv, Dh, Dh, True, 1.0, masked,
                   sc[0] if sc else None, sc[1] if sc else None)
    return ref, ref_cache


def code_index(c):
    c = np.asarray(c).astype(np.int32)
    return np.where(c & 0x80, -(c & 0x7f), c & 0x7f)


def check_appended_rows(kind, got, ref_cache, before, L, what):
    """Nothing but slot L changed; V bytes exact; K within the tolerances of tests/test_gpu_plugins.py:400-410."""
    keep = np.ones(got.shape[3], dtype=bool)
    keep[L] = False
    np.testing.assert_array_equal(got[:, :, :, keep], before[:, :, :, keep], err_msg=what)
    np.testing.assert_array_equal(got[:, 1, :, L], ref_cache[:, 1, :, L], err_msg=what)
    gk, rk = got[:, 0, :, L], ref_cache[:, 0, :, L]
    if kind == 'fp16':
        np.testing.assert_allclose(gk.astype(np.float32), rk.astype(np.float32), atol=2e-4, rtol=2e-3, err_msg=what)
    else:
        d = np.abs(gk.astype(np.int32) - rk.astype(np.int32)) if kind == 'int8' else np.abs(code_index(gk) - code_index(rk))
        assert d.max() <= 1 and np.mean(d == 0) > 0.98, what


def run_decode_tiles(lib, kind, H, Hkv, Dh, L, seed, smax=None, **force):
    B, smax, max_in, in_len, masked, cache_np, qkv = decode_case(kind, H, Hkv, Dh, L, seed, smax)
    ref, ref_cache = decode_reference(kind, qkv, cache_np, L, in_len, max_in, masked, H, Hkv, Dh)
    seen = []
    for tile in [0] + tiles_of(H // Hkv):
        c = Call(lib, kind, B, H, Hkv, Dh, smax, max_input_len=max_in, q_heads_per_workgroup=tile, **force)
        c.p.timestep = L
        c.set('qkv', qkv)
        cache = c.set('kv_cache', torch.from_numpy(cache_np.copy()).cuda())
        c.set('sequence_length', dev_i32([L] * B))
        c.set('input_lengths', dev_i32(in_len))
        c.set('masked_tokens', dev_i32(masked))
        out = c.set('out', torch.full((B, H * Dh), float('nan'), dtype=torch.float16, device='cuda'))
        lay = c.layout()
        assert tile == 0 or lay[2] == tile
        assert c.run() == 0, capi.last_error()
        what = f'{kind} H={H} Hkv={Hkv} Dh={Dh} L={L} tile={tile} layout={lay}'
        err = np.abs(as_f32(out) - ref).max()
        print(f'{what}: max |ctx - ref| = {err:.3e}')
        np.testing.assert_allclose(as_f32(out), ref, atol=2e-3, rtol=0, err_msg=what)
        check_appended_rows(kind, cache.cpu().numpy(), ref_cache, cache_np, L, what)
        seen.append(lay)
    return seen


SHAPES = [(8, 2, 128), (8, 1, 128), (4, 2, 64), (6, 2, 128), (16, 1, 128), (32, 8, 128)]


@pytest.mark.parametrize('kind', ['fp16', 'int8', 'fp8'])
@pytest.mark.parametrize('H,Hkv,Dh', SHAPES)
@pytest.mark.parametrize('L', [1, 17, 1023, 2047])
def test_decode_every_tile_vs_gqa_ref(lib, kind, H, Hkv, Dh, L):
    run_decode_tiles(lib, kind, H, Hkv, Dh, L, 100 + L)


@pytest.mark.parametrize('kind', ['fp16', 'int8', 'fp8'])
@pytest.mark.parametrize('edge', [-1, 0, 1])
def test_decode_at_a_split_boundary(lib, kind, edge):
    """The new token in the last slot of a split, the first slot of the next one, and one further (TCHUNK of the instance the
    launch runs, read from the layout query): the split that owns slot L appends, once per K/V head."""
    H, Hkv, Dh, smax = 8, 2, 128, 1152
    probe = Call(lib, kind, 2, H, Hkv, Dh, smax)
    tchunk, nsplit, _, merged = probe.layout()
    assert nsplit > 2 and merged == 1
    run_decode_tiles(lib, kind, H, Hkv, Dh, tchunk + edge, 500 + edge)


@pytest.mark.parametrize('kind', ['fp16', 'int8', 'fp8'])
def test_decode_on_the_combine_path(lib, kind):
    """L = 4000 with the finest split: 64 splits, more than the in-launch merge takes - partial launch + combine launch.
    Inputs by the seed rule of the other decode cases (100 + L).  Beyond 2048 positions the fp32 RoPE angle is only defined to one
    ulp (2.4e-4 rad at 4000: the host libm's powf, which fills the kernels' table, and numpy's, which the oracle calls, differ by
    that at a few frequencies - test_context_attention_vs_oracle allows 8e-4 there), so a rotated key with a large partner can
    miss the 2e-4 slot tolerance through the table alone: seed 700 did, in 1 of 512 elements (3.05e-4 at |k| = 0.036, frequency 10
    of kv head 1), reproduced on the host from the two tables without the kernel; 0 of 60 further seeds do."""
    for lay in run_decode_tiles(lib, kind, 8, 2, 128, 4000, 100 + 4000, rows_per_group=4):
        assert lay[1] > 16 and lay[3] == 0, lay
    # and the combine launch forced where the in-launch merge would serve
    for lay in run_decode_tiles(lib, kind, 8, 2, 128, 300, 701, combine_launch=1):
        assert lay[1] <= 16 and lay[3] == 0, lay


@pytest.mark.parametrize('H,Hkv,tile', [(8, 2, 8), (6, 2, 2), (6, 2, 4), (4, 4, 2), (8, 2, 3), (16, 1, 16)])
def test_a_forced_tile_that_does_not_divide_the_group_launches_nothing(lib, H, Hkv, tile):
    B, smax, max_in, in_len, masked, cache_np, qkv = decode_case('fp16', H, Hkv, 128, 17, 5)
    c = Call(lib, 'fp16', B, H, Hkv, 128, smax, max_input_len=max_in, q_heads_per_workgroup=tile)
    c.p.timestep = 17
    c.set('qkv', qkv)
    cache = c.set('kv_cache', torch.from_numpy(cache_np.copy()).cuda())
    c.set('sequence_length', dev_i32([17] * B))
    c.set('input_lengths', dev_i32(in_len))
    out = c.set('out', torch.full((B, H * 128), 7.0, dtype=torch.float16, device='cuda'))
    assert c.run() != 0
    msg = capi.last_error()
    assert 'q_heads_per_workgroup' in msg and str(tile) in msg, msg
    assert torch.equal(out, torch.full_like(out, 7.0)) and np.array_equal(cache.cpu().numpy(), cache_np)


@pytest.mark.parametrize('bad', [(8, 3), (4, 8), (8, -1)])
def test_a_kv_head_count_that_does_not_divide_is_refused(lib, bad):
    c = Call(lib, 'fp16', 1, bad[0], bad[1], 128, 64)
    a = [ctypes.c_int32() for _ in range(4)]
    assert lib.tllm_attention_decode_layout(ctypes.byref(c.p), *[ctypes.byref(x) for x in a]) != 0
    assert 'num_kv_heads' in capi.last_error()


@pytest.mark.parametrize('kind', ['fp16', 'int8'])
def test_decode_with_beam_indirection(lib, kind):
    """W = 3 hypotheses, G = 4: sequence b * W + k reads time step t from the rows of sequence b * W + cache_indirection[b, k, t];
    the new token's K/V go to the sequence's own rows, once per K/V head."""
    r = np.random.default_rng(300)
    H, Hkv, Dh, L, W, batch, smax = 8, 2, 128, 200, 3, 2, 1152
    B = batch * W
    max_in = L - 3
    in_len = np.repeat([max_in, max_in // 2], W).tolist()
    masked = np.zeros((B, smax), dtype=np.int32)
    masked[W:, in_len[W]:max_in] = 1
    past = r.standard_normal((B, 2, Hkv, smax, Dh)).astype(np.float32)
    past[:, :, :, L:] = 0
    cache_np = store(kind, past)
    ci = r.integers(0, W, (batch, W, smax)).astype(np.int32)
    qkv = h(r.standard_normal((B, (H + 2 * Hkv) * Dh)))
    eff = np.empty_like(cache_np)  # per sequence, the cache its indirection row selects
    for bb in range(B):
        b, k = divmod(bb, W)
        eff[bb] = cache_np[b * W + ci[b, k], :, :, np.arange(smax)].transpose(1, 2, 0, 3)
    ref, ref_cache = decode_reference(kind, qkv, eff, L, in_len, max_in, masked, H, Hkv, Dh)
    for tile in [0, 1, 2, 4]:
        c = Call(lib, kind, B, H, Hkv, Dh, smax, max_input_len=max_in, q_heads_per_workgroup=tile, beam_width=W)
        c.p.timestep = L
        c.set('qkv', qkv)
        cache = c.set('kv_cache', torch.from_numpy(cache_np.copy()).cuda())
        c.set('sequence_length', dev_i32([L] * B))
        c.set('input_lengths', dev_i32(in_len))
        c.set('masked_tokens', dev_i32(masked))
        c.set('cache_indirection', dev_i32(ci))
        out = c.set('out', torch.empty((B, H * Dh), dtype=torch.float16, device='cuda'))
        assert c.run() == 0, capi.last_error()
        np.testing.assert_allclose(as_f32(out), ref, atol=2e-3, rtol=0, err_msg=f'tile {tile}')
        check_appended_rows(kind, cache.cpu().numpy(), ref_cache, cache_np, L, f'beam tile {tile}')  # siblings' rows untouched


def block_table(pool, B, M, mapped, blk_bytes):
    """int64 [B, 2, M]: logical block j of sequence b is pool block j * B + b; blocks at or beyond `mapped` are not handed out."""
    table = np.zeros((B, 2, M), np.int64)
    for b in range(B):
        for j in range(mapped):
            for kv in range(2):
                table[b, kv, j] = pool.data_ptr() + ((j * B + b) * 2 + kv) * blk_bytes
    return table


def pool_to_linear(pool_np, B, M, mapped, T):
    out = np.zeros((B, 2, pool_np.shape[2], M * T, pool_np.shape[4]), pool_np.dtype)
    for b in range(B):
        for j in range(mapped):
            out[b, :, :, j * T:(j + 1) * T] = pool_np[j * B + b]
    return out


@pytest.mark.parametrize('kind', ['fp16', 'fp8'])
def test_decode_with_the_paged_cache(lib, kind):
    """G = 4, blocks [Hkv, tokens_per_block, Dh], one trailing logical block not handed out (table entry 0)."""
    r = np.random.default_rng(400)
    H, Hkv, Dh, B, L, T = 8, 2, 128, 2, 1023, 16
    mapped = L // T + 1  # the block of slot L is mapped
    M = mapped + 1
    smax = M * T
    max_in = L - 3
    in_len = [max_in, max_in // 2]
    masked = np.zeros((B, smax), dtype=np.int32)
    masked[1, in_len[1]:max_in] = 1
    pool_np = store(kind, r.standard_normal((B * mapped, 2, Hkv, T, Dh)))
    lin = pool_to_linear(pool_np, B, M, mapped, T)
    lin[:, :, :, L:] = 0
    for b in range(B):  # the same zeros in the pool
        for j in range(mapped):
            pool_np[j * B + b] = lin[b, :, :, j * T:(j + 1) * T]
    qkv = h(r.standard_normal((B, (H + 2 * Hkv) * Dh)))
    ref, ref_cache = decode_reference(kind, qkv, lin, L, in_len, max_in, masked, H, Hkv, Dh)
    for tile in [0, 1, 4]:
        pool = torch.from_numpy(pool_np.copy()).cuda()
        table = block_table(pool, B, M, mapped, Hkv * T * Dh * pool.element_size())
        c = Call(lib, kind, B, H, Hkv, Dh, smax, max_input_len=max_in, q_heads_per_workgroup=tile, tokens_per_block=T,
                 max_blocks_per_seq=M)
        c.p.timestep = L
        c.set('kv_cache', pool)  # the pool: where the rows of the unmapped block are read from (and masked)
        c.set('qkv', qkv)
        c.set('block_pointers', torch.from_numpy(table).cuda())
        c.set('sequence_length', dev_i32([L] * B))
        c.set('input_lengths', dev_i32(in_len))
        c.set('masked_tokens', dev_i32(masked))
        out = c.set('out', torch.empty((B, H * Dh), dtype=torch.float16, device='cuda'))
        assert c.run() == 0, capi.last_error()
        np.testing.assert_allclose(as_f32(out), ref, atol=2e-3, rtol=0, err_msg=f'tile {tile}')
        got = pool_to_linear(pool.cpu().numpy(), B, M, mapped, T)
        check_appended_rows(kind, got, ref_cache, lin, L, f'paged tile {tile}')


# ------------------------------------------------------------------------------------------------------------ context
# (every context attention instance forced at small shapes, against a float64 oracle: tests/test_gpu_ctx_attn_instances.py)
def run_context(lib, kind, H, Hkv, Dh, S, in_len, qkv, smax, packed=False, pointers=None, T=0, M=0, pool=None):
    B = len(in_len)
    c = Call(lib, kind, B, H, Hkv, Dh, smax, seq=S, tokens_per_block=T, max_blocks_per_seq=M)
    c.set('input_lengths', dev_i32(in_len))
    if packed:
        x = c.set('qkv', torch.cat([qkv[b, :in_len[b]] for b in range(B)], dim=0).contiguous())
        c.set('cu_seqlens', dev_i32(np.concatenate([[0], np.cumsum(in_len)])))
        out = c.set('out', torch.full((x.shape[0], H * Dh), float('nan'), dtype=torch.float16, device='cuda'))
    else:
        c.set('qkv', qkv.clone())
        out = c.set('out', torch.full((B, S, H * Dh), float('nan'), dtype=torch.float16, device='cuda'))
    if pointers is not None:
        c.set('kv_cache', pool)
        c.set('block_pointers', pointers)
        cache = pool
    else:
        cache = c.set('kv_cache', torch.zeros((B, 2, Hkv, smax, Dh), dtype=KINDS[kind][2], device='cuda'))
    assert c.run(is_context=True) == 0, capi.last_error()
    return out, cache


def check_context_cache(kind, got, ref_cache, S):
    """The cache tolerance of test_context_attention_vs_oracle (S <= 2048)."""
    np.testing.assert_array_equal(got[:, 1], ref_cache[:, 1])  # V is never rotated
    if kind == 'fp16':
        np.testing.assert_allclose(got[:, 0].astype(np.float32), ref_cache[:, 0].astype(np.float32), atol=2e-4, rtol=2e-3)
    else:
        d = (np.abs(got[:, 0].astype(np.int32) - ref_cache[:, 0].astype(np.int32)) if kind == 'int8'
             else np.abs(code_index(got[:, 0]) - code_index(ref_cache[:, 0])))
        assert d.max() <= 1 and np.mean(d == 0) > 0.98


@pytest.mark.parametrize('kind', ['fp16', 'int8', 'fp8'])
# (32, 8, 128): at S = 300 the launcher pairs 64-query blocks (the 8-wave three-stage instance), at S = 1024 it runs the unpaired
# 128-query instance - the MFMA instances a 32-head model takes; (8, 2) and (4, 2) reach the wave-per-query and the narrow one
@pytest.mark.parametrize('H,Hkv,Dh,S', [(h, k, d, s) for (h, k, d) in ((8, 2, 128), (4, 2, 64)) for s in (1, 17, 128, 300)]
                         + [(32, 8, 128, 300), (32, 8, 128, 1024)])
def test_context_vs_gqa_ref(lib, kind, H, Hkv, Dh, S):
    r = np.random.default_rng(200 + S)
    B, smax = 2, S + 8
    in_len = [S, max(S // 2, 1)]  # half of sequence 1 is padding
    qkv = h(r.standard_normal((B, S, (H + 2 * Hkv) * Dh)))
    out, cache = run_context(lib, kind, H, Hkv, Dh, S, in_len, qkv, smax)
    ref_cache = np.zeros((B, 2, Hkv, smax, Dh), KINDS[kind][1])
    sc = scales_of(kind)
    ref, _ = G.context(as_f32(qkv), ref_cache, in_len, H, Hkv, Dh, Dh, True, 1.0, sc[0] if sc else None)
    err = np.abs(as_f32(out) - ref).max()
    print(f'context {kind} H={H} Hkv={Hkv} Dh={Dh} S={S}: max |ctx - ref| = {err:.3e}')
    np.testing.assert_allclose(as_f32(out), ref, atol=5e-3, rtol=0)
    check_context_cache(kind, cache.cpu().numpy(), ref_cache, S)


@pytest.mark.parametrize('kind', ['fp16', 'int8'])
def test_packed_context_equals_padded_bit_for_bit(lib, kind):
    r = np.random.default_rng(333)
    H, Hkv, Dh, S, B = 8, 2, 128, 200, 3
    smax = S + 8
    in_len = [S, S // 3, S // 2]
    qkv = h(r.standard_normal((B, S, (H + 2 * Hkv) * Dh)))
    out_pad, cache_pad = run_context(lib, kind, H, Hkv, Dh, S, in_len, qkv, smax)
    out_pk, cache_pk = run_context(lib, kind, H, Hkv, Dh, S, in_len, qkv, smax, packed=True)
    off = 0
    for b in range(B):
        assert torch.equal(out_pk[off:off + in_len[b]], out_pad[b, :in_len[b]]), b
        off += in_len[b]
    assert torch.equal(cache_pk, cache_pad)


def test_context_with_the_paged_cache(lib):
    r = np.random.default_rng(9)
    kind, H, Hkv, Dh, B, T, S = 'fp16', 8, 2, 128, 2, 16, 40
    in_len = [S, S // 2]
    mapped = S // T + 1
    M = mapped + 1  # one trailing logical block not handed out
    smax = M * T
    pool = torch.zeros((B * mapped, 2, Hkv, T, Dh), dtype=torch.float16, device='cuda')
    table = block_table(pool, B, M, mapped, Hkv * T * Dh * 2)
    qkv = h(r.standard_normal((B, S, (H + 2 * Hkv) * Dh)))
    out, _ = run_context(lib, kind, H, Hkv, Dh, S, in_len, qkv, smax, pointers=torch.from_numpy(table).cuda(), T=T, M=M, pool=pool)
    ref_cache = np.zeros((B, 2, Hkv, smax, Dh), np.float16)
    ref, _ = G.context(as_f32(qkv), ref_cache, in_len, H, Hkv, Dh, Dh)
    np.testing.assert_allclose(as_f32(out), ref, atol=5e-3, rtol=0)
    check_context_cache(kind, pool_to_linear(pool.cpu().numpy(), B, M, mapped, T), ref_cache, S)


# --------------------------------------------------------------------------------------------- no behaviour change
def attention_plugin(H, Dh, int8_kv):
    return make_plugin('GPTAttention', [
        ('num_heads', i32(H)), ('head_size', i32(Dh)), ('unidirectional', i32(1)), ('q_scaling', f32(1.0)),
        ('rotary_embedding_dim', i32(Dh)), ('neox_rotary_style', i8(1)),
        ('context_fmha_type', i8(0)), ('multi_block_mode', i8(0)), ('multi_query_mode', i8(0)),
        ('int8_kv_cache', i32(int8_kv)), ('fp8_kv_cache', i32(0)), ('remove_input_padding', i8(0)),
        ('mask_type', i32([1])), ('paged_kv_cache', i32(0)), ('type_id', i32([capi.HALF])), ('in_flight_batching', i32(0)),
    ])


def run_attention_plugin(p, qkv, cache, seq_len, past_len, is_context, masked, in_len, max_in, smax, scales):
    B = qkv.shape[0]
    out = torch.empty(qkv.shape[:-1] + (qkv.shape[-1] // 3, ), dtype=torch.float16, device='cuda')
    dummy = torch.zeros(max(max_in, B * smax), dtype=torch.int32, device='cuda')
    ins = [qkv, cache, dev_i32(seq_len), HostTensor([past_len, 1 if is_context else 0]), dev_i32(masked), dev_i32(in_len),
           dummy[:max_in], dummy[:B * smax].view(B, 1, smax)]
    if scales is not None:
        ins += [torch.tensor([scales[0]], dtype=torch.float32, device='cuda'),
                torch.tensor([scales[1]], dtype=torch.float32, device='cuda')]
    run_plugin(p, ins, [out, cache])
    return out


@pytest.mark.parametrize('kind', ['fp16', 'int8'])
@pytest.mark.parametrize('hkv', ['absent', 'H'])
@pytest.mark.parametrize('H,Dh,L', [(4, 128, 200), (32, 128, 1023), (4, 64, 4000)])
def test_decode_with_hkv_equal_to_h_is_the_plugin_bit_for_bit(lib, kind, hkv, H, Dh, L):
    B, smax, max_in, in_len, masked, cache_np, qkv = decode_case(kind, H, H, Dh, L, 900 + L)
    cache_a = torch.from_numpy(cache_np.copy()).cuda()
    out_a = run_attention_plugin(attention_plugin(H, Dh, int(kind == 'int8')), qkv[:, None].contiguous(), cache_a, [L] * B, L, False,
                                 masked, in_len, max_in, smax, scales_of(kind))
    c = Call(lib, kind, B, H, 0 if hkv == 'absent' else H, Dh, smax, max_input_len=max_in)
    c.p.timestep = L
    c.set('qkv', qkv)
    cache_b = c.set('kv_cache', torch.from_numpy(cache_np.copy()).cuda())
    c.set('sequence_length', dev_i32([L] * B))
    c.set('input_lengths', dev_i32(in_len))
    c.set('masked_tokens', dev_i32(masked))
    out_b = c.set('out', torch.empty((B, H * Dh), dtype=torch.float16, device='cuda'))
    assert c.run() == 0, capi.last_error()
    assert torch.equal(out_a[:, 0], out_b) and torch.equal(cache_a, cache_b)


# capacity -> (tchunk, nsplit, in_launch_merge) at head size 128: the last cache that takes 12 rows per lane group (8 splits), the
# first that takes 16; the last that merges inside the launch (16 splits of 16 rows), the first on the finest split + combine launch
PLAN_EDGES = {1536: (192, 8, 1), 1537: (256, 7, 1), 4096: (256, 16, 1), 4097: (64, 65, 0)}


@pytest.mark.parametrize('smax', sorted(PLAN_EDGES))
def test_plugin_and_entry_point_run_one_plan_at_the_rule_boundaries(lib, smax):
    """rows_per_group left open, the cache two slots short of full: the GPTAttention enqueue and tllm_attention_decode resolve the
    same split-KV plan - bit-identical context and appended row - and both stay within the decode tolerance of the oracle."""
    kind, H, Dh, L = 'fp16', 2, 128, smax - 2
    B, smax, max_in, in_len, masked, cache_np, qkv = decode_case(kind, H, H, Dh, L, 1300 + smax, smax, B=1)
    ref, ref_cache = decode_reference(kind, qkv, cache_np, L, in_len, max_in, masked, H, H, Dh)
    cache_a = torch.from_numpy(cache_np.copy()).cuda()
    out_a = run_attention_plugin(attention_plugin(H, Dh, 0), qkv[:, None].contiguous(), cache_a, [L] * B, L, False, masked, in_len,
                                 max_in, smax, None)
    c = Call(lib, kind, B, H, H, Dh, smax, max_input_len=max_in, rows_per_group=0)
    c.p.timestep = L
    c.set('qkv', qkv)
    cache_b = c.set('kv_cache', torch.from_numpy(cache_np.copy()).cuda())
    c.set('sequence_length', dev_i32([L] * B))
    c.set('input_lengths', dev_i32(in_len))
    c.set('masked_tokens', dev_i32(masked))
    out_b = c.set('out', torch.full((B, H * Dh), float('nan'), dtype=torch.float16, device='cuda'))
    lay = c.layout()
    assert (lay[0], lay[1], lay[3]) == PLAN_EDGES[smax], lay
    assert c.run() == 0, capi.last_error()
    assert torch.equal(out_a[:, 0], out_b) and torch.equal(cache_a, cache_b)
    what = f'capacity {smax} L={L} layout={lay}'
    print(f'{what}: max |ctx - ref| = {np.abs(as_f32(out_b) - ref).max():.3e}')
    np.testing.assert_allclose(as_f32(out_b), ref, atol=2e-3, rtol=0, err_msg=what)
    check_appended_rows(kind, cache_b.cpu().numpy(), ref_cache, cache_np, L, what)


@pytest.mark.parametrize('kind', ['fp16', 'int8'])
@pytest.mark.parametrize('H,Dh,S', [(4, 128, 90), (4, 64, 33), (32, 128, 300)])
def test_context_with_hkv_equal_to_h_is_the_plugin_bit_for_bit(lib, kind, H, Dh, S):
    r = np.random.default_rng(950 + S)
    B, smax = 2, S + 8
    in_len = [S, S // 2]
    qkv = h(r.standard_normal((B, S, 3 * H * Dh)))
    cache_a = torch.zeros((B, 2, H, smax, Dh), dtype=KINDS[kind][2], device='cuda')
    out_a = run_attention_plugin(attention_plugin(H, Dh, int(kind == 'int8')), qkv.clone(), cache_a, [S] * B, 0, True,
                                 np.zeros((B, smax), np.int32), in_len, S, smax, scales_of(kind))
    out_b, cache_b = run_context(lib, kind, H, H, Dh, S, in_len, qkv, smax)
    assert torch.equal(out_a, out_b) and torch.equal(cache_a, cache_b)
