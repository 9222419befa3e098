"""GPU parity of the fp8 (OCP E4M3) KV cache at plugin level: the GPTAttention plugin with fp8_kv_cache = 1 against the
numpy restatement of the rule (tensorrt_llm/runtime/kv_fp8_ref.py) - decode over every split layout, append bit-exact,
beam (cache indirection), paged, context padded and packed, and the launch errors.

Bounds: context 2e-3 (generation) / 5e-3 (prompt), the reference's own plugin-test tolerances (test_gpt_attention.py:828-831,
685-695); cache bytes exact wherever no RoPE precedes the store (all of V; K with rot = 0); a roped K row may sit on the
adjacent code in at most 2 % of its elements (the kernel's RoPE uses fma - one fp16 ulp - and an E4M3 step is 2^7 fp16 ulps:
tests/test_kv_fp8_ref.py::test_a_one_ulp_change_of_k_moves_few_codes)."""
import numpy as np
import pytest
import torch

from helpers import HostTensor, as_f32, f32, h, i8, i32, make_plugin
from tensorrt_llm.plugin import capi
from tensorrt_llm.runtime import kv_fp8_ref as R

pytestmark = pytest.mark.gpu

_T2C = {torch.float32: capi.FLOAT, torch.float16: capi.HALF, torch.int32: capi.INT32, torch.uint8: capi.FP8}


def attention_plugin(H, Dh, rot=None, packed=0, paged=0):
    return make_plugin('GPTAttention', [
        ('num_heads', i32(H)), ('head_size', i32(Dh)), ('unidirectional', i32(1)), ('q_scaling', f32(1.0)),
        ('rotary_embedding_dim', i32(Dh if rot is None else rot)), ('neox_rotary_style', i8(1)),
        ('context_fmha_type', i8(0)), ('multi_block_mode', i8(0)), ('multi_query_mode', i8(0)),
        ('int8_kv_cache', i32(0)), ('fp8_kv_cache', i32(1)), ('remove_input_padding', i8(packed)),
        ('mask_type', i32([1])), ('paged_kv_cache', i32(paged)), ('type_id', i32([capi.HALF])), ('in_flight_batching', i32(0)),
    ])


def run_plugin(plugin, inputs, outputs, null_inputs=()):
    """helpers.run_plugin with uint8 tensors travelling as capi.FP8 (the cache ports); `null_inputs`: positions handed over as
    null pointers.  Raises RuntimeError when the enqueue fails."""
    in_shapes, in_types, in_ptrs = [], [], []
    for i, t in enumerate(inputs):
        if isinstance(t, HostTensor):
            in_shapes.append(t.shape), in_types.append(capi.INT32), in_ptrs.append(t.ptr())
        else:
            in_shapes.append(list(t.shape)), in_types.append(_T2C[t.dtype]), in_ptrs.append(0 if i in null_inputs else t.data_ptr())
    out_shapes = [list(t.shape) for t in outputs]
    out_types = [_T2C[t.dtype] for t in outputs]
    for pos in range(len(inputs) + len(outputs)):
        assert plugin.supports_format(pos, in_shapes + out_shapes, in_types + out_types, len(inputs)), pos
    ws_bytes = plugin.workspace_size(in_shapes, in_types, out_shapes, out_types)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device='cuda')
    try:
        plugin.enqueue(in_shapes, in_types, in_ptrs, out_shapes, out_types, [t.data_ptr() for t in outputs], ws.data_ptr(),
                       torch.cuda.current_stream().cuda_stream)
    finally:
        torch.cuda.synchronize()


def run_attention(p, qkv, cache, seq_len, past_len, is_context, masked, in_len, max_in, smax, scales, ci=None, pointers=None,
                  null_inputs=(), check_format=True):
    B = len(seq_len)
    out = torch.empty(qkv.shape[:-1] + (qkv.shape[-1] // 3, ), dtype=torch.float16, device='cuda')
    dummy = torch.zeros(max(max_in, B * smax), dtype=torch.int32, device='cuda')
    ins = [qkv, cache, torch.tensor(seq_len, dtype=torch.int32, device='cuda'), HostTensor([past_len, 1 if is_context else 0]),
           torch.tensor(masked, dtype=torch.int32, device='cuda'), torch.tensor(in_len, dtype=torch.int32, device='cuda'),
           dummy[:max_in], dummy[:B * smax].view(B, 1, smax)]
    if ci is not None:  # int32 [batch, beam_width, smax]
        ins[7] = torch.from_numpy(np.ascontiguousarray(ci, dtype=np.int32)).cuda()
    ins += [torch.tensor([scales[0]], dtype=torch.float32, device='cuda'),
            torch.tensor([scales[1]], dtype=torch.float32, device='cuda')]
    if pointers is not None:
        ins += [pointers]
    run_plugin(p, ins, [out, cache], null_inputs)
    return out


def code_index(c):
    """E4M3 codes on a line: adjacent finite values differ by 1, +0 and -0 coincide."""
    c = np.asarray(c).astype(np.int32)
    return np.where(c & 0x80, -(c & 0x7f), c & 0x7f)


def assert_k_bytes(got, ref):
    d = np.abs(code_index(got) - code_index(ref))
    assert d.max() <= 1, f'a K code is {d.max()} steps off'
    assert np.mean(got == ref) >= 0.98, f'only {np.mean(got == ref):.4f} of the K bytes equal the restatement'


SCALES = [(1.0, 1.0), (1.0 / 0.05, 0.05)]


def decode_case(L, H, Dh, seed):
    r = np.random.default_rng(seed)
    B, smax = 2, (1152 if L < 1152 else (2048 if L < 2048 else 4096))  # every NIT / split count the launcher can pick
    max_in = max(L - 3, 1) if L > 4 else L
    in_len = [max_in, max(max_in // 2, 1)]
    masked = np.zeros((B, smax), dtype=np.int32)
    masked[1, in_len[1]:max_in] = 1
    past = r.standard_normal((B, 2, H, smax, Dh)).astype(np.float32)
    past[:, :, :, L:] = 0
    qkv = h(r.standard_normal((B, 1, 3 * H * Dh)))
    return B, smax, max_in, in_len, masked, past, qkv


@pytest.mark.parametrize('scales', SCALES, ids=['s1', 's20'])
@pytest.mark.parametrize('H,Dh', [(4, 128), (4, 64), (2, 32)])
@pytest.mark.parametrize('L', [1, 17, 128, 1023, 2047, 4000])
def test_mmha_decode_fp8_vs_restatement(scales, H, Dh, L):
    """Generation step: new token at slot L; half of batch element 1's prompt is padding."""
    B, smax, max_in, in_len, masked, past, qkv = decode_case(L, H, Dh, 100 + L)
    cache_np = R.kv_store_fp8(past, scales[0])
    cache = torch.from_numpy(cache_np.copy()).cuda()
    out = run_attention(attention_plugin(H, Dh), qkv, cache, [L, L], L, False, masked, in_len, max_in, smax, scales)
    ref_cache = cache_np.copy()
    ref = R.mmha_decode_fp8(as_f32(qkv)[:, 0], ref_cache, [L, L], in_len, max_in, L, H, Dh, Dh, scales[0], scales[1],
                            masked_tokens=masked)
    err = np.abs(as_f32(out)[:, 0] - ref).max()
    print(f'fp8 decode H={H} Dh={Dh} L={L} scales={scales}: max |ctx - ref| = {err:.3e}')
    np.testing.assert_allclose(as_f32(out)[:, 0], ref, atol=2e-3, rtol=0)
    got = cache.cpu().numpy()
    keep = np.ones(smax, dtype=bool)
    keep[L] = False
    np.testing.assert_array_equal(got[:, :, :, keep], cache_np[:, :, :, keep])
    np.testing.assert_array_equal(got[:, 1, :, L], ref_cache[:, 1, :, L])  # V is never rotated
    assert_k_bytes(got[:, 0, :, L], ref_cache[:, 0, :, L])
    assert not np.any((got & 0x7f) == 0x7f)


@pytest.mark.parametrize('s_oq', [1.0, 4.0, 20.0])
def test_kv_cache_append_fp8_bit_exact(s_oq):
    """Without RoPE the appended K/V are pure quantisations: the cache must equal kv_store_fp8 byte for byte - zeros of both
    signs, the subnormal boundary (2^-9 the smallest code, 2^-10 ties to 0), exact ties between adjacent codes, +-448, values
    beyond it and the fp16 extremes - and nothing else may be written."""
    r = np.random.default_rng(7)
    B, H, Dh, smax, L = 2, 4, 128, 32, 16
    x = (r.standard_normal((B, 1, 3 * H * Dh)) * 3 / s_oq).astype(np.float32)
    inv = np.float32(1.0 / s_oq)
    mags = np.array([0.0, 2.0 ** -10, 2.0 ** -9, 3 * 2.0 ** -10, 5 * 2.0 ** -10, 2.0 ** -6 - 2.0 ** -10, 1.0625, 1.1875, 1.3125,
                     17.0, 19.0, 232.0, 248.0, 448.0, 449.0, 464.0, 480.0, 1000.0], np.float32) * inv
    special = np.concatenate([mags, -mags, [65504.0, -65504.0, 6.0e-8, -6.0e-8]]).astype(np.float32)
    flat = x.reshape(B, 3, H * Dh)
    for kv in (1, 2):  # K and V rows of both sequences
        flat[:, kv, :special.size] = special
    qkv = h(x)
    cache = torch.zeros((B, 2, H, smax, Dh), dtype=torch.uint8, device='cuda')
    run_attention(attention_plugin(H, Dh, rot=0), qkv, cache, [L, L], L, False, np.zeros((B, smax), np.int32), [L, L], L, smax,
                  (s_oq, 1.0 / s_oq))
    src = as_f32(qkv).reshape(B, 3, H, Dh)
    expect = np.zeros((B, 2, H, smax, Dh), np.uint8)
    expect[:, :, :, L] = R.kv_store_fp8(src[:, 1:], s_oq)
    np.testing.assert_array_equal(cache.cpu().numpy(), expect)
    assert (expect[0, 0, 0, L, 0], expect[0, 0, 0, L, mags.size]) == (0x00, 0x80)  # the sign of zero


@pytest.mark.parametrize('scales', SCALES, ids=['s1', 's20'])
@pytest.mark.parametrize('L,W', [(17, 2), (1023, 2), (17, 4), (1023, 4)])
def test_mmha_decode_fp8_beam_cache_indirection(scales, L, W):
    r = np.random.default_rng(300 + L + W)
    H, Dh, batch, smax = 4, 128, 2, 1152
    B = batch * W
    max_in = L - 3
    in_len = np.repeat([max_in, max_in // 2], W).tolist()
    masked = np.zeros((B, smax), dtype=np.int32)
    masked[W:, in_len[W]:max_in] = 1
    past = r.standard_normal((B, 2, H, smax, Dh)).astype(np.float32)
    past[:, :, :, L:] = 0
    cache_np = R.kv_store_fp8(past, scales[0])
    cache = torch.from_numpy(cache_np.copy()).cuda()
    ci = r.integers(0, W, (batch, W, smax)).astype(np.int32)
    qkv = h(r.standard_normal((B, 1, 3 * H * Dh)))
    out = run_attention(attention_plugin(H, Dh), qkv, cache, [L] * B, L, False, masked, in_len, max_in, smax, scales, ci=ci)
    eff = np.empty_like(cache_np)  # per sequence, the cache its indirection row selects
    for bb in range(B):
        b, k = divmod(bb, W)
        eff[bb] = cache_np[b * W + ci[b, k], :, :, np.arange(smax)].transpose(1, 2, 0, 3)
    ref_cache = eff.copy()
    ref = R.mmha_decode_fp8(as_f32(qkv)[:, 0], ref_cache, [L] * B, in_len, max_in, L, H, Dh, Dh, scales[0], scales[1],
                            masked_tokens=masked)
    np.testing.assert_allclose(as_f32(out)[:, 0], ref, atol=2e-3, rtol=0)
    got = cache.cpu().numpy()
    keep = np.ones(smax, dtype=bool)
    keep[L] = False
    np.testing.assert_array_equal(got[:, :, :, keep], cache_np[:, :, :, keep])  # the siblings' rows are untouched
    np.testing.assert_array_equal(got[:, 1, :, L], ref_cache[:, 1, :, L])
    assert_k_bytes(got[:, 0, :, L], ref_cache[:, 0, :, L])


def block_table(pool, B, M, mapped, H, T, Dh):
    """int64 [B, 1, 2, M]: logical block j of sequence b is pool block j * B + b (the blocks of the sequences interleave); blocks
    at or beyond `mapped` are not handed out (0)."""
    table = np.zeros((B, 1, 2, M), np.int64)
    blk_bytes = H * T * Dh
    for b in range(B):
        for j in range(mapped):
            for kv in range(2):
                table[b, 0, kv, j] = pool.data_ptr() + ((j * B + b) * 2 + kv) * blk_bytes
    return table


def pool_to_linear(pool_np, B, M, mapped, H, T, Dh):
    out = np.zeros((B, 2, H, M * T, Dh), np.uint8)
    for b in range(B):
        for j in range(mapped):
            out[b, :, :, j * T:(j + 1) * T] = pool_np[j * B + b]
    return out


@pytest.mark.parametrize('scales', SCALES, ids=['s1', 's20'])
@pytest.mark.parametrize('L,T', [(17, 16), (1023, 16), (17, 64), (1023, 64)])
def test_mmha_decode_fp8_paged(scales, L, T):
    """Pool + block pointers, one trailing logical block not handed out (table entry 0: the kernel must not form an address from
    it - its rows lie beyond the length and are masked)."""
    r = np.random.default_rng(400 + L + T)
    H, Dh, B = 4, 128, 2
    mapped = L // T + 1  # the block of slot L is mapped
    M = mapped + 1
    smax = M * T
    max_in = L - 3
    in_len = [max_in, max_in // 2]
    masked = np.zeros((B, smax), dtype=np.int32)
    masked[1, in_len[1]:max_in] = 1
    past = r.standard_normal((B * mapped, 2, H, T, Dh)).astype(np.float32)
    pool_np = R.kv_store_fp8(past, scales[0])
    lin = pool_to_linear(pool_np, B, M, mapped, H, T, Dh)
    lin[:, :, :, L:] = 0
    for b in range(B):  # the same zeros in the pool
        for j in range(mapped):
            pool_np[j * B + b] = lin[b, :, :, j * T:(j + 1) * T]
    pool = torch.from_numpy(pool_np.copy()).cuda()
    table = block_table(pool, B, M, mapped, H, T, Dh)
    pointers = torch.from_numpy(table.view(np.int32).reshape(B, 1, 2, 2 * M)).cuda()
    qkv = h(r.standard_normal((B, 1, 3 * H * Dh)))
    out = run_attention(attention_plugin(H, Dh, paged=1), qkv, pool, [L, L], L, False, masked, in_len, max_in, smax, scales,
                        pointers=pointers)
    ref_cache = lin.copy()
    ref = R.mmha_decode_fp8(as_f32(qkv)[:, 0], ref_cache, [L, L], in_len, max_in, L, H, Dh, Dh, scales[0], scales[1],
                            masked_tokens=masked)
    np.testing.assert_allclose(as_f32(out)[:, 0], ref, atol=2e-3, rtol=0)
    got = pool_to_linear(pool.cpu().numpy(), B, M, mapped, H, T, Dh)
    keep = np.ones(smax, dtype=bool)
    keep[L] = False
    np.testing.assert_array_equal(got[:, :, :, keep], lin[:, :, :, keep])
    np.testing.assert_array_equal(got[:, 1, :, L], ref_cache[:, 1, :, L])
    assert_k_bytes(got[:, 0, :, L], ref_cache[:, 0, :, L])


@pytest.mark.parametrize('scales', SCALES, ids=['s1', 's20'])
@pytest.mark.parametrize('H,Dh', [(4, 128), (2, 64)])
@pytest.mark.parametrize('S', [5, 64, 200])
def test_context_attention_fp8_padded_and_packed(scales, H, Dh, S):
    r = np.random.default_rng(200 + S)
    B, smax = 3, S + 8
    in_len = [S, max(S // 3, 1), max(S // 2, 1)]
    qkv = h(r.standard_normal((B, S, 3 * H * Dh)))
    masked = np.zeros((B, smax), np.int32)
    cache_pad = torch.zeros((B, 2, H, smax, Dh), dtype=torch.uint8, device='cuda')
    out_pad = run_attention(attention_plugin(H, Dh), qkv.clone(), cache_pad, [S] * B, 0, True, masked, in_len, S, smax, scales)
    ref_cache = np.zeros((B, 2, H, smax, Dh), np.uint8)
    ref, _ = R.context_attention_fp8(as_f32(qkv), ref_cache, in_len, H, Dh, Dh, scales[0])
    np.testing.assert_allclose(as_f32(out_pad), ref, atol=5e-3, rtol=0)
    got = cache_pad.cpu().numpy()
    np.testing.assert_array_equal(got[:, 1], ref_cache[:, 1])
    assert_k_bytes(got[:, 0], ref_cache[:, 0])
    # the packed form: the tokens of all sequences back to back in [1, T, 3 D]
    packed = torch.cat([qkv[b, :in_len[b]] for b in range(B)], dim=0)[None].contiguous()
    cache_pk = torch.zeros((B, 2, H, smax, Dh), dtype=torch.uint8, device='cuda')
    out_pk = run_attention(attention_plugin(H, Dh, packed=1), packed, cache_pk, [S] * B, 0, True, masked, in_len, S, smax, scales)
    off = 0
    for b in range(B):
        assert torch.equal(out_pk[0, off:off + in_len[b]], out_pad[b, :in_len[b]]), b
        off += in_len[b]
    assert torch.equal(cache_pk, cache_pad)


def test_context_attention_fp8_paged_with_an_unmapped_trailing_block():
    r = np.random.default_rng(9)
    H, Dh, B, T, S = 4, 128, 2, 16, 40
    mapped = -(-(S + 1) // T)
    M = mapped + 1
    smax = M * T
    in_len = [S, S // 2]
    scales = SCALES[1]
    qkv = h(r.standard_normal((B, S, 3 * H * Dh)))
    pool = torch.zeros((B * mapped, 2, H, T, Dh), dtype=torch.uint8, device='cuda')
    table = block_table(pool, B, M, mapped, H, T, Dh)
    pointers = torch.from_numpy(table.view(np.int32).reshape(B, 1, 2, 2 * M)).cuda()
    masked = np.zeros((B, smax), np.int32)
    out = run_attention(attention_plugin(H, Dh, paged=1), qkv.clone(), pool, [S] * B, 0, True, masked, in_len, S, smax, scales,
                        pointers=pointers)
    ref_cache = np.zeros((B, 2, H, smax, Dh), np.uint8)
    ref, _ = R.context_attention_fp8(as_f32(qkv), ref_cache, in_len, H, Dh, Dh, scales[0])
    np.testing.assert_allclose(as_f32(out), ref, atol=5e-3, rtol=0)
    got = pool_to_linear(pool.cpu().numpy(), B, M, mapped, H, T, Dh)
    np.testing.assert_array_equal(got[:, 1], ref_cache[:, 1])
    assert_k_bytes(got[:, 0], ref_cache[:, 0])


def test_launches_without_a_scale_or_with_both_cache_types_are_refused_and_write_nothing():
    H, Dh, L = 4, 128, 17
    B, smax, max_in, in_len, masked, past, qkv = decode_case(L, H, Dh, 1)
    cache_np = R.kv_store_fp8(past, 1.0)
    p = attention_plugin(H, Dh)
    for null in ((8, ), (9, )):
        cache = torch.from_numpy(cache_np.copy()).cuda()
        with pytest.raises(RuntimeError):
            run_attention(p, qkv, cache, [L, L], L, False, masked, in_len, max_in, smax, (1.0, 1.0), null_inputs=null)
        assert 'fp8' in capi.last_error() and 'scale' in capi.last_error(), capi.last_error()
        np.testing.assert_array_equal(cache.cpu().numpy(), cache_np)
    S = 12
    qc = h(np.random.default_rng(2).standard_normal((B, S, 3 * H * Dh)))
    cache = torch.zeros((B, 2, H, smax, Dh), dtype=torch.uint8, device='cuda')
    with pytest.raises(RuntimeError):
        run_attention(p, qc, cache, [S, S], 0, True, masked, [S, S], S, smax, (1.0, 1.0), null_inputs=(8, ))
    assert 'fp8' in capi.last_error(), capi.last_error()
    assert not cache.any()
    # both cache types: the creator refuses the pair, so the launch check is reached through a serialised configuration - the
    # blob of an fp8 plugin with the int8 flag's bytes (found by comparing blobs) set as well
    def blob(int8, fp8):
        return make_plugin('GPTAttention', [
            ('num_heads', i32(H)), ('head_size', i32(Dh)), ('unidirectional', i32(1)), ('q_scaling', f32(1.0)),
            ('rotary_embedding_dim', i32(Dh)), ('neox_rotary_style', i8(1)), ('context_fmha_type', i8(0)),
            ('multi_block_mode', i8(0)), ('multi_query_mode', i8(0)), ('int8_kv_cache', i32(int8)), ('fp8_kv_cache', i32(fp8)),
            ('remove_input_padding', i8(0)), ('mask_type', i32([1])), ('paged_kv_cache', i32(0)), ('type_id', i32([capi.HALF])),
            ('in_flight_batching', i32(0))]).serialize()
    b8, bf = bytearray(blob(1, 0)), bytearray(blob(0, 1))
    both = bytearray(bf)
    for k in range(len(both)):
        both[k] = b8[k] | bf[k]
    assert bytes(both) not in (bytes(b8), bytes(bf))
    pb = capi.Plugin.deserialize('GPTAttention', bytes(both))
    assert pb is not None

    def enqueue_raw(plugin, qkv_t, cache_t, seq, past_len, is_ctx, max_in_, in_len_):
        # format negotiation is skipped: no format exists for this configuration
        out = torch.empty(qkv_t.shape[:-1] + (qkv_t.shape[-1] // 3, ), dtype=torch.float16, device='cuda')
        dummy = torch.zeros(max(max_in_, B * smax), dtype=torch.int32, device='cuda')
        one = torch.ones(1, dtype=torch.float32, device='cuda')
        ins = [qkv_t, cache_t, torch.tensor(seq, dtype=torch.int32, device='cuda'), HostTensor([past_len, is_ctx]),
               torch.tensor(masked, dtype=torch.int32, device='cuda'), torch.tensor(in_len_, dtype=torch.int32, device='cuda'),
               dummy[:max_in_], dummy[:B * smax].view(B, 1, smax), one, one.clone()]
        shapes = [t.shape if isinstance(t, HostTensor) else list(t.shape) for t in ins]
        types = [capi.INT32 if isinstance(t, HostTensor) else _T2C[t.dtype] for t in ins]
        ptrs = [t.ptr() if isinstance(t, HostTensor) else t.data_ptr() for t in ins]
        oshapes, otypes = [list(out.shape), list(cache_t.shape)], [capi.HALF, capi.FP8]
        ws = torch.empty(max(plugin.workspace_size(shapes, types, oshapes, otypes), 16), dtype=torch.uint8, device='cuda')
        try:
            plugin.enqueue(shapes, types, ptrs, oshapes, otypes, [out.data_ptr(), cache_t.data_ptr()], ws.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
        finally:
            torch.cuda.synchronize()

    cache = torch.from_numpy(cache_np.copy()).cuda()
    with pytest.raises(RuntimeError):
        enqueue_raw(pb, qkv, cache, [L, L], L, 0, max_in, in_len)
    assert 'exclusive' in capi.last_error(), capi.last_error()
    np.testing.assert_array_equal(cache.cpu().numpy(), cache_np)
    cache = torch.zeros((B, 2, H, smax, Dh), dtype=torch.uint8, device='cuda')
    with pytest.raises(RuntimeError):
        enqueue_raw(pb, qc, cache, [S, S], 0, 1, S, [S, S])
    assert 'exclusive' in capi.last_error(), capi.last_error()
    assert not cache.any()
