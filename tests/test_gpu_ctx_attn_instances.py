"""Every instance of the context (prompt) attention on the GPU, forced through tllm_attention_params_t::context_kernel, against
oracle/attention_oracle.py - one test per case of tests/ctx_attn_cases.py (the table and what it must hold: that file and
tests/test_ctx_attn_instance_table.py).

Every launch runs on buffers full of sentinels (out: NaN, out_q8 and the cache: the byte 0xA5, 256 guard bytes of 0xA5 behind the
workspace, two guard rows behind packed buffers), twice from the same inputs, and the two runs must agree bit for bit.  Checked:

 a. the RoPE / cache stage.  The rewritten qkv: q and k of the real tokens against llama_oracle.apply_rope at the project's bound
    for rotated rows (atol 2e-4, rtol 2e-3; positions <= 2048), v of the real tokens unchanged, padding rows zero, guard rows
    untouched.  The cache: rows [0, S) equal BIT FOR BIT the store rule (a copy, kv_store, kv_store_fp8) applied to the launch's
    own rewritten k and v (padding rows: the image of zero) - RoPE ulps do not enter; rows [S, Smax), the sibling sequences under
    a beam stride, the rows of paged blocks a sequence does not map and the pool's spare blocks keep their bytes.
 b. the attention stage.  `out` against causal_attention_f64 of the launch's own q, k, v rows within attention_oracle.tolerance
    (derived there from the kernels' rounding points; no measured number); padding rows exactly zero; the workspace guard intact.
    With out_q8: the bytes of quantize_tensor(out of the twin launch without it) - and `out` untouched by the MFMA kernels, the fp16
    result under the wave-per-query kernel.  What the launcher refuses launches nothing.
 c. every key counted once.  q = 0 makes every probability exactly 1, V holds 0/1 witness codes, so out[q, d] must be
    count_d(q) / (q + 1) within one fp16 ulp: a single dropped or doubled key moves an element by 1 / (q + 1) >= 4.9e-4.  Every
    length edge and a deep length, padded and packed.
 d. forced against natural: for every kind, a shape at which the rule of the device present chooses it runs bit-identically with
    the kind forced and left open."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import ctx_attn_cases as CC
from oracle import attention_oracle as A
from oracle import llama_oracle as O
from oracle.gemv_oracle import ulp16
from tensorrt_llm.plugin import capi
from tensorrt_llm.runtime import kv_fp8_ref as F8

pytestmark = pytest.mark.gpu

KV_QUANT = 20.0          # kv_scale_orig_quant: N(0, 1) values, +-6 sigma inside 127 / 20
OUT_QUANT = 127.0 / 4.0  # out_q_scale: |out| stays below 4 for N(0, 1) values
SENT = 0xA5
GUARD_ROWS, GUARD_BYTES = 2, 256
KV = {'fp16': (capi.HALF, np.float16), 'int8': (capi.INT8, np.int8), 'fp8': (capi.FP8, np.uint8)}


def store(kv, x16):
    """the cache image of fp16 values: the store rule of the element type"""
    if kv == 'fp16':
        return np.asarray(x16, np.float16)
    if kv == 'int8':
        return O.kv_store(np.asarray(x16, np.float32), KV_QUANT)
    return F8.kv_store_fp8(np.asarray(x16, np.float32), KV_QUANT)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Geometry:
    """the buffers of one case at one batch of lengths: sizes, the paged pool's block table, and the views back into them"""

    def __init__(self, c, lens):
        self.c, self.lens = c, [int(x) for x in lens]
        self.B, self.S = len(lens), max(lens)
        self.row = (c.H + 2 * c.Hkv) * c.dh
        self.packed = c.layout == 'packed'
        self.rows = sum(self.lens) if self.packed else self.B * self.S
        self.esz = 2 if c.kv == 'fp16' else 1
        self.nseq = self.B * c.stride
        self.T = {'linear': 0, 'paged16': 16, 'paged64': 64}[c.cache]
        if self.T:
            # a sequence maps ceil((len + 1) / T) blocks (KVCacheManager.add_sequence); one more logical block than anyone maps
            self.mapped = [(self.lens[s // c.stride] + self.T) // self.T for s in range(self.nseq)]
            self.M = max(self.mapped) + 1
            self.smax = self.M * self.T
            # pool blocks in a scattered order, one spare block at each end that no table entry names
            n = 2 * sum(self.mapped)
            order = np.random.default_rng(n).permutation(n) + 1
            self.block_of, k = {}, 0
            for s in range(self.nseq):
                for kvi in range(2):
                    for j in range(self.mapped[s]):
                        self.block_of[(s, kvi, j)] = int(order[k])
                        k += 1
            self.nblocks = n + 2
            self.block_bytes = c.Hkv * self.T * c.dh * self.esz
            self.cache_bytes = self.nblocks * self.block_bytes
        else:
            self.smax = self.S + 8
            self.cache_bytes = self.nseq * 2 * c.Hkv * self.smax * c.dh * self.esz

    def cu(self):
        return np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int32)

    def to_buffer(self, padded):
        """[B, S, W] -> the launch's token-major buffer (packed: the real rows, + guard rows of 7.0)"""
        if not self.packed:
            return np.ascontiguousarray(padded).reshape(self.rows, -1)
        real = np.concatenate([padded[b, :n] for b, n in enumerate(self.lens)], axis=0)
        return np.concatenate([real, np.full((GUARD_ROWS, real.shape[1]), 7.0, padded.dtype)], axis=0)

    def to_padded(self, buf, fill=0):
        """the launch's buffer -> [B, S, W], packed: `fill` where no row exists"""
        if not self.packed:
            return buf[:self.rows].reshape(self.B, self.S, -1)
        out = np.full((self.B, self.S, buf.shape[1]), fill, buf.dtype)
        cu = self.cu()
        for b, n in enumerate(self.lens):
            out[b, :n] = buf[cu[b]:cu[b] + n]
        return out

    def table(self, pool_ptr):
        t = np.zeros((self.nseq, 2, self.M), np.int64)
        for (s, kvi, j), blk in self.block_of.items():
            t[s, kvi, j] = pool_ptr + blk * self.block_bytes
        return t

    def cache_view(self, raw, dtype):
        """bytes -> ([nseq, 2, Hkv, smax, Dh] elements, exists [nseq, smax]); paged: rows of unmapped blocks do not exist"""
        c = self.c
        if not self.T:
            return raw.view(dtype).reshape(self.nseq, 2, c.Hkv, self.smax, c.dh), np.ones((self.nseq, self.smax), bool)
        blocks = raw.view(dtype).reshape(self.nblocks, c.Hkv, self.T, c.dh)
        lin = np.zeros((self.nseq, 2, c.Hkv, self.smax, c.dh), dtype)
        exists = np.zeros((self.nseq, self.smax), bool)
        for (s, kvi, j), blk in self.block_of.items():
            lin[s, kvi, :, j * self.T:(j + 1) * self.T] = blocks[blk]
            exists[s, j * self.T:(j + 1) * self.T] = True
        return lin, exists

    def spare_blocks(self, raw):
        used = set(self.block_of.values())
        blocks = raw.reshape(self.nblocks, self.block_bytes)
        return blocks[[i for i in range(self.nblocks) if i not in used]]


class Result:
    pass


def launch(lib, c, g, qkv_padded, kind, q8=False, workspace=True):
    """one tllm_attention_context call on fresh sentinel-filled buffers; everything it could have written comes back as numpy"""
    rot, neox = CC.rotary(c)
    p = capi.AttentionParams(batch=g.B, seq=g.S, num_heads=c.H, num_kv_heads=c.Hkv, head_size=c.dh, rotary_dim=rot, neox=neox,
                             q_scaling=CC.q_scaling(c), kv_cache_type=KV[c.kv][0], max_seq_len=g.smax, cache_seq_stride=c.stride,
                             tokens_per_block=g.T, max_blocks_per_seq=g.M if g.T else 0, context_kernel=kind)
    keep = []

    def put(name, t):
        keep.append(t)
        setattr(p, name, t.data_ptr())
        return t

    qkv = put('qkv', dev(g.to_buffer(qkv_padded)))
    put('input_lengths', dev(np.asarray(g.lens, np.int32)))
    if g.packed:
        put('cu_seqlens', dev(g.cu()))
    if c.kv != 'fp16':
        put('kv_scale_orig_quant', torch.tensor([KV_QUANT], dtype=torch.float32, device='cuda'))
    cache = put('kv_cache', torch.full((g.cache_bytes, ), SENT, dtype=torch.uint8, device='cuda'))
    if g.T:
        put('block_pointers', dev(g.table(cache.data_ptr())))
    nout = qkv.shape[0] * c.H * c.dh
    out = put('out', torch.full((nout, ), float('nan'), dtype=torch.float16, device='cuda'))
    out_q8 = torch.full((nout, ), SENT, dtype=torch.uint8, device='cuda')
    if q8:
        put('out_q8', out_q8)
        put('out_q_scale', torch.tensor([OUT_QUANT], dtype=torch.float32, device='cuda'))
    size = lib.tllm_attention_workspace_size(ctypes.byref(p), 1)
    ws = torch.full((size + GUARD_BYTES, ), SENT, dtype=torch.uint8, device='cuda')
    if workspace:
        p.workspace = ws.data_ptr()
    r = Result()
    r.rc = lib.tllm_attention_context(ctypes.byref(p), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    r.error = capi.last_error() if r.rc else ''
    r.qkv = qkv.cpu().numpy()
    r.out = out.cpu().numpy().reshape(qkv.shape[0], c.H * c.dh)
    r.out_q8 = out_q8.cpu().numpy().view(np.int8).reshape(qkv.shape[0], c.H * c.dh)
    r.cache = cache.cpu().numpy()
    r.guard = ws[size:].cpu().numpy()
    a = [ctypes.c_int32(-1) for _ in range(4)]
    r.layout = None if lib.tllm_attention_context_layout(ctypes.byref(p), 0, *[ctypes.byref(x) for x in a]) else tuple(x.value for x in a)
    return r


def same_bits(a, b):
    return all(np.array_equal(getattr(a, n).view(np.uint8), getattr(b, n).view(np.uint8)) for n in ('qkv', 'out', 'out_q8', 'cache', 'guard'))


def untouched(r, qkv_buffer):
    return (np.array_equal(r.qkv.view(np.uint16), qkv_buffer.view(np.uint16)) and np.isnan(r.out).all() and (r.out_q8 == np.int8(SENT - 256)).all()
            and (r.cache == SENT).all() and (r.guard == SENT).all())


def run_twice(lib, c, g, qkv_padded, kind, q8=False, workspace=True):
    r = launch(lib, c, g, qkv_padded, kind, q8, workspace)
    assert r.rc == 0, r.error
    again = launch(lib, c, g, qkv_padded, kind, q8, workspace)
    assert again.rc == 0 and same_bits(r, again), 'two runs from the same inputs differ'
    assert (r.guard == SENT).all(), 'bytes behind the workspace were written'
    return r


def split(c, rows):
    """[..., row] -> q [..., H*Dh], k, v [..., Hkv*Dh]"""
    a, b = c.H * c.dh, (c.H + c.Hkv) * c.dh
    return rows[..., :a], rows[..., a:b], rows[..., b:]


def real_mask(g):
    return np.arange(g.S)[None, :] < np.asarray(g.lens)[:, None]  # [B, S]


def check_rope_and_cache(c, g, qkv_in, r):
    """stage a; returns the rewritten rows in padded form (zeros where a packed batch has no row)"""
    rot, neox = CC.rotary(c)
    after = g.to_padded(r.qkv)
    real = real_mask(g)
    if g.packed:
        np.testing.assert_array_equal(r.qkv[g.rows:].view(np.uint16), np.full((GUARD_ROWS, g.row), 7.0, np.float16).view(np.uint16),
                                      err_msg='rows behind the packed qkv were written')
    else:
        assert not after[~real].any(), 'padding rows of qkv are not zero'
    q_in, k_in, v_in = split(c, qkv_in)
    q, k, v = split(c, after)
    np.testing.assert_array_equal(v[real].view(np.uint16), v_in[real].view(np.uint16), err_msg='v of real tokens changed')
    for name, got, x in (('q', q, q_in), ('k', k, k_in)):
        want = np.zeros(x.shape, np.float32)
        xr = x.astype(np.float32).reshape(g.B, g.S, -1, c.dh)
        for s in range(g.S):
            want[:, s] = O.apply_rope(xr[:, s], s, rot, bool(neox)).reshape(g.B, -1)
        np.testing.assert_allclose(got[real].astype(np.float32), want[real], atol=2e-4, rtol=2e-3, err_msg=f'RoPE of {name}')
    # the cache, bit for bit from the launch's own rows
    lin, exists = g.cache_view(r.cache, KV[c.kv][1])
    sent = np.full(1, SENT, np.uint8).repeat(g.esz).view(KV[c.kv][1])[0]
    want = np.full(lin.shape, sent, lin.dtype)
    for b in range(g.B):
        for kvi, rows in enumerate((k, v)):
            pad = np.where(real[b][:, None], rows[b], np.float16(0)).reshape(g.S, c.Hkv, c.dh).transpose(1, 0, 2)
            want[b * c.stride, kvi, :, :g.S] = store(c.kv, pad)
    want[np.broadcast_to(~exists[:, None, None, :, None], want.shape)] = 0
    lin = lin.copy()
    lin[np.broadcast_to(~exists[:, None, None, :, None], lin.shape)] = 0
    np.testing.assert_array_equal(lin.view(np.uint8), want.view(np.uint8), err_msg='cache bytes (rows [0, S) by the store rule, the rest untouched)')
    if g.T:
        assert (g.spare_blocks(r.cache) == SENT).all(), 'a pool block no table entry names was written'
    return after


def check_attention(c, g, after, out_padded, what):
    """stage b: `out` within the oracle's tolerance on the launch's own rows; returns the worst |got - oracle| / tolerance"""
    q, k, v = (x.astype(np.float64) for x in split(c, after))
    scale = np.float32(1.0) / (np.sqrt(np.float32(c.dh)) * np.float32(CC.q_scaling(c)))  # the launch's fp32 score scale
    ref, absmass = A.causal_attention_f64(q, k, v, g.lens, c.H, c.Hkv, c.dh, np.float64(scale))
    tol = A.tolerance(ref, absmass, g.S, np.abs(v).max())
    real = real_mask(g)
    got = out_padded.astype(np.float64)
    assert np.isfinite(got[real]).all(), f'{what}: rows of real tokens not written'
    ratio = float((np.abs(got - ref)[real] / tol[real]).max())
    print(f'CTXATTN-RATIO {CC.KIND_NAME[c.kind]}-dh{c.dh} {ratio:.4f} {what}')
    assert ratio <= 1.0, f'{what}: |got - oracle| / tolerance = {ratio:.3f} (tolerance median {np.median(tol[real]):.2e})'
    if not g.packed:
        assert not got[~real].any(), f'{what}: rows beyond the sequence are not zero'
    return ratio


def inputs(c, g):
    r = np.random.default_rng(zlib.crc32(CC.case_id(c).encode()))
    return r.standard_normal((g.B, g.S, g.row)).astype(np.float16)


RUN = [c for c in CC.GRID + CC.NATURAL]


@pytest.mark.parametrize('c', RUN, ids=CC.case_id)
def test_instance_vs_oracle(lib, c):
    g = Geometry(c, c.lens)
    qkv_in = inputs(c, g)
    kind = c.kind if c.forced else 0
    r = run_twice(lib, c, g, qkv_in, kind, workspace=bool(c.workspace))
    assert r.layout is not None and r.layout[0] == c.kind, (r.layout, c.kind)  # the instance that ran
    if c.forced and c.workspace and CC.q_scaling(c) > 0:
        assert r.layout == CC.plan(c.dh, g.S, g.B, c.H, True, True, 0, c.kind)
    what = CC.case_id(c)
    after = check_rope_and_cache(c, g, qkv_in, r)
    assert (r.out_q8 == np.int8(SENT - 256)).all(), 'out_q8 written without being passed'
    check_attention(c, g, after, g.to_padded(r.out, fill=0), what)
    if g.packed:
        assert np.isnan(r.out[g.rows:]).all(), 'rows behind the packed out were written'
    if not c.q8:
        return
    # the int8 output: the same launch with out_q8 - RoPE, cache and (wave-per-query) out as before, out_q8 the quantiser's bytes
    rq = run_twice(lib, c, g, qkv_in, kind, q8=True, workspace=bool(c.workspace))
    assert np.array_equal(rq.qkv.view(np.uint16), r.qkv.view(np.uint16)) and np.array_equal(rq.cache, r.cache)
    n = g.rows
    want = O.quantize_tensor(r.out[:n].astype(np.float32), OUT_QUANT)
    np.testing.assert_array_equal(rq.out_q8[:n], want, err_msg='out_q8 is not quantize_tensor(out)')
    assert (rq.out_q8[n:] == np.int8(SENT - 256)).all(), 'rows behind the packed out_q8 were written'
    if c.kind == CC.WAVE:
        assert np.array_equal(rq.out.view(np.uint16), r.out.view(np.uint16)), 'the wave-per-query kernel keeps writing out'
    else:
        assert np.isnan(rq.out).all(), 'the MFMA kernels must not write out next to out_q8'


@pytest.mark.parametrize('c', CC.REFUSED, ids=CC.case_id)
def test_a_refused_launch_writes_nothing(lib, c):
    g = Geometry(c, c.lens)
    qkv_in = inputs(c, g)
    r = launch(lib, c, g, qkv_in, c.kind if c.forced else 0, q8=bool(c.q8), workspace=bool(c.workspace))
    assert r.rc != 0 and c.refused in r.error, (r.rc, r.error)
    assert untouched(r, g.to_buffer(qkv_in)), 'a refused launch wrote something'
    if c.refused != 'padded':
        assert r.layout is None  # the layout query refuses it too


@pytest.mark.parametrize('c', CC.WITNESS, ids=CC.case_id)
def test_every_key_is_counted_once(lib, c):
    worst = 0.0
    for S in c.lengths:
        g = Geometry(c, CC.witness_lens(c, S))
        r = np.random.default_rng(S)
        qkv_in = np.zeros((g.B, g.S, g.row), np.float16)
        qkv_in[..., c.dh:2 * c.dh] = r.standard_normal((g.B, g.S, c.dh)).astype(np.float16)
        real = real_mask(g)
        for code in A.WITNESS_KINDS:
            V, want = A.witness(code, g.S, c.dh)
            qkv_in[..., 2 * c.dh:] = V.astype(np.float16)[None]
            res = run_twice(lib, c, g, qkv_in, c.kind)
            assert res.layout[0] == c.kind
            got = g.to_padded(res.out, fill=0).astype(np.float64)
            want = np.broadcast_to(want[None], got.shape)
            err = np.abs(got - want)[real] / ulp16(want[real])
            assert np.isfinite(err).all() and err.max() <= 1.0, (
                f'{CC.case_id(c)} lens {g.lens} code {code}: a key is miscounted - first at (sequence, query) '
                f'{np.argwhere((np.abs(got - want) > ulp16(want)) & real[..., None])[0][:2].tolist()}')
            worst = max(worst, float(err.max()))
            if not g.packed:
                assert not got[~real].any()
            v_after = split(c, g.to_padded(res.qkv))[2]
            assert np.array_equal(v_after[real], qkv_in[..., 2 * c.dh:][real])
    print(f'CTXATTN-WITNESS {CC.case_id(c)}: worst |got - count / (q + 1)| = {worst:.3f} fp16 ulp over {len(c.lengths)} lengths x 2 codes')


# (num_heads, batch, seq): shapes of growing 128-query workgroup counts, for the rule of whatever device is present
CANDIDATES = [(2, 2, 40), (2, 2, 130), (4, 3, 257), (8, 2, 300), (16, 2, 300), (32, 1, 300), (32, 2, 300), (32, 2, 512), (32, 2, 640),
              (32, 3, 640), (32, 4, 640), (32, 4, 1024)]


@pytest.mark.parametrize('kind', [CC.WAVE, CC.NARROW, CC.WIDE, CC.PAIRED], ids=lambda k: CC.KIND_NAME[k])
@pytest.mark.parametrize('dh', [64, 128])
def test_forced_equals_natural(lib, kind, dh):
    for H, B, S in CANDIDATES:
        c = CC.Case('natural-shape', kind, dh, H, H, tuple([S, S // 2, 1, S - 1][:B]), kv='int8')
        g = Geometry(c, c.lens)
        p = capi.AttentionParams(batch=B, seq=S, num_heads=H, head_size=dh, q_scaling=1.0, workspace=256)
        a = [ctypes.c_int32(-1) for _ in range(4)]
        assert lib.tllm_attention_context_layout(ctypes.byref(p), 0, *[ctypes.byref(x) for x in a]) == 0, capi.last_error()
        if a[0].value == kind:
            break
    else:
        print(f'CTXATTN-NATURAL {CC.KIND_NAME[kind]}-dh{dh}: the rule of this device chooses it at none of {CANDIDATES}; nothing compared')
        return
    qkv_in = inputs(c, g)
    natural = run_twice(lib, c, g, qkv_in, 0)
    forced = run_twice(lib, c, g, qkv_in, kind)
    assert natural.layout[0] == kind and same_bits(natural, forced), f'{CC.KIND_NAME[kind]} forced differs from the rule at H={H} B={B} S={S}'
    print(f'CTXATTN-NATURAL {CC.KIND_NAME[kind]}-dh{dh}: the rule chooses it at H={H} B={B} S={S} (layout {natural.layout}); forced run bit-identical')
