"""The append attention (csrc/kernels/append_attn.hip) through tllm_attention_append, both kernels forced where both can run,
every cache type, against the float64 restatement tensorrt_llm/runtime/append_ref.py within oracle.attention_oracle.tolerance.

Every case runs B = 3 sequences with different past lengths p_b, H = 2 query heads on Hkv in {2, 1} K/V heads.  Before the launch
the masked slots and every slot >= p_b hold NaN (fp16) or the bytes 0x7f / 0x80, and guard rows lie behind qkv and out."""
import functools

import numpy as np
import pytest
import torch

from oracle import attention_oracle as AO
from oracle import llama_oracle as O
from tensorrt_llm.plugin import capi
from tensorrt_llm.runtime import append_ref as R
from tensorrt_llm.runtime.native import APPEND_ATTN_MFMA, APPEND_ATTN_WAVE, attention_append, attention_append_kernel

pytestmark = pytest.mark.gpu
B, H = 3, 2
KV = {'fp16': (0, torch.float16, None), 'int8': (capi.INT8, torch.int8, 1 / 32.0), 'fp8': (capi.FP8, torch.uint8, 1 / 16.0)}
GUARD = 0x7bff  # fp16 65504 in the guard rows

# (past, n, Hkv, Dh, masked profile) - pairs, not the product
MFMA_CASES = [(0, 16, 2, 64, 0), (1, 17, 1, 128, 0), (63, 63, 2, 128, 1), (64, 64, 1, 64, 1), (65, 65, 2, 64, 1),
              (200, 129, 1, 128, 1), (0, 64, 1, 128, 0), (200, 17, 2, 64, 0)]
WAVE_CASES = [(0, 1, 2, 64, 0), (1, 2, 1, 128, 0), (64, 3, 2, 64, 1), (200, 8, 1, 128, 1), (200, 15, 2, 64, 1), (64, 1, 1, 64, 0),
              (0, 15, 1, 128, 0), (1, 8, 2, 64, 1), (65, 5, 2, 32, 1), (65, 5, 1, 256, 1)]


def pasts_of(past):
    return np.array([past, past // 2, max(past - 1, 0)], np.int32)


@functools.lru_cache(maxsize=None)
def make_case(past, n, Hkv, Dh, masked_profile, kv, counting=False):
    """host arrays of one case (cached: both kernels get the same inputs and are held to the same reference)"""
    r = np.random.default_rng(1000 * past + n)
    code, _, qo = KV[kv]
    if counting and qo is not None:
        qo = 1.0
    pasts = pasts_of(past)
    smax = int(pasts.max()) + n + 3
    max_in = int(pasts.min())
    lens = np.full(B, max_in, np.int32)
    masked = None
    if masked_profile:
        lens = np.maximum(max_in - 2 * np.arange(B), min(1, max_in)).astype(np.int32)
        masked = np.zeros((B, smax), np.int32)
        for b in range(B):
            masked[b, lens[b]:max_in] = 1
    W = (H + 2 * Hkv) * Dh
    qkv = r.standard_normal((B, n, W)).astype(np.float16)
    if kv == 'fp16':
        cache = r.standard_normal((B, 2, Hkv, smax, Dh)).astype(np.float16)
    elif kv == 'int8':
        cache = r.integers(-127, 128, (B, 2, Hkv, smax, Dh)).astype(np.int8)
    else:
        cache = r.integers(0, 256, (B, 2, Hkv, smax, Dh)).astype(np.uint8)
        cache[(cache & 0x7f) == 0x7f] = 0x38
    if counting:
        # q = 0: every visible key weighs the same; V rows one-hot at slot % Dh: the output counts the keys of every residue
        qkv[:, :, :H * Dh] = 0
        one = {'fp16': np.float16(1.0), 'int8': np.int8(1), 'fp8': np.uint8(0x38)}[kv]
        cache[:, 1] = 0
        for t in range(smax):
            cache[:, 1, :, t, t % Dh] = one
        for b in range(B):
            for i in range(n):
                v = np.zeros(Dh, np.float16)
                v[(pasts[b] + i) % Dh] = 1
                qkv[b, i, (H + Hkv) * Dh:] = np.tile(v, Hkv)
    # what must never be read: masked slots and everything from p_b on
    flat = cache.view(np.uint16 if kv == 'fp16' else np.uint8)
    poison = np.uint16(0x7e00) if kv == 'fp16' else None
    for b in range(B):
        dead = np.zeros(smax, bool)
        dead[pasts[b]:] = True
        if masked is not None:
            dead |= masked[b] != 0
        if kv == 'fp16':
            flat[b][:, :, dead] = poison
        else:
            pat = np.where(np.arange(Dh) % 2 == 0, 0x7f, 0x80).astype(np.uint8)
            flat[b][:, :, dead] = pat
    return dict(pasts=pasts, smax=smax, max_in=max_in, lens=lens, masked=masked, qkv=qkv, cache=cache, qo=qo,
                oq=None if qo is None else 1.0 / qo, code=code)


def launch(c, kv, n, Hkv, Dh, kernel, max_past=None):
    dev = 'cuda'
    W = (H + 2 * Hkv) * Dh
    qkv_full = torch.full((B * n + 4, W), GUARD, dtype=torch.int16, device=dev)
    qkv_full[:B * n] = torch.from_numpy(c['qkv'].view(np.int16).reshape(B * n, W)).to(dev)
    out_full = torch.full((B * n + 4, H * Dh), GUARD, dtype=torch.int16, device=dev)
    cache = torch.from_numpy(c['cache'].copy()).to(dev)
    seq = torch.from_numpy(c['pasts']).to(dev)
    lens = torch.from_numpy(c['lens']).to(dev)
    masked = None if c['masked'] is None else torch.from_numpy(c['masked']).to(dev)
    oq = None if c['oq'] is None else torch.tensor([c['oq']], dtype=torch.float32, device=dev)
    qo = None if c['qo'] is None else torch.tensor([c['qo']], dtype=torch.float32, device=dev)
    qkv = qkv_full[:B * n].view(torch.float16).view(B, n, W)
    out = out_full[:B * n].view(torch.float16).view(B, n, H * Dh)
    err = None
    try:
        attention_append(qkv, cache, out, seq, lens, num_heads=H, num_kv_heads=Hkv, head_size=Dh, max_input_len=c['max_in'],
                         max_past=int(c['pasts'].max()) if max_past is None else max_past, masked_tokens=masked,
                         kv_cache_type=c['code'], kv_scale_orig_quant=oq, kv_scale_quant_orig=qo, append_kernel=kernel)
    except RuntimeError as e:
        err = str(e)
    torch.cuda.synchronize()
    return dict(qkv=qkv_full.cpu().numpy(), out=out_full.cpu().numpy(), cache=cache.cpu().numpy(), err=err)


@functools.lru_cache(maxsize=None)
def rope_rows(past, n, Hkv, Dh, masked_profile, kv):
    """apply_rope on the case's q and k rows at the rule's positions (float32 holding fp16 values)"""
    c = make_case(past, n, Hkv, Dh, masked_profile, kv)
    pos = R.positions(c['pasts'], n, c['max_in'], c['lens'])
    x = c['qkv'].astype(np.float32).reshape(B, n, H + 2 * Hkv, Dh)
    want = x.copy()
    for b in range(B):
        for i in range(n):
            want[b, i, :H + Hkv] = O.apply_rope(x[b, i, :H + Hkv], int(pos[b, i]), Dh, True)
    return want.reshape(B, n, -1)


def check_run(c, got, kv, n, Hkv, Dh, tag):
    """cache bytes, memory outside, and the output against append_ref on the launch's own rows"""
    W = (H + 2 * Hkv) * Dh
    assert got['err'] is None, got['err']
    rows = got['qkv'][:B * n].view(np.float16).reshape(B, n, W)
    assert (got['qkv'][B * n:].view(np.uint16) == GUARD).all() and (got['out'][B * n:].view(np.uint16) == GUARD).all(), 'guard rows'
    q16, k16, v16 = rows[..., :H * Dh], rows[..., H * Dh:(H + Hkv) * Dh], rows[..., (H + Hkv) * Dh:]
    # the cache: slots [p_b, p_b + n) hold the store rule of the launch's own k and v rows, every other byte is untouched
    want = c['cache'].copy()
    for b in range(B):
        p = int(c['pasts'][b])
        for j, src in ((0, k16), (1, v16)):
            want[b, j, :, p:p + n] = R.store_rows(src[b].reshape(n, Hkv, Dh).transpose(1, 0, 2), kv, c['oq'])
    same = want.view(np.uint8) == got['cache'].view(np.uint8)
    assert same.all(), f'{tag}: {int((~same).sum())} cache bytes differ from the store rule / were written outside [p_b, p_b + n)'
    ref, absmass = R.append_ref(q16, k16, v16, c['cache'], c['pasts'], H, Hkv, Dh, 1.0 / np.sqrt(Dh), kv, c['qo'], c['masked'])
    out = got['out'][:B * n].view(np.float16).reshape(B, n, H * Dh).astype(np.float64)
    assert np.isfinite(out).all(), f'{tag}: non-finite output (a masked or unused slot was read)'
    for b in range(B):
        p = int(c['pasts'][b])
        vmax = max(np.abs(v16[b].astype(np.float64)).max(),
                   np.abs(np.nan_to_num(R.effective(c['cache'][b, 1, :, :p], kv, c['qo']))).max() if p else 0.0)
        tol = AO.tolerance(ref[b], absmass[b], p + n, vmax)
        d = np.abs(out[b] - ref[b])
        print(f'[{tag} b={b} p={p}] max |d| {d.max():.3e}, max d / tol {np.max(d / tol):.3f}')
        assert (d <= tol).all(), f'{tag} b={b}: {int((d > tol).sum())} elements outside the tolerance, worst {np.max(d / tol):.2f} x'
    return rows


def kernels_for(n, Dh):
    ks = [APPEND_ATTN_WAVE]
    if n >= 16 and Dh in (64, 128):
        ks.append(APPEND_ATTN_MFMA)
    return ks


ALL = [(c, k) for c in MFMA_CASES + WAVE_CASES for k in kernels_for(c[1], c[3])]


@pytest.mark.parametrize('kv', list(KV))
@pytest.mark.parametrize('case,kernel', ALL, ids=[f'p{c[0]}-n{c[1]}-kvh{c[2]}-d{c[3]}-m{c[4]}-k{k}' for c, k in ALL])
def test_append_attention_against_the_restatement(case, kernel, kv):
    past, n, Hkv, Dh, prof = case
    c = make_case(past, n, Hkv, Dh, prof, kv)
    assert prof == 0 or (c['lens'] < c['max_in']).any() or c['max_in'] == 0
    tag = f'{kv} k{kernel} p{past} n{n} Hkv{Hkv} Dh{Dh}'
    got = launch(c, kv, n, Hkv, Dh, kernel)
    rows = check_run(c, got, kv, n, Hkv, Dh, tag)
    # RoPE at the project's bound; v untouched
    W = (H + 2 * Hkv) * Dh
    want = rope_rows(past, n, Hkv, Dh, prof, kv)
    np.testing.assert_allclose(rows[..., :(H + Hkv) * Dh].astype(np.float32), want[..., :(H + Hkv) * Dh], atol=2e-4, rtol=2e-3)
    assert np.array_equal(rows[..., (H + Hkv) * Dh:].view(np.uint16), c['qkv'][..., (H + Hkv) * Dh:].view(np.uint16))
    # determinism: a second run from the same inputs gives the same bits
    again = launch(c, kv, n, Hkv, Dh, kernel)
    for k in ('qkv', 'out', 'cache'):
        assert np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)), f'{tag}: {k} differs between two runs'


def test_the_rule_picks_the_mfma_kernel_where_it_serves():
    assert attention_append_kernel(16, 64) == APPEND_ATTN_MFMA and attention_append_kernel(129, 128) == APPEND_ATTN_MFMA
    assert attention_append_kernel(15, 64) == APPEND_ATTN_WAVE and attention_append_kernel(64, 32) == APPEND_ATTN_WAVE
    assert attention_append_kernel(64, 256) == APPEND_ATTN_WAVE


@pytest.mark.parametrize('kv', list(KV))
@pytest.mark.parametrize('kernel,past,n,Dh', [(APPEND_ATTN_WAVE, 200, 15, 64), (APPEND_ATTN_WAVE, 130, 70, 128),
                                               (APPEND_ATTN_MFMA, 200, 129, 64), (APPEND_ATTN_MFMA, 130, 70, 128)])
def test_every_visible_key_is_counted_exactly_once(kernel, past, n, Dh, kv):
    """q = 0 and one-hot V rows (slot % Dh): out[b, i, h, d] = (visible keys of residue d) / (visible keys).  A dropped, doubled
    or masked-but-read key moves an element by 1 / (visible keys) - far outside the tolerance - or makes it NaN."""
    c = make_case(past, n, 1, Dh, 1, kv, counting=True)
    got = launch(c, kv, n, 1, Dh, kernel)
    check_run(c, got, kv, n, 1, Dh, f'count {kv} k{kernel}')
    # and the expected counts themselves, independent of append_ref
    out = got['out'][:B * n].view(np.float16).reshape(B, n, H, Dh).astype(np.float64)
    for b in range(B):
        p = int(c['pasts'][b])
        seen = np.ones(p, bool) & (c['masked'][b, :p] == 0)
        for i in (0, n // 2, n - 1):
            slots = np.concatenate([np.nonzero(seen)[0], p + np.arange(i + 1)])
            want = np.bincount(slots % Dh, minlength=Dh) / len(slots)
            assert np.abs(out[b, i] - want[None, :]).max() < 0.25 / len(slots), (b, i)


def test_refusals_write_nothing():
    c = make_case(64, 16, 2, 64, 1, 'fp16')
    c32 = make_case(65, 5, 2, 32, 1, 'fp16')
    small = make_case(64, 3, 2, 64, 1, 'fp16')
    for what, cc, n, Hkv, Dh, kernel, max_past in (
            ('max_past + n > Smax', c, 16, 2, 64, 0, c['smax'] - 16 + 1),
            ('MFMA forced at n < 16', small, 3, 2, 64, APPEND_ATTN_MFMA, None),
            ('MFMA forced at head size 32', c32, 5, 2, 32, APPEND_ATTN_MFMA, None)):
        got = launch(cc, 'fp16', n, Hkv, Dh, kernel, max_past)
        assert got['err'], what
        assert np.array_equal(got['cache'].view(np.uint16), cc['cache'].view(np.uint16)), what
        assert (got['out'].view(np.uint16) == GUARD).all(), what
        assert np.array_equal(got['qkv'][:B * n].view(np.uint16).ravel(), cc['qkv'].view(np.uint16).ravel()), what
    # num_kv_heads that does not divide num_heads: H = 3 query heads on 2 K/V heads (the buffers are sized for it)
    Hq, Hkv, Dh, n = 3, 2, 64, 4
    dev = 'cuda'
    qkv = torch.ones((1, n, (Hq + 2 * Hkv) * Dh), dtype=torch.float16, device=dev)
    cache = torch.zeros((1, 2, Hkv, 16, Dh), dtype=torch.float16, device=dev)
    out = torch.ones((1, n, Hq * Dh), dtype=torch.float16, device=dev)
    z = torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match='num_kv_heads'):
        attention_append(qkv, cache, out, z, z, num_heads=Hq, num_kv_heads=Hkv, head_size=Dh, max_input_len=0, max_past=0)
    torch.cuda.synchronize()
    assert (qkv == 1).all() and (cache == 0).all() and (out == 1).all()
