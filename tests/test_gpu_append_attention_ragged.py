"""The append attention with a different number of tokens per sequence (tllm_attention_append_ragged; csrc/kernels/append_attn.hip,
n_per_seq): B = 3 sequences append n_b <= n_max of their n_max rows.  The cases, their inputs and the bound are those of
tests/test_gpu_append_attention.py; on top of its poison (NaN / 0x7f 0x80 in every dead cache slot, guard rows behind qkv and out)
the padded rows of qkv - rows i >= n_b - hold fp16 NaN before the launch.  Held per case: the cache is written in [p_b, p_b + n_b)
alone and by the store rule, `out` below n_b lies within oracle.attention_oracle.tolerance of append_ref(..., lengths=...), `out`
from n_b on is exactly zero, the padded qkv rows keep their bits, the real ones carry RoPE, and a second run gives the same bits."""
import numpy as np
import pytest
import torch

from oracle import attention_oracle as AO
from tensorrt_llm.runtime import append_ref as R
from tensorrt_llm.runtime.native import APPEND_ATTN_MFMA, APPEND_ATTN_WAVE, attention_append

from test_gpu_append_attention import B, GUARD, H, KV, kernels_for, launch, make_case, pasts_of, rope_rows

pytestmark = pytest.mark.gpu
NAN16 = 0x7e00

# (past, n_max, lengths, Hkv, Dh): the smallest shapes at which each of the kernels' new decisions is taken both ways
WAVE_CASES = [(1, 5, (5, 1, 3), 2, 64), (200, 15, (15, 4, 9), 1, 128), (65, 5, (5, 2, 1), 2, 32), (65, 5, (1, 5, 4), 1, 256),
              (130, 70, (70, 64, 3), 2, 128)]
MFMA_CASES = [(0, 16, (16, 1, 7), 2, 64),       # no past; sequences below the kernel's own threshold
              (63, 70, (70, 64, 3), 1, 128),    # a second query block for one sequence only; one exactly full; one nearly empty
              (200, 129, (129, 65, 128), 2, 64),  # three blocks against two with one row against two full
              (64, 64, (17, 64, 33), 1, 64)]
# the wave cases run the wave kernel alone (as the table names it) except where both can run at N; the MFMA cases run both
ALL = [(c, k) for c in WAVE_CASES + MFMA_CASES for k in kernels_for(c[1], c[4])]


def launch_ragged(c, n, lengths, Hkv, Dh, kernel, max_end=None, poison=True):
    """test_gpu_append_attention.launch with n_per_seq; lengths None: the uniform entry on the same buffers"""
    dev = 'cuda'
    W = (H + 2 * Hkv) * Dh
    rows = c['qkv'].view(np.uint16).reshape(B, n, W).copy()
    if lengths is not None and poison:
        for b in range(B):
            rows[b, lengths[b]:] = NAN16
    qkv_full = torch.full((B * n + 4, W), GUARD, dtype=torch.int16, device=dev)
    qkv_full[:B * n] = torch.from_numpy(rows.view(np.int16).reshape(B * n, W)).to(dev)
    out_full = torch.full((B * n + 4, H * Dh), GUARD, dtype=torch.int16, device=dev)
    cache = torch.from_numpy(c['cache'].copy()).to(dev)
    seq = torch.from_numpy(c['pasts']).to(dev)
    lens = torch.from_numpy(c['lens']).to(dev)
    masked = None if c['masked'] is None else torch.from_numpy(c['masked']).to(dev)
    oq = None if c['oq'] is None else torch.tensor([c['oq']], dtype=torch.float32, device=dev)
    qo = None if c['qo'] is None else torch.tensor([c['qo']], dtype=torch.float32, device=dev)
    qkv = qkv_full[:B * n].view(torch.float16).view(B, n, W)
    out = out_full[:B * n].view(torch.float16).view(B, n, H * Dh)
    kw = dict(num_heads=H, num_kv_heads=Hkv, head_size=Dh, max_input_len=c['max_in'], masked_tokens=masked, kv_cache_type=c['code'],
              kv_scale_orig_quant=oq, kv_scale_quant_orig=qo, append_kernel=kernel)
    err = None
    try:
        if lengths is None:
            attention_append(qkv, cache, out, seq, lens, max_past=int(c['pasts'].max()), **kw)
        else:
            nps = torch.tensor(list(lengths), dtype=torch.int32, device=dev)
            if max_end is None:
                max_end = int((c['pasts'] + np.asarray(lengths)).max())
            attention_append(qkv, cache, out, seq, lens, n_per_seq=nps, max_end=max_end, **kw)
    except RuntimeError as e:
        err = str(e)
    torch.cuda.synchronize()
    return dict(qkv=qkv_full.cpu().numpy(), out=out_full.cpu().numpy(), cache=cache.cpu().numpy(), err=err, sent=rows)


def check_ragged(c, got, kv, n, lengths, Hkv, Dh, tag):
    """test_gpu_append_attention.check_run with the lengths: returns the launch's rows [B, n, W] as uint16"""
    W = (H + 2 * Hkv) * Dh
    assert got['err'] is None, got['err']
    bits = got['qkv'][:B * n].view(np.uint16).reshape(B, n, W)
    assert (got['qkv'][B * n:].view(np.uint16) == GUARD).all() and (got['out'][B * n:].view(np.uint16) == GUARD).all(), 'guard rows'
    for b in range(B):
        assert np.array_equal(bits[b, lengths[b]:], got['sent'][b, lengths[b]:]), f'{tag} b={b}: a padded qkv row was rewritten'
    rows = bits.view(np.float16)
    q16, k16, v16 = rows[..., :H * Dh], rows[..., H * Dh:(H + Hkv) * Dh], rows[..., (H + Hkv) * Dh:]
    # the cache: slots [p_b, p_b + n_b) hold the store rule of the launch's own rows, every other byte - [p_b + n_b, p_b + n_max)
    # included - is untouched
    want = c['cache'].copy()
    for b in range(B):
        p, nb = int(c['pasts'][b]), lengths[b]
        for j, src in ((0, k16), (1, v16)):
            want[b, j, :, p:p + nb] = R.store_rows(src[b, :nb].reshape(nb, Hkv, Dh).transpose(1, 0, 2), kv, c['oq'])
    same = want.view(np.uint8) == got['cache'].view(np.uint8)
    assert same.all(), f'{tag}: {int((~same).sum())} cache bytes differ from the store rule / were written outside [p_b, p_b + n_b)'
    ref, absmass = R.append_ref(q16, k16, v16, c['cache'], c['pasts'], H, Hkv, Dh, 1.0 / np.sqrt(Dh), kv, c['qo'], c['masked'],
                                lengths=lengths)
    out16 = got['out'][:B * n].view(np.uint16).reshape(B, n, H * Dh)
    out = out16.view(np.float16).astype(np.float64)
    for b in range(B):
        p, nb = int(c['pasts'][b]), lengths[b]
        assert (out16[b, nb:] == 0).all(), f'{tag} b={b}: out rows from n_b = {nb} on are not exactly zero'
        assert np.isfinite(out[b, :nb]).all(), f'{tag} b={b}: non-finite output (a padded row, or a masked or unused slot, was read)'
        vmax = max(np.abs(v16[b, :nb].astype(np.float64)).max(),
                   np.abs(np.nan_to_num(R.effective(c['cache'][b, 1, :, :p], kv, c['qo']))).max() if p else 0.0)
        tol = AO.tolerance(ref[b, :nb], absmass[b, :nb], p + nb, vmax)
        d = np.abs(out[b, :nb] - ref[b, :nb])
        print(f'[{tag} b={b} p={p} n_b={nb}] max |d| {d.max():.3e}, max d / tol {np.max(d / tol):.3f}')
        assert (d <= tol).all(), f'{tag} b={b}: {int((d > tol).sum())} elements outside the tolerance, worst {np.max(d / tol):.2f} x'
    return bits


@pytest.mark.parametrize('kv', list(KV))
@pytest.mark.parametrize('case,kernel', ALL, ids=[f'p{c[0]}-n{c[1]}-l{"_".join(map(str, c[2]))}-kvh{c[3]}-d{c[4]}-k{k}' for c, k in ALL])
def test_ragged_append_attention_against_the_restatement(case, kernel, kv):
    past, n, lengths, Hkv, Dh = case
    c = make_case(past, n, Hkv, Dh, 1, kv)
    tag = f'{kv} k{kernel} p{past} n{n} l{lengths} Hkv{Hkv} Dh{Dh}'
    got = launch_ragged(c, n, lengths, Hkv, Dh, kernel)
    bits = check_ragged(c, got, kv, n, lengths, Hkv, Dh, tag)
    # RoPE at the project's bound on the rows below n_b; v untouched
    want = rope_rows(past, n, Hkv, Dh, 1, kv)
    rows = bits.view(np.float16)
    for b in range(B):
        nb = lengths[b]
        np.testing.assert_allclose(rows[b, :nb, :(H + Hkv) * Dh].astype(np.float32), want[b, :nb, :(H + Hkv) * Dh], atol=2e-4, rtol=2e-3)
        assert np.array_equal(bits[b, :nb, (H + Hkv) * Dh:], c['qkv'][b, :nb, (H + Hkv) * Dh:].view(np.uint16))
    again = launch_ragged(c, n, lengths, Hkv, Dh, kernel)
    for k in ('qkv', 'out', 'cache'):
        assert np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)), f'{tag}: {k} differs between two runs'


@pytest.mark.parametrize('kv', list(KV))
@pytest.mark.parametrize('kernel,case', [(APPEND_ATTN_WAVE, (65, 5, 2, 32)), (APPEND_ATTN_MFMA, (63, 70, 1, 128))])
def test_lengths_all_equal_to_n_are_the_uniform_launch_bit_for_bit(kernel, case, kv):
    past, n, Hkv, Dh = case
    c = make_case(past, n, Hkv, Dh, 1, kv)
    uni = launch_ragged(c, n, None, Hkv, Dh, kernel)
    rag = launch_ragged(c, n, (n, n, n), Hkv, Dh, kernel)
    assert uni['err'] is None and rag['err'] is None, (uni['err'], rag['err'])
    for k in ('qkv', 'out', 'cache'):
        assert np.array_equal(uni[k].view(np.uint8), rag[k].view(np.uint8)), k
    # (and the helper's uniform launch is the existing file's)
    ref = launch(c, kv, n, Hkv, Dh, kernel)
    for k in ('qkv', 'out', 'cache'):
        assert np.array_equal(uni[k].view(np.uint8), ref[k].view(np.uint8)), k


@pytest.mark.parametrize('kv', list(KV))
@pytest.mark.parametrize('kernel', [APPEND_ATTN_WAVE, APPEND_ATTN_MFMA])
def test_every_visible_key_of_a_ragged_sequence_is_counted_exactly_once(kernel, kv):
    """the counting test of tests/test_gpu_append_attention.py (q = 0, one-hot V rows at slot % Dh) with lengths (70, 64, 3)"""
    past, n, Dh, lengths = 130, 70, 128, (70, 64, 3)
    c = make_case(past, n, 1, Dh, 1, kv, counting=True)
    got = launch_ragged(c, n, lengths, 1, Dh, kernel)
    check_ragged(c, got, kv, n, lengths, 1, Dh, f'count {kv} k{kernel}')
    out = got['out'][:B * n].view(np.float16).reshape(B, n, H, Dh).astype(np.float64)
    for b in range(B):
        p, nb = int(c['pasts'][b]), lengths[b]
        seen = np.ones(p, bool) & (c['masked'][b, :p] == 0)
        for i in sorted({0, nb // 2, nb - 1}):
            slots = np.concatenate([np.nonzero(seen)[0], p + np.arange(i + 1)])
            want = np.bincount(slots % Dh, minlength=Dh) / len(slots)
            assert np.abs(out[b, i] - want[None, :]).max() < 0.25 / len(slots), (b, i)


def small_cache_case():
    """pasts (40, 10, 10) with lengths (2, 30, 30) in a cache of 42: max_b (p_b + n_b) = 42 = Smax although max_past + n_max = 70"""
    r = np.random.default_rng(7)
    Hkv, Dh, n, smax = 2, 64, 30, 42
    pasts = np.array([40, 10, 10], np.int32)
    cache = r.standard_normal((B, 2, Hkv, smax, Dh)).astype(np.float16)
    for b in range(B):
        cache.view(np.uint16)[b][:, :, pasts[b]:] = NAN16
    return dict(pasts=pasts, smax=smax, max_in=10, lens=np.full(B, 10, np.int32), masked=None, cache=cache, qo=None, oq=None, code=0,
                qkv=r.standard_normal((B, n, (H + 2 * Hkv) * Dh)).astype(np.float16)), n, Hkv, Dh


def test_max_end_is_the_capacity_check():
    c, n, Hkv, Dh = small_cache_case()
    lengths = (2, 30, 30)
    for kernel in (APPEND_ATTN_WAVE, APPEND_ATTN_MFMA):
        # max_end > Smax is refused and writes nothing
        got = launch_ragged(c, n, lengths, Hkv, Dh, kernel, max_end=c['smax'] + 1)
        assert got['err'] and 'max_end' in got['err'], got['err']
        assert np.array_equal(got['cache'].view(np.uint16), c['cache'].view(np.uint16))
        assert (got['out'].view(np.uint16) == GUARD).all()
        assert np.array_equal(got['qkv'][:B * n].view(np.uint16).reshape(B, n, -1), got['sent'])
        # max_end == Smax is served, although max_past + n_max > Smax (which the uniform entry refuses)
        got = launch_ragged(c, n, lengths, Hkv, Dh, kernel, max_end=c['smax'])
        check_ragged(c, got, 'fp16', n, lengths, Hkv, Dh, f'full cache k{kernel}')
    uni = launch_ragged(c, n, None, Hkv, Dh, APPEND_ATTN_WAVE)
    assert uni['err'] and 'exceeds the cache capacity' in uni['err'], uni['err']


def test_n_per_seq_and_max_end_go_together():
    t = torch.ones(B, dtype=torch.int32, device='cuda')
    qkv = torch.zeros((B, 1, 3 * H * 64), dtype=torch.float16, device='cuda')
    cache = torch.zeros((B, 2, H, 4, 64), dtype=torch.float16, device='cuda')
    out = torch.zeros((B, 1, H * 64), dtype=torch.float16, device='cuda')
    for kw in (dict(n_per_seq=t), dict(max_end=2), dict()):
        with pytest.raises(ValueError):
            attention_append(qkv, cache, out, t, t, num_heads=H, head_size=64, max_input_len=1, **kw)
