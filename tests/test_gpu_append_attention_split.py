"""The split-KV append attention (csrc/kernels/append_attn_split.hip) through tllm_attention_append_split, held to what holds the
other two kernels: the cases, inputs, poison and bound of tests/test_gpu_append_attention.py (append_ref within
oracle.attention_oracle.tolerance, cache bytes by the store rule, guard rows, two runs bit for bit), its launchers with the entry
swapped for the new one."""
import functools

import numpy as np
import pytest
import torch

import test_gpu_append_attention as A
import test_gpu_append_attention_ragged as RG
from tensorrt_llm.runtime.native import APPEND_ATTN_SPLIT, attention_append_split
from test_gpu_append_attention import B, GUARD, H, KV, check_run, make_case

pytestmark = pytest.mark.gpu

# (past, n, Hkv, Dh, masked profile, split_chunk); pasts per sequence are (p, p // 2, max(p - 1, 0))
CASES = [(0, 1, 2, 64, 0, 64),       # no past: only the chunk range has keys
         (1, 2, 1, 128, 0, 64),      # one past key
         (64, 3, 2, 64, 1, 64),      # one range exactly full; another sequence at 63 and one at 32
         (65, 5, 1, 128, 1, 64),     # one key in the second range
         (200, 8, 1, 128, 1, 64),    # four ranges; two of them empty for the sequence with 100 slots
         (200, 15, 2, 64, 1, 128),   # another chunk length
         (200, 17, 1, 64, 0, 64),    # 34 columns: the second tile is partly filled and straddles the head boundary
         (130, 32, 1, 128, 1, 0)]    # the largest n, 64 columns (two tile groups), the plan's own chunk


def split_entry(*args, append_kernel=0, chunk=0, **kw):
    """attention_append's signature on the split entry (which has no append_kernel)"""
    attention_append_split(*args, split_chunk=chunk, **kw)


@pytest.fixture
def split(monkeypatch):
    """launch / launch_ragged of the two existing files call the split entry with this chunk"""
    def use(chunk, **kw):
        for mod in (A, RG):
            monkeypatch.setattr(mod, 'attention_append', functools.partial(split_entry, chunk=chunk, **kw))
    return use


@pytest.mark.parametrize('kv', list(KV))
@pytest.mark.parametrize('case', CASES, ids=[f'p{c[0]}-n{c[1]}-kvh{c[2]}-d{c[3]}-m{c[4]}-c{c[5]}' for c in CASES])
def test_split_append_attention_against_the_restatement(case, kv, split):
    past, n, Hkv, Dh, prof, chunk = case
    split(chunk)
    c = make_case(past, n, Hkv, Dh, prof, kv)
    tag = f'{kv} split c{chunk} p{past} n{n} Hkv{Hkv} Dh{Dh}'
    got = A.launch(c, kv, n, Hkv, Dh, APPEND_ATTN_SPLIT)
    check_run(c, got, kv, n, Hkv, Dh, tag)
    again = A.launch(c, kv, n, Hkv, Dh, APPEND_ATTN_SPLIT)
    for k in ('qkv', 'out', 'cache'):
        assert np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)), f'{tag}: {k} differs between two runs'


@pytest.mark.parametrize('kv', list(KV))
def test_every_visible_key_is_counted_exactly_once_across_the_range_seams(kv, split):
    """q = 0 and one-hot V rows (slot % Dh): out[b, i, h, d] = (visible keys of residue d) / (visible keys)"""
    past, n, Dh = 200, 8, 128
    split(64)
    c = make_case(past, n, 1, Dh, 1, kv, counting=True)
    got = A.launch(c, kv, n, 1, Dh, APPEND_ATTN_SPLIT)
    check_run(c, got, kv, n, 1, Dh, f'count {kv} split')
    out = got['out'][:B * n].view(np.float16).reshape(B, n, H, Dh).astype(np.float64)
    for b in range(B):
        p = int(c['pasts'][b])
        seen = np.nonzero(c['masked'][b, :p] == 0)[0]
        for i in range(n):
            slots = np.concatenate([seen, p + np.arange(i + 1)])
            want = np.bincount(slots % Dh, minlength=Dh) / len(slots)
            assert np.abs(out[b, i] - want[None, :]).max() < 0.25 / len(slots), (b, i)


def check_ragged(c, got, kv, n, lengths, Hkv, Dh, tag, monkeypatch):
    """RG.check_ragged; trailing sequences that append NOTHING (that helper's bound takes a maximum over the n_b rows) are held here -
    their out rows zero, their qkv rows and cache as sent - and the helper runs on the sequences in front of them"""
    nz = B
    while nz and lengths[nz - 1] == 0:
        nz -= 1
    for b in range(nz, B):
        assert (got['out'][b * n:(b + 1) * n] == 0).all(), f'{tag} b={b}: out rows are not exactly zero'
        assert np.array_equal(got['qkv'][b * n:(b + 1) * n].view(np.uint16), got['sent'][b]), f'{tag} b={b}: a padded qkv row was rewritten'
        assert np.array_equal(got['cache'][b].view(np.uint8), c['cache'][b].view(np.uint8)), f'{tag} b={b}: the cache was written'
    front = lambda a: np.concatenate([a[:nz * n], a[B * n:]])  # the first nz sequences' rows and the guard rows
    c = dict(c, pasts=c['pasts'][:nz], cache=c['cache'][:nz], masked=c['masked'][:nz])
    got = dict(got, qkv=front(got['qkv']), out=front(got['out']), cache=got['cache'][:nz], sent=got['sent'][:nz])
    with monkeypatch.context() as m:
        m.setattr(RG, 'B', nz)
        RG.check_ragged(c, got, kv, n, lengths[:nz], Hkv, Dh, tag)


@pytest.mark.parametrize('kv', list(KV))
@pytest.mark.parametrize('n,Dh', [(8, 128), (17, 64)])
def test_ragged_split_append_attention(n, Dh, kv, split, monkeypatch):
    """n_b per sequence, the padded qkv rows NaN: rows i >= n_b of out exactly zero, the rest within the tolerance"""
    split(64)
    c = make_case(200, n, 1, Dh, 1, kv)
    for lengths in ((n, 1, 0), (n - 1, n, 2)):
        tag = f'{kv} split ragged n{n} l{lengths} Dh{Dh}'
        got = RG.launch_ragged(c, n, lengths, 1, Dh, APPEND_ATTN_SPLIT)
        check_ragged(c, got, kv, n, lengths, 1, Dh, tag, monkeypatch)
        again = RG.launch_ragged(c, n, lengths, 1, Dh, APPEND_ATTN_SPLIT)
        assert np.array_equal(got['out'], again['out']), tag


def test_refusals_write_nothing(split):
    def refused(what, cc, n, Hkv, Dh, needle):
        got = A.launch(cc, 'fp16', n, Hkv, Dh, APPEND_ATTN_SPLIT)
        assert got['err'] and needle in got['err'], (what, got['err'])
        assert np.array_equal(got['cache'].view(np.uint16), cc['cache'].view(np.uint16)), what
        assert (got['out'].view(np.uint16) == GUARD).all(), what
        assert np.array_equal(got['qkv'][:B * n].view(np.uint16).ravel(), cc['qkv'].view(np.uint16).ravel()), what

    small = make_case(64, 3, 2, 64, 1, 'fp16')
    ws = torch.empty(1 << 20, dtype=torch.uint8, device='cuda')
    for what, chunk, w, needle in (('split_chunk 96', 96, ws, 'multiple of 64'), ('split_chunk -64', -64, ws, 'multiple of 64'),
                                   ('workspace null', 64, ws[:0], 'null'), ('workspace misaligned', 64, ws[8:], 'misaligned'),
                                   ('workspace too small', 64, ws[:64], 'too small')):
        split(chunk, workspace=w)
        refused(what, small, 3, 2, 64, needle)
    split(64)
    refused('head size 32', make_case(65, 5, 2, 32, 1, 'fp16'), 5, 2, 32, 'head size 64 or 128')
    refused('n = 33', make_case(64, 33, 2, 64, 1, 'fp16'), 33, 2, 64, 'n <= 32')
    # what launch_append_attention refuses for every kernel: max_past + n > Smax
    got = A.launch(small, 'fp16', 3, 2, 64, APPEND_ATTN_SPLIT, small['smax'] - 3 + 1)
    assert got['err'] and 'exceeds the cache capacity' in got['err'] and (got['out'].view(np.uint16) == GUARD).all()


def test_the_other_entries_refuse_the_split_kernel_by_name():
    """append_kernel = 3 through an entry without a workspace: refused, naming tllm_attention_append_split; the paged entry too"""
    small = make_case(64, 3, 2, 64, 1, 'fp16')
    for got in (A.launch(small, 'fp16', 3, 2, 64, APPEND_ATTN_SPLIT),
                RG.launch_ragged(small, 3, (3, 1, 2), 2, 64, APPEND_ATTN_SPLIT)):
        assert got['err'] and 'tllm_attention_append_split' in got['err'], got['err']
        assert (got['out'].view(np.uint16) == GUARD).all()
        assert np.array_equal(got['cache'].view(np.uint16), small['cache'].view(np.uint16))
    from tensorrt_llm.runtime.native import attention_append_paged
    t = torch.ones(1, dtype=torch.int32, device='cuda')
    qkv = torch.ones((1, 1, 3 * 64), dtype=torch.float16, device='cuda')
    pool = torch.zeros((2, 1, 64, 64), dtype=torch.float16, device='cuda')
    table = torch.tensor([[[pool[0].data_ptr()], [pool[1].data_ptr()]]], dtype=torch.int64, device='cuda')
    out = torch.ones((1, 1, 64), dtype=torch.float16, device='cuda')
    with pytest.raises(RuntimeError, match='tllm_attention_append_split'):
        attention_append_paged(qkv, pool, table, out, t, t, tokens_per_block=64, max_seq_len=64, num_heads=1, head_size=64,
                               max_input_len=1, max_past=1, append_kernel=APPEND_ATTN_SPLIT)
    torch.cuda.synchronize()
    assert (qkv == 1).all() and (pool == 0).all() and (out == 1).all()
