"""The split-KV append attention on the paged KV cache (tllm_attention_append_split_paged; the PG instances of
csrc/kernels/append_attn_split.hip) on the pool, table and inputs of tests/test_gpu_append_attention_paged.py, whose two entries are
swapped for the split ones: the linear split launch on the same logical cache bit for bit, and append_ref within its tolerance."""
import numpy as np
import pytest
import torch

import test_gpu_append_attention_paged as P
from tensorrt_llm.runtime.native import APPEND_ATTN_SPLIT, attention_append_split, attention_append_split_paged
from test_gpu_append_attention import B, GUARD, KV, check_run, make_case
from test_gpu_paged import gather_pool

pytestmark = pytest.mark.gpu

# (past, n, Hkv, Dh, T, masked profile, split_chunk); pasts per sequence are (p, p // 2, max(p - 1, 0))
CASES = [(0, 1, 2, 64, 8, 0, 64),        # no past: no table entry is read
         (5, 3, 2, 64, 4, 1, 64),        # 16 entries per block, few live
         (65, 5, 1, 128, 1, 1, 64),      # T = 1: all 64 + 64 ring entries; one key in the second range
         (64, 3, 2, 64, 64, 1, 64),      # block = page, one range exactly full
         (200, 8, 1, 128, 16, 1, 64),    # four ranges, two of them empty for the sequence at 100
         (200, 15, 2, 64, 128, 1, 64),   # two ranges per page, the seam mid-page
         (200, 17, 1, 64, 64, 0, 128),   # two pages per range, 34 columns
         (130, 32, 1, 128, 32, 1, 0)]    # largest n, the plan's own chunk


@pytest.fixture
def split(monkeypatch):
    """run_linear / run_paged of the paged file call the split entries (which have no append_kernel) with this chunk"""
    def use(chunk, table=True, **kw):
        monkeypatch.setattr(P, 'attention_append', lambda *a, append_kernel=0, **k: attention_append_split(
            *a, split_chunk=chunk, **kw, **k))
        monkeypatch.setattr(P, 'attention_append_paged', lambda q, pool, tab, *a, append_kernel=0, **k: attention_append_split_paged(
            q, pool, tab if table else None, *a, split_chunk=chunk, **kw, **k))
    return use


@pytest.mark.parametrize('kv', list(KV))
@pytest.mark.parametrize('case', CASES, ids=[f'p{c[0]}-n{c[1]}-kvh{c[2]}-d{c[3]}-T{c[4]}-m{c[5]}-c{c[6]}' for c in CASES])
def test_paged_split_equals_the_linear_split_launch_and_the_restatement(case, kv, split):
    past, n, Hkv, Dh, T, prof, chunk = case
    split(chunk)
    c = make_case(past, n, Hkv, Dh, prof, kv)
    tag = f'{kv} paged split c{chunk} p{past} n{n} Hkv{Hkv} Dh{Dh} T{T}'
    lin = P.run_linear(c, n, Hkv, Dh, APPEND_ATTN_SPLIT)
    got = P.run_paged(c, kv, n, Hkv, Dh, T, APPEND_ATTN_SPLIT)
    P.check_against_linear(c, lin, got, T, tag)
    check_run(c, dict(got, cache=gather_pool(got['pool_t'], got['table'], Hkv, T, Dh, c['smax'])), kv, n, Hkv, Dh, tag)
    again = P.run_paged(c, kv, n, Hkv, Dh, T, APPEND_ATTN_SPLIT)
    for k in ('qkv', 'out', 'pool'):
        P.same_bits(got[k], again[k], f'{tag}: {k} differs between two runs')


@pytest.mark.parametrize('kv', list(KV))
def test_ragged_lengths_equal_the_ragged_linear_split_launch(kv, split):
    n, Dh, T = 8, 128, 16
    split(64)
    c = make_case(200, n, 1, Dh, 1, kv)
    for per in ((8, 1, 0), (7, 8, 2)):
        ragged = (list(per), int(max(c['pasts'][b] + per[b] for b in range(B))))
        lin = P.run_linear(c, n, 1, Dh, APPEND_ATTN_SPLIT, ragged=ragged)
        got = P.run_paged(c, kv, n, 1, Dh, T, APPEND_ATTN_SPLIT, ragged=ragged)
        P.check_against_linear(c, lin, got, T, f'{kv} ragged paged split {per}')
        assert (lin['out'][:B * n].view(np.uint16) != GUARD).any()


@pytest.mark.parametrize('kv', list(KV))
@pytest.mark.parametrize('guard', [True, False], ids=['poisoned-spare-block', 'zero-entry'])
def test_blocks_wholly_behind_the_appended_slots_are_never_read(guard, kv, split):
    """the entries of every block behind p_b + n_b name one spare block full of NaN / 0x7f 0x80, or are 0"""
    past, n, Hkv, Dh, T, prof, chunk = CASES[4]
    split(chunk)
    c = make_case(past, n, Hkv, Dh, prof, kv)
    nblk, full = P.interleaved_ids(-(-c['smax'] // T))
    ids = [full[b][:-(-(int(c['pasts'][b]) + n) // T)] for b in range(B)]
    assert all(len(ids[b]) < len(full[b]) for b in range(B))
    got = P.run_paged(c, kv, n, Hkv, Dh, T, APPEND_ATTN_SPLIT, ids=ids, guard=guard, nblk=nblk)
    assert guard or (got['table'][:, 0, :, -1] == 0).all()
    P.check_against_linear(c, P.run_linear(c, n, Hkv, Dh, APPEND_ATTN_SPLIT), got, T, f'{kv} unmapped tail, guard {guard}')


def test_refusals_write_nothing(split):
    ws = torch.empty(1 << 20, dtype=torch.uint8, device='cuda')
    small = (16, 8, 1, 128, 16, 0)
    M = -(-make_case(16, 8, 1, 128, 0, 'fp16')['smax'] // 16)
    for what, case, kw, w, why in (('a NULL table', small, {}, None, 'block_pointers is null'),
                                   ('T = 48', small, dict(tpb=48), ws, 'power of two'),
                                   ('a table too short', small, dict(max_blocks=M - 1), ws, 'max_blocks_per_seq'),
                                   ('head size 32', (65, 5, 2, 32, 16, 1), {}, ws, 'head size 64 or 128'),
                                   ('n = 33', (64, 33, 2, 64, 16, 1), {}, ws, 'n <= 32'),
                                   ('workspace too small', small, {}, ws[:64], 'too small')):
        past, n, Hkv, Dh, T, prof = case
        split(64, table=w is not None, workspace=ws if w is None else w)
        c = make_case(past, n, Hkv, Dh, prof, 'fp16')
        got = P.run_paged(c, 'fp16', n, Hkv, Dh, T, APPEND_ATTN_SPLIT, **kw)
        assert got['err'] and why in got['err'], (what, got['err'])
        P.same_bits(got['pool'], got['init'], what)
        assert (got['out'].view(np.uint16) == GUARD).all(), what
        assert np.array_equal(got['qkv'][:B * n].view(np.uint16).ravel(), c['qkv'].view(np.uint16).ravel()), what
