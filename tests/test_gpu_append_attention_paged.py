"""The append attention on the paged KV cache (tllm_attention_append_paged; csrc/kernels/append_attn.hip, the paged instances).

Paging only changes WHERE a K/V row lives, so the oracle is the linear launch on the same logical cache and the check is
assert_array_equal, never a tolerance (the linear kernels are held to append_ref.py in test_gpu_append_attention.py).  Inputs are
that file's make_case - B = 3 sequences with different past lengths p_b, H = 2 - scattered into a pool whose physical blocks
interleave across the sequences in DESCENDING address order (logical block j of sequence b is block id top - (j * B + b)), with
spare blocks below and above them.  The pool is pre-filled with the byte 0xa5; after every launch the WHOLE pool is compared with
what the linear launch left in its cache, scattered the same way - so a store outside the slots [p_b, p_b + n_b) of a sequence's own
blocks, in a spare block, in another head's rows or in another sequence's block, fails every test here.

Which sequence meets which block edge (pasts_of(past) = [past, past // 2, max(past - 1, 0)]; test_the_cases_meet_every_block_edge
holds this table to the code):
  (5, 3, T 4)      slots 5-7 / 2-4 / 4-6:  b = 1 starts mid-block and crosses a boundary, b = 2 starts exactly on a boundary,
                                           b = 0 ends exactly on a block's last row;
  (16, 8, T 16)    slots 16-23 / 8-15 / 15-22:  b = 0 starts on a boundary, b = 1 ends on a last row, b = 2 crosses;
  (63, 63, T 16)   slots 63-125 / 31-93 / 62-124:  all three start mid-block and cross several boundaries;
  (64, 64, T 64)   slots 64-127 / 32-95 / 63-126:  b = 0 starts on a boundary AND ends on a last row, b = 1 and b = 2 cross;
  (200, 129, T 128) slots 200-328 / 100-228 / 199-327:  all three cross one boundary mid-chunk."""
import functools

import numpy as np
import pytest
import torch

from tensorrt_llm.runtime.kv_cache_manager import GenerationSequence, KVCacheManager
from tensorrt_llm.runtime.native import APPEND_ATTN_MFMA, APPEND_ATTN_WAVE, attention_append, attention_append_paged
from test_gpu_append_attention import B, GUARD, H, KV, kernels_for, make_case
from test_gpu_paged import gather_pool

pytestmark = pytest.mark.gpu
FILL = 0xa5  # the pool before the cache is scattered into it

# (past, n, Hkv, Dh, T, masked profile): the masked profile on six of the ten
WAVE_CASES = [(5, 3, 2, 64, 4, 1), (16, 8, 1, 128, 16, 0), (65, 5, 2, 32, 64, 1), (65, 5, 1, 256, 1, 1), (0, 15, 1, 128, 8, 0)]
MFMA_CASES = [(63, 63, 2, 128, 16, 1), (64, 64, 1, 64, 64, 1), (200, 129, 1, 128, 128, 1), (1, 17, 1, 128, 32, 0),
              (0, 16, 2, 64, 64, 0)]
ALL = [(c, k) for c in WAVE_CASES + MFMA_CASES for k in kernels_for(c[1], c[3])]
IDS = [f'p{c[0]}-n{c[1]}-kvh{c[2]}-d{c[3]}-T{c[4]}-m{c[5]}-k{k}' for c, k in ALL]


def np_dtype(kv):
    return {'fp16': np.float16, 'int8': np.int8, 'fp8': np.uint8}[kv]


def interleaved_ids(M):
    """logical block j of sequence b -> physical block id: interleaved across the sequences, descending; ids 0, 1 and the top one
    stay spare"""
    nblk = B * M + 3
    return nblk, [[nblk - 2 - (j * B + b) for j in range(M)] for b in range(B)]


def scatter(cache, ids, pool, nblk, T):
    """rows of the linear cache [B, 2, Hkv, smax, Dh] into pool [2 * nblk, Hkv, T, Dh] (K block i at i, its V block at nblk + i)"""
    smax = cache.shape[3]
    for b in range(B):
        for j, i in enumerate(ids[b]):
            if i is None or j * T >= smax:
                continue
            rows = min(T, smax - j * T)
            for two in range(2):
                pool[two * nblk + i][:, :rows] = cache[b, two, :, j * T:j * T + rows]


def device_inputs(c, n, Hkv, Dh):
    dev = 'cuda'
    W = (H + 2 * Hkv) * Dh
    qkv_full = torch.full((B * n + 4, W), GUARD, dtype=torch.int16, device=dev)
    qkv_full[:B * n] = torch.from_numpy(c['qkv'].view(np.int16).reshape(B * n, W)).to(dev)
    out_full = torch.full((B * n + 4, H * Dh), GUARD, dtype=torch.int16, device=dev)
    t = dict(qkv_full=qkv_full, out_full=out_full, seq=torch.from_numpy(c['pasts']).to(dev), lens=torch.from_numpy(c['lens']).to(dev),
             masked=None if c['masked'] is None else torch.from_numpy(c['masked']).to(dev),
             oq=None if c['oq'] is None else torch.tensor([c['oq']], dtype=torch.float32, device=dev),
             qo=None if c['qo'] is None else torch.tensor([c['qo']], dtype=torch.float32, device=dev))
    t['qkv'] = qkv_full[:B * n].view(torch.float16).view(B, n, W)
    t['out'] = out_full[:B * n].view(torch.float16).view(B, n, H * Dh)
    return t


def common_args(c, t, Hkv, Dh, kernel, ragged, max_past):
    a = dict(num_heads=H, num_kv_heads=Hkv, head_size=Dh, max_input_len=c['max_in'], masked_tokens=t['masked'],
             kv_cache_type=c['code'], kv_scale_orig_quant=t['oq'], kv_scale_quant_orig=t['qo'], append_kernel=kernel)
    if ragged is None:
        a['max_past'] = int(c['pasts'].max()) if max_past is None else max_past
    else:
        a['n_per_seq'] = torch.tensor(ragged[0], dtype=torch.int32, device='cuda')
        a['max_end'] = ragged[1]
    return a


def finish(t, err, **more):
    torch.cuda.synchronize()
    return dict(qkv=t['qkv_full'].cpu().numpy(), out=t['out_full'].cpu().numpy(), err=err, **more)


def run_linear(c, n, Hkv, Dh, kernel, ragged=None):
    """ragged: (n_per_seq, max_end) or None"""
    t = device_inputs(c, n, Hkv, Dh)
    cache = torch.from_numpy(c['cache'].copy()).to('cuda')
    attention_append(t['qkv'], cache, t['out'], t['seq'], t['lens'], **common_args(c, t, Hkv, Dh, kernel, ragged, None))
    return finish(t, None, cache=cache.cpu().numpy())


def run_paged(c, kv, n, Hkv, Dh, T, kernel, ids=None, guard=False, ragged=None, max_past=None, tpb=None, max_blocks=None, nblk=None):
    """ids[b][j]: the physical block of logical block j of sequence b, None = unmapped (table entry 0, or - guard - the address of
    spare block 0, which is then filled with what must never be read).  tpb / max_blocks: what the launch is TOLD (refusals)."""
    smax = c['smax']
    M = -(-smax // T)
    if ids is None:
        nblk, ids = interleaved_ids(M)
    ids = [list(r) + [None] * (M - len(r)) for r in ids]
    pool = np.full((2 * nblk, Hkv, T, Dh), FILL, np.uint8).repeat(np.dtype(np_dtype(kv)).itemsize, axis=-1).view(np_dtype(kv))
    if guard:
        poison = np.full(Dh, 0x7e00, np.uint16).view(np.float16) if kv == 'fp16' else \
            np.where(np.arange(Dh) % 2 == 0, 0x7f, 0x80).astype(np.uint8).view(np_dtype(kv))
        pool[0], pool[nblk] = poison, poison
    scatter(c['cache'], ids, pool, nblk, T)
    pool_t = torch.from_numpy(pool.copy()).to('cuda')
    base, nbytes = pool_t.data_ptr(), Hkv * T * Dh * pool.itemsize
    table = np.zeros((B, 1, 2, M), np.int64)
    for b in range(B):
        for j, i in enumerate(ids[b]):
            if i is None and not guard:
                continue
            table[b, 0, 0, j] = base + (0 if i is None else i) * nbytes
            table[b, 0, 1, j] = base + (nblk + (0 if i is None else i)) * nbytes
    t = device_inputs(c, n, Hkv, Dh)
    told = table[:, 0] if max_blocks is None else table[:, 0, :, :max_blocks]
    err = None
    try:
        attention_append_paged(t['qkv'], pool_t, torch.from_numpy(np.ascontiguousarray(told)).to('cuda'), t['out'], t['seq'], t['lens'],
                               tokens_per_block=T if tpb is None else tpb, max_seq_len=smax,
                               **common_args(c, t, Hkv, Dh, kernel, ragged, max_past))
    except RuntimeError as e:
        err = str(e)
    return finish(t, err, pool=pool_t.cpu().numpy(), pool_t=pool_t, init=pool, table=table, ids=ids, nblk=nblk)


def same_bits(a, b, what):
    np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg=what)


def check_against_linear(c, lin, got, T, tag):
    """qkv (RoPE in place), out, the guard rows behind both, and the whole pool against the linear launch's cache scattered over
    the pool as it was"""
    assert got['err'] is None, got['err']
    same_bits(got['qkv'], lin['qkv'], f'{tag}: qkv')
    same_bits(got['out'], lin['out'], f'{tag}: out')
    want = got['init'].copy()
    scatter(lin['cache'], got['ids'], want, got['nblk'], T)
    same_bits(got['pool'], want, f'{tag}: pool bytes (a store that is missing, or one outside the slots [p_b, p_b + n_b) of a '
                                 f'sequence\'s own blocks)')


@functools.lru_cache(maxsize=None)
def linear_run(case, kernel, kv):
    past, n, Hkv, Dh, T, prof = case
    return run_linear(make_case(past, n, Hkv, Dh, prof, kv), n, Hkv, Dh, kernel)


@functools.lru_cache(maxsize=None)
def full_run(case, kernel, kv):
    """the fully mapped paged launch of a case (shared, never modified: the on-demand test compares against it)"""
    past, n, Hkv, Dh, T, prof = case
    return run_paged(make_case(past, n, Hkv, Dh, prof, kv), kv, n, Hkv, Dh, T, kernel)


# ------------------------------------------------------------------------------------------------ 1. paged equals linear
@pytest.mark.parametrize('kv', list(KV))
@pytest.mark.parametrize('case,kernel', ALL, ids=IDS)
def test_paged_equals_linear_bit_for_bit(case, kernel, kv):
    past, n, Hkv, Dh, T, prof = case
    c = make_case(past, n, Hkv, Dh, prof, kv)
    lin, got = linear_run(case, kernel, kv), full_run(case, kernel, kv)
    tag = f'{kv} k{kernel} p{past} n{n} Hkv{Hkv} Dh{Dh} T{T}'
    check_against_linear(c, lin, got, T, tag)
    # and the pool read back through the table IS the linear cache
    np.testing.assert_array_equal(gather_pool(got['pool_t'], got['table'], Hkv, T, Dh, c['smax']).view(np.uint8),
                                  lin['cache'].view(np.uint8))
    assert (lin['out'][:B * n].view(np.uint16) != GUARD).any()


def test_the_cases_meet_every_block_edge():
    """the table of the module docstring, from the numbers"""
    def edges(past, n, T):
        p = np.array([past, past // 2, max(past - 1, 0)])
        mid_cross = [int(b) for b in range(B) if p[b] % T and p[b] // T != (p[b] + n - 1) // T]
        on_boundary = [int(b) for b in range(B) if p[b] % T == 0]
        last_row = [int(b) for b in range(B) if (p[b] + n) % T == 0]
        return mid_cross, on_boundary, last_row
    assert edges(5, 3, 4) == ([1], [2], [0])
    assert edges(16, 8, 16) == ([2], [0], [1])
    assert edges(63, 63, 16) == ([0, 1, 2], [], [])
    assert edges(64, 64, 64) == ([1, 2], [0], [0])
    assert edges(200, 129, 128) == ([0, 1, 2], [], [])
    # the blocks of a sequence are neither contiguous nor ascending
    nblk, ids = interleaved_ids(4)
    assert all(ids[b][j] - ids[b][j + 1] == B for b in range(B) for j in range(3)) and ids[0][0] == nblk - 2
    assert sum(c[5] for c in WAVE_CASES + MFMA_CASES) * 2 >= len(WAVE_CASES + MFMA_CASES)


# ------------------------------------------------------------------------------------------------ 2. ragged
@pytest.mark.parametrize('kv', list(KV))
@pytest.mark.parametrize('case,kernel', [((5, 3, 2, 64, 4, 1), APPEND_ATTN_WAVE), ((63, 63, 2, 128, 16, 1), APPEND_ATTN_MFMA),
                                         ((63, 63, 2, 128, 16, 1), APPEND_ATTN_WAVE)], ids=['wave-T4', 'mfma-T16', 'wave-T16'])
def test_ragged_lengths_equal_the_ragged_linear_launch(case, kernel, kv):
    past, n, Hkv, Dh, T, prof = case
    c = make_case(past, n, Hkv, Dh, prof, kv)
    per = [n + 5, 0, max(n // 2, 1)]  # above n and 0: both clamped on the device
    max_end = int(max(c['pasts'][b] + min(per[b], n) for b in range(B)))
    lin = run_linear(c, n, Hkv, Dh, kernel, ragged=(per, max_end))
    got = run_paged(c, kv, n, Hkv, Dh, T, kernel, ragged=(per, max_end))
    check_against_linear(c, lin, got, T, f'ragged {kv} k{kernel}')
    assert (got['out'][n:2 * n] == 0).all(), 'the rows of a sequence that appends nothing are zeros'
    # every store counted once: outside the slots [p_b, p_b + n_b) of the sequences' own blocks no byte of the pool moved
    touched = np.zeros(got['pool'].shape[:3], bool)  # [block, head, row]
    for b in range(B):
        for s in range(int(c['pasts'][b]), int(c['pasts'][b]) + min(per[b], n)):
            for two in range(2):
                touched[two * got['nblk'] + got['ids'][b][s // T], :, s % T] = True
    moved = (got['pool'].view(np.uint8) != got['init'].view(np.uint8)).reshape(touched.shape + (-1, )).any(-1)
    assert not (moved & ~touched).any(), 'a byte outside the appended slots moved'
    assert moved[touched].mean() > 0.9, 'the appended slots were written'
    # lengths all equal to n: the uniform paged launch
    uni = run_paged(c, kv, n, Hkv, Dh, T, kernel, ragged=([n] * B, int(c['pasts'].max()) + n))
    ref = full_run(case, kernel, kv)
    for k in ('qkv', 'out', 'pool'):
        same_bits(uni[k], ref[k], f'n_per_seq = n against the uniform launch: {k}')


# ------------------------------------------------------------------------------------------------ 3. every store counted once
@pytest.mark.parametrize('kv', list(KV))
@pytest.mark.parametrize('case,kernel', [((65, 5, 2, 32, 64, 1), APPEND_ATTN_WAVE), ((200, 129, 1, 128, 128, 1), APPEND_ATTN_MFMA),
                                         ((16, 8, 1, 128, 16, 0), APPEND_ATTN_WAVE)], ids=['T64', 'T128', 'T16'])
def test_every_store_lands_once_in_the_sequences_own_blocks(case, kernel, kv):
    """the pool holds 0xa5 in its spare blocks and in the rows behind the capacity; after the launch exactly the bytes of the
    slots [p_b, p_b + n) of every K/V head of the sequences' own blocks may differ from before - and they hold the linear
    launch's rows (check_against_linear)"""
    past, n, Hkv, Dh, T, prof = case
    c = make_case(past, n, Hkv, Dh, prof, kv)
    got = full_run(case, kernel, kv)
    touched = np.zeros(got['pool'].shape[:3], bool)
    for b in range(B):
        for s in range(int(c['pasts'][b]), int(c['pasts'][b]) + n):
            for two in range(2):
                touched[two * got['nblk'] + got['ids'][b][s // T], :, s % T] = True
    moved = (got['pool'].view(np.uint8) != got['init'].view(np.uint8)).reshape(touched.shape + (-1, )).any(-1)
    assert not (moved & ~touched).any()
    for spare in (0, 1, got['nblk'] - 1):
        for two in range(2):
            assert (got['pool'][two * got['nblk'] + spare].view(np.uint8) == FILL).all(), f'spare block {spare}'


# ------------------------------------------------------------------------------------------------ 4. on-demand table
def on_demand_ids(c, n, T, nblk):
    """what KVCacheManager.extend maps for p_b + n tokens: ceil((p_b + n) / T) blocks per sequence (block 0 is kept out of the
    manager's hands: it is the guard)"""
    M = -(-c['smax'] // T)
    mgr = KVCacheManager([np.zeros(2 * nblk * 8, np.uint8)], nblk, T, M)
    keep = GenerationSequence(99, B)
    mgr.blocks_manager.allocate(keep)  # block 0
    for b in range(B):
        mgr.add_sequence(GenerationSequence(b, b), 0)
    mgr.extend([int(p) + n for p in c['pasts']])
    ids = [mgr.blocks_manager.block_ids(s)[0] for s in mgr.sequences]
    assert [len(r) for r in ids] == [-(-(int(p) + n) // T) for p in c['pasts']] and all(0 not in r for r in ids)
    return ids


@pytest.mark.parametrize('kv', list(KV))
@pytest.mark.parametrize('case,kernel', ALL, ids=IDS)
def test_on_demand_table_with_the_rest_on_a_guard_block(case, kernel, kv):
    """only ceil((p_b + n) / T) blocks per sequence are mapped (KVCacheManager.extend); every other entry names ONE spare block
    full of NaN (fp16) / 0x7f 0x80: the results are the fully mapped run's, so no unmapped entry contributes a value"""
    past, n, Hkv, Dh, T, prof = case
    c = make_case(past, n, Hkv, Dh, prof, kv)
    nblk = B * -(-c['smax'] // T) + 3
    ids = on_demand_ids(c, n, T, nblk)
    got = run_paged(c, kv, n, Hkv, Dh, T, kernel, ids=ids, guard=True, nblk=nblk)
    ref = full_run(case, kernel, kv)
    assert got['err'] is None, got['err']
    same_bits(got['qkv'], ref['qkv'], 'qkv')
    same_bits(got['out'], ref['out'], 'out')
    check_against_linear(c, linear_run(case, kernel, kv), got, T, f'on demand {kv} k{kernel}')  # (the guard block unchanged too)


def test_a_zero_entry_behind_the_last_needed_block_changes_nothing():
    """the zero-entry contract, first of two: the MFMA kernel's K loads are unconditional - a 64-key tile reaches past p_b into
    logical blocks whose table entries are 0 - and no address may be formed from such an entry"""
    case, kv = (63, 63, 2, 128, 16, 1), 'fp16'
    past, n, Hkv, Dh, T, prof = case
    c = make_case(past, n, Hkv, Dh, prof, kv)
    nblk, full = interleaved_ids(-(-c['smax'] // T))
    ids = [full[b][:-(-(int(c['pasts'][b]) + n) // T)] for b in range(B)]
    assert all(len(ids[b]) < len(full[b]) for b in range(B))
    got = run_paged(c, kv, n, Hkv, Dh, T, APPEND_ATTN_MFMA, ids=ids, nblk=nblk)
    assert (got['table'][:, 0, :, -1] == 0).all()
    check_against_linear(c, linear_run(case, APPEND_ATTN_MFMA, kv), got, T, 'zero entries behind the needed blocks')


def test_a_zero_entry_on_a_slot_to_be_stored_skips_that_store():
    """the zero-entry contract, second of two: sequence 1 appends to slots 2 - 4 (T = 4) and its block 1 - slot 4 - is not mapped:
    slots 2 and 3 are stored, the store of slot 4 is skipped, nothing else in the pool moves, `out` is what it would have been
    (the appended tokens' own k and v come from the QKV buffer) and the call reports no error"""
    case, kv = (5, 3, 2, 64, 4, 1), 'fp16'
    past, n, Hkv, Dh, T, prof = case
    c = make_case(past, n, Hkv, Dh, prof, kv)
    nblk, ids = interleaved_ids(-(-c['smax'] // T))
    assert list(c['pasts']) == [5, 2, 4]
    ids[1][1] = None
    got = run_paged(c, kv, n, Hkv, Dh, T, APPEND_ATTN_WAVE, ids=ids, nblk=nblk)
    assert got['table'][1, 0, 0, 1] == 0 and got['table'][1, 0, 1, 1] == 0
    check_against_linear(c, linear_run(case, APPEND_ATTN_WAVE, kv), got, T, 'zero entry on a stored slot')
    # (check_against_linear scatters the linear cache through the same table: the unmapped block receives nothing)
    lost = interleaved_ids(-(-c['smax'] // T))[1][1][1]
    for two in range(2):
        assert (got['pool'][two * nblk + lost].view(np.uint8) == got['init'][two * nblk + lost].view(np.uint8)).all()


# ------------------------------------------------------------------------------------------------ 5. shared read-only blocks
@pytest.mark.parametrize('kernel', [APPEND_ATTN_WAVE, APPEND_ATTN_MFMA])
@pytest.mark.parametrize('kv', ['fp16', 'int8'])
def test_two_sequences_that_share_their_prefix_blocks(kernel, kv):
    """sequences 0 and 1 (p_b = 64 and 32, T = 16) name the SAME two physical blocks for slots 0 - 31, which lie below both p_b:
    each equals its linear run on a cache that holds those rows twice.  (The kernel precondition of prefix sharing.)"""
    past, n, Hkv, Dh, T = 64, 17, 2, 64, 16
    base_case = make_case(past, n, Hkv, Dh, 0, kv)
    assert list(base_case['pasts'][:2]) == [64, 32]
    c = dict(base_case, cache=base_case['cache'].copy())
    c['cache'][1, :, :, :32] = c['cache'][0, :, :, :32]
    nblk, ids = interleaved_ids(-(-c['smax'] // T))
    ids[1][0], ids[1][1] = ids[0][0], ids[0][1]
    lin = run_linear(c, n, Hkv, Dh, kernel)
    got = run_paged(c, kv, n, Hkv, Dh, T, kernel, ids=ids, nblk=nblk)
    check_against_linear(c, lin, got, T, f'shared prefix {kv} k{kernel}')


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_enqueue_nothing():
    case, kv = (16, 8, 1, 128, 16, 0), 'fp16'
    past, n, Hkv, Dh, T, prof = case
    c = make_case(past, n, Hkv, Dh, prof, kv)
    M = -(-c['smax'] // T)
    for what, kw, why in (('T = 48', dict(tpb=48), 'power of two'),
                          ('max_blocks_per_seq * T < max_seq_len', dict(max_blocks=M - 1), 'max_blocks_per_seq'),
                          ('max_end > max_seq_len', dict(ragged=([n] * B, c['smax'] + 1)), 'max_end')):
        got = run_paged(c, kv, n, Hkv, Dh, T, APPEND_ATTN_WAVE, **kw)
        assert got['err'] and why in got['err'], (what, got['err'])
        same_bits(got['pool'], got['init'], what)
        assert (got['out'].view(np.uint16) == GUARD).all(), what
        assert np.array_equal(got['qkv'][:B * n].view(np.uint16).ravel(), c['qkv'].view(np.uint16).ravel()), what
    # a table without a pool
    t = device_inputs(c, n, Hkv, Dh)
    table = torch.zeros((B, 2, M), dtype=torch.int64, device='cuda')
    with pytest.raises(RuntimeError, match='pool'):
        attention_append_paged(t['qkv'], None, table, t['out'], t['seq'], t['lens'], tokens_per_block=T, max_seq_len=c['smax'],
                               **common_args(c, t, Hkv, Dh, APPEND_ATTN_WAVE, None, None))
    torch.cuda.synchronize()
    assert (t['out_full'].cpu().numpy().view(np.uint16) == GUARD).all()
