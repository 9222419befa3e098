"""No GPU: the case table of tests/test_gpu_fused_instances.py (tests/fused_cases.py) against the dispatch of the one-launch decode
attention as the source states it (qkv_attn_fused.hip fused_kernel_of / fused_kernel) and against bench._fused_nit, the Python
mirror of pick_nit that names the instance.  An instance added to the dispatch without a case fails here."""
import os
import re

import bench
import fused_cases as FC

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'trtllm-llama_amd', 'csrc', 'kernels',
                   'qkv_attn_fused.hip')


def _body(src, head):
    """the text of the function whose definition starts with `head`, up to its closing brace at column 0"""
    i = src.index(head)
    return src[i:src.index('\n}\n', i)]


def dispatch():
    """(the NIT of every `case N:` of fused_kernel_of, the (int8 KV, weight kind) pairs fused_kernel hands to it)"""
    src = open(SRC).read()
    of = _body(src, 'const void* fused_kernel_of(int nit)')
    nits = {int(n) for n, m in re.findall(r'case (\d+): return reinterpret_cast<const void\*>\(qkv_attn_fused_kernel<(\d+), INT8KV, WK>\)', of)
            if n == m}
    assert len(re.findall(r'case \d+:', of)) == len(nits), 'a case of fused_kernel_of that does not name its own NIT'
    kinds = {(kv == 'true', wk) for kv, wk in re.findall(r'fused_kernel_of<(true|false), (WK_\w+)>', _body(src, 'const void* fused_kernel(int nit'))}
    return nits, kinds


def pick_nit_of_the_source():
    """pick_nit restated from its own text: kMembers, kWavesF, the lane groups per wave of each cache type and the NIT loop"""
    src = open(SRC).read()
    members = int(re.search(r'constexpr int kMembers = (\d+);', src).group(1))
    waves = int(re.search(r'constexpr int kWavesF = (\d+);', src).group(1))
    body = _body(src, 'int pick_nit(int max_seq_len, bool int8_kv)')
    rpw8, rpw16 = map(int, re.search(r'const int ngrp = kWavesF \* \(int8_kv \? (\d+) : (\d+)\);', body).groups())
    assert 'const int need = (max_seq_len + kMembers * ngrp - 1) / (kMembers * ngrp);' in body
    loop = [int(n) for n in re.search(r'for \(int n : \{([\d, ]+)\}\)', body).group(1).split(',')]

    def pick(smax, int8_kv):
        ngrp = waves * (rpw8 if int8_kv else rpw16)
        need = (smax + members * ngrp - 1) // (members * ngrp)
        return next((n for n in loop if need <= n), 0)
    return pick, members, waves, rpw8, rpw16


def test_the_python_mirror_is_pick_nit():
    """bench._fused_nit and the table's bucket arithmetic against pick_nit's own constants: a change of kMembers, kWavesF, the rows
    per wave or the NIT set moves the cases to other instances, and fails here rather than silently"""
    pick, members, waves, rpw8, rpw16 = pick_nit_of_the_source()
    src = open(SRC).read()
    assert 'constexpr int RPW = 64 / LPR;' in src and 'constexpr int TCHUNK = NGRP * NIT;' in src
    for kv, rpw in ((1, rpw8), (0, rpw16)):
        assert FC.slots_per_nit(kv) == members * waves * rpw
        for nit in FC.NITS:
            assert FC.member_span(nit, kv) == waves * rpw * nit  # TCHUNK = NGRP * NIT
        for c in range(1, 8 * FC.slots_per_nit(kv) + 600):
            assert bench._fused_nit(c, kv) == pick(c, kv), (c, kv)


def test_the_dispatch_is_what_the_table_assumes():
    nits, kinds = dispatch()
    assert nits == set(FC.NITS)
    assert kinds == {(kv, wk) for kv in (False, True) for wk in ('WK_SQ', 'WK_WOQ8', 'WK_WOQ4', 'WK_FP16')}
    assert {wk for _, _, wk in FC.MODES.values()} == {wk for _, wk in kinds}


def test_the_python_mirror_picks_exactly_the_dispatched_buckets():
    """bench._fused_nit over every capacity up to past the largest bucket: the same set of NITs, a new one exactly at 512 n (int8
    cache) / 256 n (fp16 cache) + 1, 0 (the general launches) beyond 8 x that."""
    nits, _ = dispatch()
    for kv in (1, 0):
        per = FC.slots_per_nit(kv)
        top = max(nits) * per
        got = [bench._fused_nit(c, kv) for c in range(1, top + per + 1)]
        assert set(got) - {0} == nits
        switches = {c for c in range(1, top + per) if got[c - 1] != got[c]}  # capacity c serves another instance than c + 1
        assert switches == {n * per for n in nits}, sorted(switches)
        for n in nits:
            lo, hi = FC.bucket(n, kv)
            assert bench._fused_nit(lo, kv) == bench._fused_nit(hi, kv) == n
        assert bench._fused_nit(top + 1, kv) == 0


def test_every_instance_has_a_one_launch_case():
    """Every (NIT, cache, weight kind) instance of the dispatch - and per-token SmoothQuant and the opt-in int4 O-projection stage,
    which run the same instances with other operands - has at least one case that takes the one-launch form."""
    nits, kinds = dispatch()
    have = {}
    for mode, kv, S, length, cap, steps, form in FC.CASES:
        assert 1 <= length <= S and cap >= S + steps and steps >= 1, (mode, S, length, cap, steps)
        nit = bench._fused_nit(cap, kv)
        assert (form & 1) == (nit != 0), ('the one-launch form is served up to 4096 / 2048 slots', mode, kv, cap, form)
        if form & 1:
            have.setdefault((mode, bool(kv)), set()).add(nit)
    missing = [(nit, kv, wk) for kv, wk in sorted(kinds) for nit in sorted(nits)
               if not any(nit in have.get((m, kv), ()) for m, (_, _, w) in FC.MODES.items() if w == wk)]
    assert not missing, f'instances without a one-launch case: {missing}'
    for mode in FC.MODES:
        for kv in (False, True):
            assert have.get((mode, kv), set()) == nits, (mode, kv, sorted(nits - have.get((mode, kv), set())))


def test_the_headline_configuration_has_both_edges_of_every_bucket():
    """SmoothQuant static + int8 KV: capacity 512 n and 512 n_prev + 1 for every bucket (bucket 1: the smallest capacity a case
    can have), a step that writes the last slot, short prompts in buckets 4 / 6 / 8, a member boundary inside the steps, a padded
    prompt in a large bucket, and the hand-over 4096 -> 4097."""
    nits, _ = dispatch()
    hl = [c for c in FC.CASES if c[0] == 'sq_static_pc' and c[1] == 1]
    caps = {c[4] for c in hl if c[6] & 1}
    for n in nits:
        lo, hi = FC.bucket(n, 1)
        assert hi in caps, ('upper edge', n, hi)
        assert (lo in caps) if n > 1 else min(caps) <= 8, ('lower edge', n, lo)
    assert any(c[6] & 1 and c[2] + c[5] == c[4] for c in hl), 'no step writes the last slot'
    short = {bench._fused_nit(c[4], 1) for c in hl if c[3] <= 64}
    assert {4, 6, 8} <= short, short
    assert any(c[2] > c[3] and bench._fused_nit(c[4], 1) >= 6 for c in hl), 'no padded prompt in a large bucket'
    span = lambda c: FC.member_span(bench._fused_nit(c[4], 1), 1)
    # the steps write slots S .. S + steps - 1: the first and the last of them in different members, none of them the last slot
    assert any(c[6] & 1 and c[2] // span(c) != (c[2] + c[5] - 1) // span(c) and c[2] + c[5] < c[4] for c in hl), \
        'no case whose steps cross a member boundary'
    assert {(c[4], c[6] & 1) for c in FC.HANDOVER if c[1] == 1} == {(4096, 1), (4097, 0)}
    assert {(c[4], c[6] & 1) for c in FC.HANDOVER if c[1] == 0} == {(2048, 1), (2049, 0)}
