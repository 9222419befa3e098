"""No GPU: the case table of tests/test_gpu_ctx_attn_instances.py (tests/ctx_attn_cases.py) against the launch rule of the context
attention - ctx_attn_cases.plan(), the Python restatement, against tllm_attention_context_layout at a CU count given by the caller
(no device is asked), at the seams of the rule and for every case of the table; then every instance must meet every option value
and the option pairs that share code (packed x paged, packed x int8 output, paged x beam stride, GQA x paged, GQA x packed).  An
option added to the kernels without a case fails here once it is added to OPTIONS below."""
import ctypes
import itertools
import os
import re

import pytest

import ctx_attn_cases as CC
from tensorrt_llm.plugin import capi

KDIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'trtllm-llama_amd', 'csrc', 'kernels')


def layout(lib, head_size, seq, batch, num_heads, has_workspace, q_scaling, cus, forced=0):
    p = capi.AttentionParams(batch=batch, seq=seq, num_heads=num_heads, head_size=head_size, q_scaling=q_scaling,
                             context_kernel=forced, workspace=256 if has_workspace else None)  # (the pointer is never followed)
    a = [ctypes.c_int32(-1) for _ in range(4)]
    rc = lib.tllm_attention_context_layout(ctypes.byref(p), cus, *[ctypes.byref(x) for x in a])
    return None if rc else tuple(x.value for x in a)


def test_the_kinds_are_the_headers():
    assert (capi.CTX_ATTN_WAVE, capi.CTX_ATTN_MFMA_NARROW, capi.CTX_ATTN_MFMA_WIDE, capi.CTX_ATTN_MFMA_PAIRED) \
        == (CC.WAVE, CC.NARROW, CC.WIDE, CC.PAIRED)
    k = open(os.path.join(KDIR, 'kernels.h')).read()
    for name, v in (('CTX_ATTN_RULE', 0), ('CTX_ATTN_WAVE', 1), ('CTX_ATTN_MFMA_NARROW', 2), ('CTX_ATTN_MFMA_WIDE', 3), ('CTX_ATTN_MFMA_PAIRED', 4)):
        assert re.search(rf'\b{name} = {v}\b', k), name


def test_the_launcher_states_the_rule_once():
    """launch_dh takes everything from the plan: the pairing window, the literal 256 and the 64-token threshold appear in
    context_attention_plan and nowhere else in the file"""
    src = open(os.path.join(KDIR, 'context_attn.hip')).read()
    at = src.index('ContextAttnPlan context_attention_plan(int32_t head_size')
    before, rule = src[:at], src[at:]
    assert 'context_attention_plan(DH, p.seq, p.batch, p.num_heads, p.workspace != nullptr, p.inv_sqrt_dh > 0.f, 0, p.kernel)' in before
    for piece in ('wg128 <= cus && 4 * wg128 >= cus', 'wg128 < 256', 'seq >= 64', 'launch_util::device_cus()'):
        assert piece in rule and piece not in before, piece


@pytest.mark.parametrize('cus', [256, 304, 80])
def test_the_rule_at_its_seams(lib, cus):
    """wg128 = ceil(S / 128) * H * B on both sides of: 64 (a quarter of 256 CUs), cus / 4, cus, 256 - at 256 CUs and two other counts"""
    seen = set()
    for wg in sorted({63, 64, 65, cus // 4 - 1, cus // 4, cus // 4 + 1, cus - 1, cus, cus + 1, 255, 256, 257, 4 * cus, 4 * cus + 1}):
        if wg < 1:
            continue
        for dh, (S, B) in itertools.product((64, 128), ((128, 1), (129, 1), (1024, 1), (64, 1))):
            blocks = (S + 127) // 128
            if wg % blocks:
                continue
            H = wg // blocks
            got = layout(lib, dh, S, B, H, True, 1.0, cus)
            want = CC.plan(dh, S, B, H, True, True, cus)
            assert got == want, (cus, wg, dh, S, H, got, want)
            paired = wg <= cus <= 4 * wg
            assert want[0] == (CC.PAIRED if paired else (CC.NARROW if wg < 256 else CC.WIDE)), (cus, wg)
            seen.add((wg, want[0]))
            # below 64 tokens, without the workspace or with a negative score scale: the wave-per-query kernel
            for args in ((dh, 63, B, H, True, 1.0), (dh, S, B, H, False, 1.0), (dh, S, B, H, True, -1.0)):
                assert layout(lib, *args, cus)[0] == CC.WAVE
    kinds = {k for _, k in seen}
    assert kinds == {CC.NARROW, CC.WIDE, CC.PAIRED}, seen
    if cus == 256:
        assert {(63, CC.NARROW), (64, CC.PAIRED), (256, CC.PAIRED), (257, CC.WIDE), (255, CC.PAIRED)} <= seen
    if cus == 304:
        assert {(75, CC.NARROW), (76, CC.PAIRED), (304, CC.PAIRED), (305, CC.WIDE), (256, CC.PAIRED)} <= seen
    if cus == 80:  # a narrow band between the pairing window and 256 workgroups
        assert {(19, CC.NARROW), (20, CC.PAIRED), (80, CC.PAIRED), (81, CC.NARROW), (255, CC.NARROW), (256, CC.WIDE)} <= seen


def test_the_plan_of_known_launches(lib):
    """the restatement itself, pinned where the numbers are known: the 32-head model on 256 CUs"""
    assert CC.plan(128, 1024, 1, 32, True, True, 256) == (CC.PAIRED, 128, 3, 256)
    assert CC.plan(128, 1025, 1, 32, True, True, 256) == (CC.WIDE, 128, 2, 288)
    assert CC.plan(128, 128, 1, 32, True, True, 256) == (CC.NARROW, 64, 2, 64)
    assert CC.plan(128, 129, 1, 32, True, True, 256) == (CC.PAIRED, 128, 3, 64)
    assert CC.plan(64, 300, 2, 4, True, True, 256) == (CC.NARROW, 64, 2, 40)
    assert CC.plan(64, 300, 2, 4, False, True, 256) == (CC.WAVE, 4, 0, 600)
    assert CC.plan(256, 300, 2, 4, True, True, 256) == (CC.WAVE, 4, 0, 600)
    for args in ((128, 1024, 1, 32), (128, 1025, 1, 32), (64, 300, 2, 4), (256, 300, 2, 4), (32, 7, 3, 1)):
        assert layout(lib, *args, True, 1.0, 256) == CC.plan(*args, True, True, 256)


def test_forced_kinds_and_their_refusals(lib):
    for dh, S, ws, qs, forced in itertools.product((32, 64, 128, 256), (1, 63, 64, 300), (True, False), (1.0, -1.0, 0.0),
                                                   (-1, 1, 2, 3, 4, 5)):
        got = layout(lib, dh, S, 2, 3, ws, qs, 256, forced)
        want = CC.plan(dh, S, 2, 3, ws, qs >= 0, 256, forced)  # (q_scaling 0 means 1)
        assert got == want, (dh, S, ws, qs, forced, got, want)
        serves = dh in (64, 128) and S >= 64 and ws and qs >= 0
        assert (got is not None) == (forced == 1 or (forced in (2, 3, 4) and serves))
        if got is None:
            assert 'refused' in capi.last_error()
        else:
            assert got[0] == forced  # exactly that instance, never a substitute
    assert layout(lib, 24, 64, 1, 1, True, 1.0, 256) is None and layout(lib, 64, 0, 1, 1, True, 1.0, 256) is None


def test_every_case_has_the_plan_the_library_gives(lib):
    ids = [CC.case_id(c) for c in CC.CASES]
    assert len(ids) == len(set(ids)), [i for i in ids if ids.count(i) > 1]
    for c in CC.CASES:
        shapes = [c.lens] if c.lens else [CC.witness_lens(c, S) for S in c.lengths]
        for lens in shapes:
            cc = c._replace(lens=tuple(lens))
            want = CC.expected_plan(cc, 256)
            got = layout(lib, c.dh, CC.seq(cc), len(lens), c.H, bool(c.workspace), CC.q_scaling(c), 256, c.kind if c.forced else 0)
            assert got == want, (CC.case_id(cc), got, want)
            if c.refused and c.refused != 'padded':  # (the packed int8 output is refused by the launch, not by the plan)
                assert want is None, CC.case_id(cc)
            else:
                assert want is not None and want[0] == c.kind, CC.case_id(cc)
            if not c.forced:
                # 'natural' cases must not depend on the device: the same kind at any CU count
                assert {CC.expected_plan(cc, n)[0] for n in (1, 64, 256, 1024)} == {c.kind}
            assert 1 <= c.H <= 4 and len(lens) == 3 and c.H % c.Hkv == 0


OPTIONS = dict(kv=('fp16', 'int8', 'fp8'), hkv=('H', 'H/2', '1'), layout=('padded', 'packed'),
               cache=('linear', 'paged16', 'paged64'), stride=(1, 3), q8=(0, 1), rope=('neox', 'gptj', 'none'))
PAIRS = [(('layout', 'packed'), ('cache', 'paged')), (('layout', 'packed'), ('q8', 1)), (('cache', 'paged'), ('stride', 3)),
         (('hkv', 'gqa'), ('cache', 'paged')), (('hkv', 'gqa'), ('layout', 'packed'))]


def option(c, name):
    if name == 'hkv':
        return 'H' if c.Hkv == c.H and c.H > 1 else ('1' if c.Hkv == 1 and c.H > 1 else ('H/2' if c.H > 1 else None))
    return getattr(c, name)


def has(c, name, value):
    if (name, value) == ('cache', 'paged'):
        return c.cache != 'linear'
    if (name, value) == ('hkv', 'gqa'):
        return c.Hkv < c.H
    return option(c, name) == value


def runs(c):
    return not c.refused and not c.witness


def missing(cases):
    out = []
    groups = [(f'{CC.KIND_NAME[k]}-dh{dh}', [c for c in cases if runs(c) and (c.kind, c.dh) == (k, dh)]) for k, dh in CC.INSTANCES]
    for who, mine in groups:
        for name, values in OPTIONS.items():
            for v in values:
                if not any(option(c, name) == v for c in mine):
                    out.append((who, name, v))
    # the pairs: for every MFMA instance, and for the wave-per-query kernel as a whole
    pair_groups = [g for g in groups if not g[0].startswith('wave')] + [('wave', [c for c in cases if runs(c) and c.kind == CC.WAVE])]
    for who, mine in pair_groups:
        for a, b in PAIRS:
            if who == 'wave' and (a, b) == (('layout', 'packed'), ('q8', 1)):
                if not any(c.kind == CC.WAVE and c.refused == 'padded' and c.layout == 'packed' and c.q8 for c in cases):
                    out.append((who, 'refusal of', a, b))
                continue
            if not any(has(c, *a) and has(c, *b) for c in mine):
                out.append((who, a, b))
    return out


def test_every_instance_meets_every_option_and_pair():
    assert not missing(CC.CASES), missing(CC.CASES)
    # and the check has teeth: without the packed + paged cases of an instance, that pair is reported for it
    cut = [c for c in CC.CASES if not ((c.kind, c.dh) == (CC.PAIRED, 128) and c.layout == 'packed' and c.cache != 'linear')]
    assert ('paired-dh128', ('layout', 'packed'), ('cache', 'paged')) in missing(cut)
    cut = [c for c in CC.CASES if not (c.kind == CC.WAVE and c.kv == 'fp8' and c.dh == 256)]
    assert ('wave-dh256', 'kv', 'fp8') in missing(cut)


def test_the_lengths_and_batches_the_kernels_can_get_wrong():
    edge = [c for c in CC.GRID if c.name == 'edge']
    for kind, dh in CC.INSTANCES:
        mine = [c for c in edge if (c.kind, c.dh) == (kind, dh)]
        want = CC.WAVE_LENGTHS if kind == CC.WAVE else CC.MFMA_LENGTHS
        assert sorted(CC.seq(c) for c in mine) == sorted(want), (kind, dh)
        assert all(c.lens == CC.padded_lens(CC.seq(c)) for c in mine)
        pk = [c for c in CC.GRID if (c.kind, c.dh) == (kind, dh) and c.name == 'packed-edge']
        assert all(c.layout == 'packed' for c in pk)
        tails = {c.lens[1:] for c in pk}
        assert tails == {(64, 65), (1, 127), (128, 63)}, (kind, dh, tails)
        wit = [c for c in CC.WITNESS if (c.kind, c.dh) == (kind, dh)]
        assert sorted(c.witness for c in wit) == [1, 2, 3, 4] and all(c.H == 1 for c in wit)
        deep = CC.WAVE_DEEP if kind == CC.WAVE else CC.MFMA_DEEP
        assert all(set(c.lengths) == set(want) | {deep} for c in wit)
    assert CC.MFMA_LENGTHS == (64, 65, 127, 128, 129, 191, 192, 193, 257, 449, 512) and CC.MFMA_DEEP == 2048
    assert CC.WAVE_LENGTHS == (1, 3, 4, 5, 17, 63, 64, 65, 200) and CC.WAVE_DEEP == 1024
    assert CC.packed_edge_lens(449) == [(449, 64, 65), (449, 1, 127), (449, 128, 63)]
    # every refusal of the launcher has a case
    assert {c.refused for c in CC.REFUSED} == {'workspace', 'head size', 'seq', 'score scale', 'unknown', 'padded'}
    # no workspace and a non-positive scale at 64 tokens and more, head size 256: reached through the rule
    nat = [c for c in CC.NATURAL]
    assert any(not c.workspace and CC.seq(c) >= 64 and c.dh == d for c in nat for d in (64, 128))
    assert any(CC.q_scaling(c) < 0 and CC.seq(c) >= 64 for c in nat) and any(c.dh == 256 for c in nat)
