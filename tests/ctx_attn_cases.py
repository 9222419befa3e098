"""The case table of the context (prompt) attention (kernels/context_attn.hip) - importable without a GPU.

launch_context_attention runs one of four attention kernels, each built per head size: ten instances

    WAVE   at head size 32, 64, 128, 256     context_attn_kernel<DH>                      one wave per query, 4 queries a workgroup
    NARROW at head size 64, 128              context_attn_mfma_ks_kernel<DH, 2>           64 queries a workgroup, 2 operand stages
    WIDE   at head size 64, 128              context_attn_mfma_ks_kernel<DH, 4>           128 queries a workgroup, 2 stages
    PAIRED at head size 64, 128              context_attn_mfma_ks_kernel<DH, 4, true, 3>  two 64-query blocks a workgroup, 3 stages

chosen by context_attention_plan (kernels.h) from the shape and the CU count of the device, or forced through
tllm_attention_params_t::context_kernel.  plan() below is a Python restatement of that rule; tests/test_ctx_attn_instance_table.py
holds it against tllm_attention_context_layout and checks, without a GPU, that every instance meets every option;
tests/test_gpu_ctx_attn_instances.py runs every case against oracle/attention_oracle.py.  Every case forces its kernel (the cases
named 'natural' leave the choice to the rule, where the rule does not depend on the device), so the shapes stay small: 1 - 4 heads,
3 sequences."""
from collections import namedtuple

WAVE, NARROW, WIDE, PAIRED = 1, 2, 3, 4  # TLLM_CTX_ATTN_* (include/tllm_runtime_api.h)
KIND_NAME = {0: 'rule', WAVE: 'wave', NARROW: 'narrow', WIDE: 'wide', PAIRED: 'paired'}
MFMA_KINDS = (NARROW, WIDE, PAIRED)
INSTANCES = [(WAVE, dh) for dh in (32, 64, 128, 256)] + [(k, dh) for k in MFMA_KINDS for dh in (64, 128)]


def plan(head_size, seq, batch, num_heads, has_workspace, scale_positive, cus, forced=0):
    """context_attention_plan: (kind, queries per workgroup, operand stages, workgroups), or None where the launch is refused"""
    if seq < 1 or batch < 1 or num_heads < 1 or head_size not in (32, 64, 128, 256) or forced not in (0, WAVE, NARROW, WIDE, PAIRED):
        return None
    serves = head_size in (64, 128) and has_workspace and seq >= 64 and scale_positive
    kind = forced
    if kind in MFMA_KINDS and not serves:
        return None
    if kind == 0:
        kind = WAVE
        if serves:
            wg128 = (seq + 127) // 128 * num_heads * batch
            kind = PAIRED if (wg128 <= cus and 4 * wg128 >= cus) else (NARROW if wg128 < 256 else WIDE)
    if kind == WAVE:
        return (WAVE, 4, 0, (seq + 3) // 4 * num_heads * batch)
    qb = 64 if kind == NARROW else 128
    return (kind, qb, 3 if kind == PAIRED else 2, num_heads * ((seq + qb - 1) // qb) * batch)


_FIELDS = dict(name='', kind=0, dh=0, H=1, Hkv=1, lens=(),
               layout='padded',  # 'packed': qkv / out hold the real tokens only, cu_seqlens set
               cache='linear',   # 'paged16' / 'paged64': tokens_per_block 16 / 64, one trailing block no sequence maps
               stride=1,         # cache_seq_stride: prompt b fills sequence b * stride, the siblings keep their bytes
               kv='fp16',        # cache element: fp16 / int8 / fp8
               q8=0,             # out_q8 / out_q_scale set
               rope='neox',      # 'neox' (full), 'gptj' (rotary_dim = Dh / 2, q_scaling = 2), 'none'
               forced=1,         # 0: context_kernel left to the rule ('natural')
               workspace=1,      # 0: workspace NULL
               q_scaling=0.0,    # non-zero: instead of the rope profile's
               witness=0,        # the key-counting runs of section c (q = 0, V = the witness codes), at every length of `lengths`
               lengths=(),
               refused='')       # the launch must fail with this word in the error, nothing written
Case = namedtuple('Case', list(_FIELDS), defaults=list(_FIELDS.values()))

MFMA_LENGTHS = (64, 65, 127, 128, 129, 191, 192, 193, 257, 449, 512)
WAVE_LENGTHS = (1, 3, 4, 5, 17, 63, 64, 65, 200)
MFMA_DEEP, WAVE_DEEP = 2048, 1024


def padded_lens(S):
    return (S, max(S // 2, 1), 1)


def packed_edge_lens(S):
    """ends on a 64-key block / one past it; inside the first block / one short of two; two whole blocks / one short of one -
    clipped to S, the longest sequence of the batch"""
    return [tuple(min(x, S) for x in t) for t in ((S, 64, 65), (S, 1, 127), (S, 128, 63))]


# option profiles: (kv, K/V heads: 'H' | 'H/2' | '1', layout, cache, stride, q8, rope).  Every instance runs every profile (each at
# another length), so every instance meets every value of every option and the pairs {packed, paged}, {packed, out_q8},
# {paged, stride 3}, {GQA, paged}, {GQA, packed}.
PROFILES = [
    ('fp16', 'H', 'padded', 'linear', 1, 0, 'neox'),
    ('int8', 'H/2', 'packed', 'paged16', 1, 1, 'gptj'),
    ('fp8', '1', 'padded', 'paged64', 3, 0, 'none'),
    ('fp16', 'H/2', 'packed', 'linear', 3, 0, 'neox'),
    ('int8', 'H', 'padded', 'linear', 1, 1, 'neox'),
    ('fp8', '1', 'packed', 'paged64', 3, 1, 'gptj'),
    ('fp16', 'H', 'padded', 'paged16', 3, 1, 'none'),
    ('int8', '1', 'packed', 'linear', 1, 0, 'none'),
    ('fp8', 'H/2', 'padded', 'linear', 1, 0, 'gptj'),
    ('fp16', '1', 'packed', 'paged16', 1, 0, 'gptj'),
    ('int8', 'H/2', 'padded', 'paged64', 1, 1, 'neox'),
]
PACKED_PROFILES = [p for p in PROFILES if p[2] == 'packed']


def _hkv(H, sel):
    return {'H': H, 'H/2': max(H // 2, 1), '1': 1}[sel]


def _case(name, kind, dh, H, lens, prof, **kw):
    kv, sel, layout, cache, stride, q8, rope = prof
    if kind == WAVE and layout == 'packed':
        q8 = 0  # refused on this path (REFUSED holds the refusal)
    return Case(name=name, kind=kind, dh=dh, H=H, Hkv=_hkv(H, sel), lens=tuple(lens), layout=layout, cache=cache, stride=stride,
                kv=kv, q8=q8, rope=rope, **kw)


def _grid():
    cases = []
    for n, (kind, dh) in enumerate(INSTANCES):
        lengths = WAVE_LENGTHS if kind == WAVE else MFMA_LENGTHS
        for i, S in enumerate(lengths):
            prof = PROFILES[(i + 3 * n) % len(PROFILES)]
            H = 4 if prof[1] == 'H/2' else (4, 2, 3)[(i + n) % 3]  # (H/2 of an odd count is no divisor)
            cases.append(_case('edge', kind, dh, H, padded_lens(S), prof))
        # packed batches whose shorter sequences end on, one past and inside a 64-key block
        deep = (200, ) if kind == WAVE else (129, 192, 257, 449, 512)
        for li in range(3):
            for j in range(1 if kind == WAVE else 3):
                S = deep[(li + j * 2 + n) % len(deep)]
                prof = PACKED_PROFILES[(li + j + n) % len(PACKED_PROFILES)]
                H = 4 if prof[1] == 'H/2' else (2, 3, 1)[(li + j) % 3]
                cases.append(_case('packed-edge', kind, dh, H, packed_edge_lens(S)[li], prof))
    return cases


GRID = _grid()

# the rule itself where it does not depend on the device: no workspace, or a non-positive score scale, is the wave-per-query
# kernel at any length; so are head sizes 32 / 256
NATURAL = [
    Case('natural', WAVE, 64, 2, 1, (64, 32, 1), forced=0, workspace=0),
    Case('natural', WAVE, 128, 2, 2, (130, 65, 1), forced=0, workspace=0, kv='int8', q8=1),
    Case('natural', WAVE, 128, 4, 2, (128, 64, 1), forced=0, q_scaling=-1.0, rope='gptj'),
    Case('natural', WAVE, 64, 3, 3, (65, 32, 1), forced=0, q_scaling=-0.5, layout='packed', cache='paged16'),
    Case('natural', WAVE, 256, 2, 1, (130, 65, 1), forced=0, kv='fp8', stride=3),
    Case('natural', WAVE, 32, 2, 2, (129, 64, 1), forced=0),
]


def _witness():
    cases = []
    for n, (kind, dh) in enumerate(INSTANCES):
        lengths = (WAVE_LENGTHS + (WAVE_DEEP, )) if kind == WAVE else (MFMA_LENGTHS + (MFMA_DEEP, ))
        rope = ('neox', 'gptj', 'none')[n % 3]
        cases.append(Case('witness', kind, dh, 1, 1, (), rope=rope, witness=1, lengths=lengths))
        for li in range(3):
            cases.append(Case(f'witness-edge{li}', kind, dh, 1, 1, (), layout='packed', rope=rope, witness=2 + li, lengths=lengths))
    return cases


WITNESS = _witness()  # witness = 1: padded_lens(S); 2 + li: packed_edge_lens(S)[li]

# what the launch refuses, with nothing enqueued: a forced MFMA kind without a workspace, at head sizes 32 / 256, below 64 tokens,
# with a non-positive score scale; an unknown kind; the wave-per-query kernel with packed inputs and the int8 output
REFUSED = [
    Case('refused', NARROW, 64, 2, 2, (128, 64, 1), workspace=0, refused='workspace'),
    Case('refused', PAIRED, 128, 2, 1, (65, 32, 1), workspace=0, refused='workspace'),
    Case('refused', WIDE, 32, 2, 2, (128, 64, 1), refused='head size'),
    Case('refused', PAIRED, 256, 1, 1, (128, 64, 1), refused='head size'),
    Case('refused', NARROW, 128, 2, 2, (63, 31, 1), refused='seq'),
    Case('refused', WIDE, 64, 2, 2, (17, 8, 1), refused='seq'),
    Case('refused', PAIRED, 64, 2, 2, (128, 64, 1), q_scaling=-1.0, refused='score scale'),
    Case('refused', 5, 64, 2, 2, (128, 64, 1), refused='unknown'),
    Case('refused', -1, 128, 2, 2, (128, 64, 1), refused='unknown'),
    Case('refused', WAVE, 64, 2, 2, (65, 32, 1), layout='packed', q8=1, refused='padded'),
    Case('refused', WAVE, 32, 2, 1, (17, 8, 1), layout='packed', q8=1, forced=0, refused='padded'),
]

CASES = GRID + NATURAL + WITNESS + REFUSED


def q_scaling(c):
    return c.q_scaling if c.q_scaling else (2.0 if c.rope == 'gptj' else 1.0)


def rotary(c):
    """(rotary_dim, neox)"""
    return {'neox': (c.dh, 1), 'gptj': (c.dh // 2, 0), 'none': (0, 1)}[c.rope]


def seq(c):
    return max(c.lens)


def expected_plan(c, cus=256):
    return plan(c.dh, seq(c), len(c.lens), c.H, bool(c.workspace), q_scaling(c) > 0, cus, c.kind if c.forced else 0)


def witness_lens(c, S):
    return padded_lens(S) if c.witness == 1 else packed_edge_lens(S)[c.witness - 2]


def case_id(c):
    s = f'{c.name}-{KIND_NAME.get(c.kind, c.kind)}-dh{c.dh}-H{c.H}k{c.Hkv}'
    if c.lens:
        s += '-L' + '.'.join(str(x) for x in c.lens)
    s += f'-{c.layout}-{c.cache}-{c.kv}-{c.rope}' + ('-stride3' if c.stride == 3 else '') + ('-q8' if c.q8 else '')
    s += ('' if c.forced else '-unforced') + ('' if c.workspace else '-nows') + (f'-qs{c.q_scaling}' if c.q_scaling else '')
    return s
