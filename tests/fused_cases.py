"""The case table of the one-launch decode attention (kernels/qkv_attn_fused.hip) - importable without a GPU.

The session picks one instance qkv_attn_fused_kernel<NIT, INT8KV, WK> per setup: NIT (cache rows per lane group) from the cache
CAPACITY Smax = max_input_len + max_new_tokens (pick_nit, mirrored by bench._fused_nit: 512 slots per NIT with an int8 cache,
256 with an fp16 cache), WK from the projection weights.  A case is

    (mode, int8_kv, max_input_len, prompt length, capacity, steps, decode_form)

run by tests/test_gpu_fused_instances.py against the oracle: setup(1, max_input_len, capacity - max_input_len), a synthetic
context of `prompt length` real tokens, `steps` generation steps (they write slots max_input_len .. + steps - 1), and the
decode form the session must report (tllm_session_decode_form: bit 0 the one-launch projection + attention, bit 1 its
O-projection stage).  tests/test_fused_instance_table.py checks, without a GPU, that the table names every instance the
dispatch holds."""

# mode -> (quantisation of the synthetic model (test_gpu_fused_envelope.model), session key fuse_o_projection, weight kind of
# the dispatch (qkv_attn_fused.hip WK_*))
MODES = {
    'sq_static_pc': ('sq_static_pc', -1, 'WK_SQ'),
    'sq_dyn_pc': ('sq_dyn_pc', -1, 'WK_SQ'),  # per-token SmoothQuant: no O-projection stage (its quantiser is static)
    'woq8': ('woq8', -1, 'WK_WOQ8'),
    'woq4': ('woq4', -1, 'WK_WOQ4'),  # the int4 O-projection stage is opt-in ...
    'woq4+o': ('woq4', 1, 'WK_WOQ4'),  # ... fuse_o_projection = 1
    'fp16': ('fp16', -1, 'WK_FP16'),  # no O-projection stage (a row worker's share of fp16 rows does not fit its LDS)
}

NITS = (1, 2, 3, 4, 6, 8)
STEPS = 4
# the O-projection stage as the session serves it by default (session_setup.cpp decide_decode_form: o_fused), measured resident on an MI355X for every
# instance below (96 KB of dynamic LDS next to the kernel's own; 256 workgroups, one per CU)
FORM = {'sq_static_pc': 3, 'sq_dyn_pc': 1, 'woq8': 3, 'woq4': 1, 'woq4+o': 3, 'fp16': 1}


def slots_per_nit(int8_kv):
    """cache slots one NIT step covers: 8 members x 8 waves x (8 | 4) lane groups"""
    return 512 if int8_kv else 256


def member_span(nit, int8_kv):
    """cache slots of one member (workgroup) of a head: t0 = mem * NGRP * NIT"""
    return slots_per_nit(int8_kv) // 8 * nit


def bucket(nit, int8_kv):
    """(lowest, highest) capacity the instance of `nit` serves"""
    prev = {1: 0, 2: 1, 3: 2, 4: 3, 6: 4, 8: 6}[nit]
    return prev * slots_per_nit(int8_kv) + 1, nit * slots_per_nit(int8_kv)


def _last(cap, steps=STEPS):
    """a prompt that fills the cache: the last step writes slot cap - 1"""
    return cap - steps, cap - steps, cap


def _straddle(nit, int8_kv, m, cap):
    """the `steps` generated tokens cross the boundary of members m - 1 and m (slots b - 2 .. b + 1)"""
    b = m * member_span(nit, int8_kv)
    return b - 2, b - 2, cap


def _case(mode, kv, shape, form=None, steps=STEPS):
    S, length, cap = shape
    return (mode, kv, S, length, cap, steps, FORM[mode] if form is None else form)


# ---- SmoothQuant static per-channel + int8 KV (the headline configuration): both edges of every bucket, the last slot, short
# prompts in large capacities (members 1 .. 7 of every head hold no valid slot), member boundaries, a padded prompt
HEADLINE = [_case('sq_static_pc', 1, s) for s in [
    (3, 3, 7),  # the smallest capacity: bucket 1's lower edge, last slot
    _last(512),
    _straddle(1, 1, 1, 300),
    (40, 40, 513),  # 512 + 1: most tail loads clamp to Smax - 1
    _last(1024),
    (700, 700, 1025),
    _last(1536),
    (40, 40, 1537),
    _straddle(4, 1, 5, 1800),
    _last(2048),
    (64, 64, 2049),
    _last(3072),
    _straddle(6, 1, 6, 2600),
    (3000, 2950, 3073),  # padded: slots 2950 .. 2999 masked
    (24, 24, 4000),
]]  # (the upper edge, _last(4096), is the first case of HANDOVER)

# ---- every other instance, one case each, the edges spread over them (int8 KV, then fp16 KV)
OTHERS_KV8 = {
    'sq_dyn_pc': [(49, 40, 300), _last(1024), (700, 700, 1025), (40, 40, 2048), (2300, 2300, 2600), (24, 24, 4000), _last(4096)],
    'woq8': [(3, 3, 7), (40, 40, 513), _last(1536), _straddle(4, 1, 3, 2048), (2300, 2300, 3072), (32, 32, 4096)],
    'woq4': [_last(512), (49, 40, 1000), (1200, 1200, 1300), _last(1536), _last(2048), (60, 60, 2049), (4000, 4000, 4096)],
    'woq4+o': [(49, 40, 300), (900, 900, 1024), _last(1536), (40, 40, 1537), _last(3072), (3582, 3582, 4000)],
    'fp16': [(3, 3, 7), _last(1024), (1100, 1100, 1500), (40, 40, 2048), _straddle(6, 1, 5, 3000), _last(4096)],
}
OTHERS_KV16 = {
    'sq_static_pc': [(3, 3, 7), _last(512), (300, 300, 513), (40, 40, 1024), _last(1536)],  # + HANDOVER's _last(2048)
    'sq_dyn_pc': [(49, 40, 256), (300, 300, 400), _last(768), (40, 40, 900), (1021, 1021, 1025), (2000, 2000, 2048)],
    'woq8': [_last(256), (49, 40, 512), (600, 600, 700), _last(1024), (40, 40, 1536), (1600, 1600, 1800)],
    'woq4': [(3, 3, 7), (40, 40, 500), _last(768), (800, 800, 1000), (1400, 1400, 1500), (16, 16, 2048)],
    'woq4+o': [_last(256), (400, 400, 512), (520, 520, 600), (40, 40, 1024), (1021, 1021, 1025), _last(2048)],
    'fp16': [(49, 40, 200), _last(512), (513 - 4, 513 - 4, 513), _straddle(4, 0, 3, 1024), (1200, 1200, 1500), (1700, 1650, 2048)],
}

ONE_LAUNCH = HEADLINE + [_case(m, 1, s) for m, v in OTHERS_KV8.items() for s in v] \
    + [_case(m, 0, s) for m, v in OTHERS_KV16.items() for s in v]

# ---- cases the HIP kernels hold only against the oracle's exact dequantisation of the int8 cache.  The reference rounds every
# dequantised cache element to fp16 (llama_oracle.kv_load), the HIP decode kernels - the one-launch form AND the general launches,
# measured alike on an MI355X - apply the scale once to the sums; at long contexts that rounding moves the context by a few fp16
# ulps, enough for the bounds below.  Measured against the fp16-rounding oracle (one-launch / general launches):
#   per-token SmoothQuant, 4092 in 4096: mlp_in signed sum -131 / -132, bound 119 / 120 (exact dequantisation: -36 / -37, bound 90)
#   int4, 1200 in 1300: context 0.0156 (4 fp16 ulp) against 0.0145 (exact dequantisation: 0.0039, 1 ulp)
REFERENCE_DEQUANT_MISSES = [_case('sq_dyn_pc', 1, _last(4096)), _case('woq4', 1, (1200, 1200, 1300))]

# ---- the hand-over to the general launches (QKV GEMV + mmha_partial_kernel + O GEMV): the largest capacity the one-launch form
# serves and one more slot, both filled to the last slot (one session per cache type).  At 4097 int8 slots the attention takes
# the fine split with its own combine launch; at 2049 fp16 slots the merge stays inside the attention launch
HANDOVER = [_case('sq_static_pc', 1, _last(4096)), _case('sq_static_pc', 1, _last(4097), form=0),
            _case('sq_static_pc', 0, _last(2048)), _case('sq_static_pc', 0, _last(2049), form=0)]

CASES = ONE_LAUNCH + HANDOVER


def case_id(c):
    mode, kv, S, length, cap, steps, form = c
    return f'{mode}-kv{8 if kv else 16}-S{S}-len{length}-cap{cap}'
