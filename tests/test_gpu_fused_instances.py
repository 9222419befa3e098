"""Every instance of the one-launch decode attention (qkv_attn_fused_kernel<NIT, INT8KV, WK>: NIT 1 / 2 / 3 / 4 / 6 / 8 x int8 / fp16
cache x SmoothQuant / weight-only int8 / int4 / fp16 weights) and the edges of its cache buckets against the ORACLE, one decoder
layer at LLaMA-7B dimensions, batch 1 - the case table is tests/fused_cases.py (checked against the dispatch without a GPU by
tests/test_fused_instance_table.py).  The comparison is test_gpu_fused_envelope.run_cases: the same cache bytes on both sides, the
int8 operands in LSBs (with the bias bound on the signed differences), the context, the appended cache bytes, every other slot of
the capacity unchanged, the logits.

Per case the session's decode form is asserted as the table states it: which instances are resident on an MI355X with and
without the O-projection stage's dynamic LDS is a measured fact of the table, not a silent fall-back."""
import numpy as np
import pytest

import fused_cases as FC
from oracle import quant_oracle as QO
from test_gpu_fused_envelope import D, H, I, V, run_cases
from test_gpu_session import synth_model

pytestmark = pytest.mark.gpu

GROUPS = {}
for _c in FC.ONE_LAUNCH:
    if _c not in FC.REFERENCE_DEQUANT_MISSES:
        GROUPS.setdefault((_c[0], _c[1]), []).append(_c)


def shapes(cases):
    return [(S, length, cap, steps, form) for _, _, S, length, cap, steps, form in cases]


@pytest.mark.parametrize('mode,int8_kv', list(GROUPS), ids=[f'{m}-kv{8 if k else 16}' for m, k in GROUPS])
def test_every_instance_and_bucket_edge_vs_oracle(mode, int8_kv):
    qmode, fuse_o, _ = FC.MODES[mode]
    run_cases(qmode, int8_kv, shapes(GROUPS[(mode, int8_kv)]), one_launch=True, fuse_o=fuse_o)


@pytest.mark.parametrize('int8_kv', [1, 0], ids=['kv8', 'kv16'])
def test_hand_over_to_the_general_launches_vs_oracle(int8_kv):
    """int8 cache 4096 -> 4097 slots, fp16 cache 2048 -> 2049: the one-launch form gives way to the QKV GEMV + mmha_partial_kernel
    + O GEMV (int8 at 4097: the fine split with its own combine launch; fp16 at 2049: the merge inside the attention launch), both
    filled to the last slot, both against the oracle."""
    cases = [c for c in FC.HANDOVER if c[1] == int8_kv]
    assert [c[6] & 1 for c in cases] == [1, 0]
    run_cases('sq_static_pc', int8_kv, shapes(cases), one_launch=True)


def _miss_id(c):
    return FC.case_id(c)


@pytest.mark.parametrize('case', FC.REFERENCE_DEQUANT_MISSES, ids=[_miss_id(c) for c in FC.REFERENCE_DEQUANT_MISSES])
def test_long_context_cases_vs_the_exact_dequantisation_oracle(case):
    """The cases of fused_cases.REFERENCE_DEQUANT_MISSES at every bound of run_cases, the oracle reading the int8 cache as the HIP
    kernels do (without the fp16 rounding of each dequantised element)."""
    mode, kv, S, length, cap, steps, form = case
    qmode, fuse_o, _ = FC.MODES[mode]
    run_cases(qmode, kv, [(S, length, cap, steps, form)], one_launch=True, fuse_o=fuse_o, exact_dequant=True)


_dc_models = {}


def dc_model(mode):
    """The envelope test's synthetic layer with a same-sign DC offset in q: four outlier channels of the embedding hold +6 for every
    token (~11 behind input_layernorm) and every Q row weighs them alike, so q of every head carries an offset of ~5, four times its
    random part (std ~1.3).  The int8-cache score of the one-launch form dots the raw splices 1024 + (k + 128) with q and takes
    1152 x sum(q) off once per row and lane: the bias term is ~60x the signal here."""
    if mode not in _dc_models:
        cfg, w = synth_model(23, L=1, H=H, D=D, I=I, V=V)
        w = dict(w)
        out = [11, 1500, 2222, 3901]
        emb = w['vocab_embedding.weight'].copy()
        emb[:, out] = 6.0
        qkv = w['layers.0.attention.qkv.weight'].copy()
        qkv[:D, out] += np.float16(0.12)
        w['vocab_embedding.weight'], w['layers.0.attention.qkv.weight'] = emb, qkv
        r = np.random.default_rng(31)
        ids = r.integers(3, V, (1, 64)).astype(np.int32)
        _dc_models[mode] = (cfg, QO.quantise_model(cfg, w, mode, 1, calib_ids=ids, calib_lens=np.array([64], np.int32)))
    return _dc_models[mode]


DC_SHAPES = {'sq_static_pc': [(700, 700, 1025, 4)], 'woq8': [(2044, 2044, 2048, 4)], 'woq4': [(2044, 2044, 2048, 4)]}


@pytest.mark.parametrize('mode', list(DC_SHAPES))
def test_int8_cache_score_with_a_dc_offset_in_q(mode):
    """The DC model (int8 cache) through the one-launch form and through the general launches (fuse_qkv_attention = 0: mmha takes
    1152 off every element pair, exact), each against the oracle at the zero-mean cases' bounds (run_cases prints the weight-only
    contexts' error in fp16 ulps), the oracle dequantising the cache as both kernels do.  Between the two forms: the appended cache
    bytes identical, for the weight-only kinds the normalised operand row too, and the contexts within one LSB (SmoothQuant) /
    one fp16 ulp of the largest element: the once-per-row 1152 x sum(q) loses nothing the per-pair subtraction keeps.
    (Against the reference's fp16 rounding of every dequantised element both forms miss alike - see
    test_the_reference_dequantisation_misses.)"""
    built = dc_model(mode)
    assert built[1]['oracle']['int8_kv']
    fused = run_cases(mode, 1, [s + (FC.FORM[mode],) for s in DC_SHAPES[mode]], one_launch=True, built=built, exact_dequant=True)
    general = run_cases(mode, 1, [s + (0,) for s in DC_SHAPES[mode]], one_launch=False, built=built, exact_dequant=True)
    for shape, a, b in zip(DC_SHAPES[mode], fused, general):
        np.testing.assert_array_equal(a['tokens'], b['tokens'])
        np.testing.assert_array_equal(a['cache'], b['cache'])
        for i in range(shape[3]):
            ga, gb = a['taps'][i]['o_in'][0], b['taps'][i]['o_in'][0]
            if mode.startswith('sq'):
                d = int(np.abs(ga.astype(np.int32) - gb.astype(np.int32)).max())
                print(f'[dc {mode} cap={shape[2]}] step {i}: one launch vs general launches, context max {d} LSB')
                assert d <= 1, (mode, shape, i, d)
            else:
                np.testing.assert_array_equal(a['taps'][i]['qkv_in'][0], b['taps'][i]['qkv_in'][0])
                top = max(float(np.abs(gb.astype(np.float32)).max()), 1.0)
                ulp = 2.0 ** (np.floor(np.log2(top)) - 10)
                d = float(np.abs(ga.astype(np.float32) - gb.astype(np.float32)).max())
                print(f'[dc {mode} cap={shape[2]}] step {i}: one launch vs general launches, context max |d| {d / ulp:.2f} fp16 ulp')
                assert d <= ulp, (mode, shape, i, d / ulp)


MISSES = [('dc', m, None) for m in DC_SHAPES] + [('table', c[0], c) for c in FC.REFERENCE_DEQUANT_MISSES]


@pytest.mark.xfail(strict=True, raises=AssertionError, reason=(
    'the oracle rounds every dequantised int8 cache element to fp16 as the reference does, the HIP decode kernels (one-launch and '
    'general alike) do not: measured against that oracle, DC model: SmoothQuant context 3 LSB (bound 1), int8 weights 0.106 '
    '(13.6 fp16 ulp) and int4 0.114 against 0.025 - 1.8 / 2.5 ulp with exact dequantisation; fused_cases.REFERENCE_DEQUANT_MISSES '
    'as stated there'))
@pytest.mark.parametrize('what,mode,case', MISSES, ids=[f'{w}-{m if c is None else FC.case_id(c)}' for w, m, c in MISSES])
def test_the_reference_dequantisation_misses(what, mode, case):
    """Pinned: these cases miss the bounds against the reference's rounding of the dequantised cache (strict: once they pass, the
    kernels or the oracle changed and the note in fused_cases / the exact-dequantisation tests must be revisited)."""
    if what == 'dc':
        run_cases(mode, 1, [s + (FC.FORM[mode],) for s in DC_SHAPES[mode]], one_launch=True, built=dc_model(mode))
    else:
        _, kv, S, length, cap, steps, form = case
        qmode, fuse_o, _ = FC.MODES[mode]
        run_cases(qmode, kv, [(S, length, cap, steps, form)], one_launch=True, fuse_o=fuse_o)
