"""The fp8 (OCP E4M3) KV cache rule of tensorrt_llm/runtime/kv_fp8_ref.py against torch's CPU float8_e4m3fn cast - an
independent implementation of the same encoding - exhaustively, and the restated decode attention against the oracle's.
Host-only."""
import numpy as np
import pytest
import torch

from oracle import llama_oracle as O
from tensorrt_llm.runtime import kv_fp8_ref as R

ALL_FP16 = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
FINITE_FP16 = ALL_FP16[np.isfinite(ALL_FP16)]
FINITE_CODES = np.array([c for c in range(256) if (c & 0x7f) != 0x7f], dtype=np.uint8)


def test_the_module_needs_no_torch():
    import subprocess
    import sys
    code = ('import sys; sys.path[:0] = %r; import tensorrt_llm.runtime.kv_fp8_ref as R; '
            'assert "torch" not in sys.modules; assert R.kv_store_fp8([1.0], 1.0)[0] == 0x38' % (sys.path, ))
    subprocess.run([sys.executable, '-c', code], check=True)


@pytest.mark.parametrize('scale', [1.0, 20.0, 1.0 / 0.37])
def test_store_equals_torch_on_every_finite_fp16_value(scale):
    """All 63 488 finite fp16 values: ties between adjacent codes, the subnormals (2^-9 the smallest, 2^-10 -> 0), +-0 and
    saturation.  torch's CPU cast rounds to nearest even and gives NaN above 464, hence the clip - which is the rule's own."""
    assert FINITE_FP16.size == 63488
    got = R.kv_store_fp8(FINITE_FP16, scale)
    prod = np.clip(FINITE_FP16.astype(np.float32) * np.float32(scale), -448.0, 448.0).astype(np.float32)
    ref = torch.from_numpy(prod).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    np.testing.assert_array_equal(got, ref)
    assert not np.any((got & 0x7f) == 0x7f), 'a NaN code was written'


def test_store_edge_cases_by_hand():
    s = R.kv_store_fp8
    assert s(np.float16(0.0), 1.0) == 0x00 and s(np.float16(-0.0), 1.0) == 0x80  # the sign of zero is kept
    assert s(2.0 ** -9, 1.0) == 0x01 and s(-2.0 ** -9, 1.0) == 0x81               # smallest subnormal
    assert s(2.0 ** -10, 1.0) == 0x00 and s(-2.0 ** -10, 1.0) == 0x80             # a tie, to even = 0
    assert s(3 * 2.0 ** -10, 1.0) == 0x02                                         # tie between 1 and 2 subnormal steps -> even
    assert s(448.0, 1.0) == 0x7e and s(65504.0, 1.0) == 0x7e and s(-65504.0, 1.0) == 0xfe
    assert s(1.0625, 1.0) == 0x38 and s(1.1875, 1.0) == 0x3a                      # ties between 1.0 / 1.125 and 1.125 / 1.25
    assert s(24.0, 20.0) == 0x7e                                                   # 480 clamps to 448


def test_load_equals_torch_on_every_finite_code():
    assert FINITE_CODES.size == 254
    ref = torch.from_numpy(FINITE_CODES).view(torch.float8_e4m3fn).to(torch.float32).numpy()
    np.testing.assert_array_equal(R.kv_load_fp8(FINITE_CODES, 1.0, exact=True), ref)
    np.testing.assert_array_equal(R.kv_load_fp8(FINITE_CODES, 1.0), ref)  # every E4M3 value is an fp16 value
    for scale in (0.05, 0.37):
        prod = ref * np.float32(scale)
        np.testing.assert_array_equal(R.kv_load_fp8(FINITE_CODES, scale, exact=True), prod)
        # exact=False rounds the product to fp16 (the reference's per-element form)
        np.testing.assert_array_equal(R.kv_load_fp8(FINITE_CODES, scale), prod.astype(np.float16).astype(np.float32))
    # store(load(c)) == c for every finite code but -0/+0 aliasing nothing: a fixed point
    np.testing.assert_array_equal(R.kv_store_fp8(ref, 1.0), FINITE_CODES)


@pytest.mark.parametrize('H,Dh,L', [(2, 32, 1), (2, 64, 17), (4, 128, 40)])
def test_decode_with_scale_one_on_representable_values_equals_the_fp16_oracle(H, Dh, L):
    r = np.random.default_rng(L)
    B, smax = 2, L + 4
    codes = r.choice(FINITE_CODES[(FINITE_CODES & 0x7f) < 0x48], size=(B, 2, H, smax, Dh)).astype(np.uint8)  # |x| < 4
    codes[:, :, :, L:] = 0
    vals16 = R.kv_load_fp8(codes, 1.0, exact=True).astype(np.float16)
    # the new token's k, v: representable too, and no RoPE, so that the appended row quantises without loss
    qkv = r.standard_normal((B, 3 * H * Dh)).astype(np.float16).astype(np.float32)
    qkv = qkv.reshape(B, 3, H * Dh)
    qkv[:, 1:] = R.kv_load_fp8(R.kv_store_fp8(qkv[:, 1:], 1.0), 1.0)
    qkv = qkv.reshape(B, -1)
    in_len = [L, max(L // 2, 1)]
    masked = np.zeros((B, smax), np.int32)
    masked[1, in_len[1]:L] = 1
    c8, c16 = codes.copy(), vals16.copy()
    got = R.mmha_decode_fp8(qkv, c8, [L, L], in_len, L, L, H, Dh, 0, 1.0, 1.0, masked_tokens=masked)
    ref = O.mmha_decode(qkv, c16, [L, L], in_len, L, L, H, Dh, 0, True, 1.0, masked)
    np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(R.kv_load_fp8(c8, 1.0, exact=True), c16.astype(np.float32))
    # exact / per-element dequantisation agree when the scale is 1
    got2 = R.mmha_decode_fp8(qkv, codes.copy(), [L, L], in_len, L, L, H, Dh, 0, 1.0, 1.0, masked_tokens=masked,
                             exact_kv_dequant=True)
    np.testing.assert_array_equal(got2, ref)


def test_context_attention_writes_the_rule_and_computes_the_fp16_result():
    r = np.random.default_rng(3)
    B, S, H, Dh = 2, 9, 2, 32
    smax = S + 3
    qkv = r.standard_normal((B, S, 3 * H * Dh)).astype(np.float16).astype(np.float32)
    in_len = [S, 5]
    c8 = np.zeros((B, 2, H, smax, Dh), np.uint8)
    c16 = np.zeros((B, 2, H, smax, Dh), np.float16)
    got, q1 = R.context_attention_fp8(qkv, c8, in_len, H, Dh, Dh, 1 / 0.37)
    ref, q2 = O.context_attention(qkv, c16, in_len, H, Dh, Dh)
    np.testing.assert_array_equal(got, ref)  # the prefill never reads the cache
    np.testing.assert_array_equal(q1, q2)
    np.testing.assert_array_equal(c8, R.kv_store_fp8(c16, 1 / 0.37))


def test_a_one_ulp_change_of_k_moves_few_codes():
    """The GPU tests allow the K bytes of a freshly roped row to sit on the adjacent code in at most 2 % of the elements (the
    kernel's RoPE uses fma, the restatement does not: at most one fp16 ulp).  An E4M3 step is 2^7 fp16 ulps wide, so one ulp
    crosses a rounding boundary in about 1 of 128 elements: the restatement alone stays inside the figure."""
    r = np.random.default_rng(11)
    k = r.standard_normal(1 << 16).astype(np.float16)
    up = np.nextafter(k, np.float16(np.inf))
    for s in (1.0, 20.0):
        a, b = R.kv_store_fp8(k, s), R.kv_store_fp8(up, s)
        d = np.abs(a.astype(np.int32) - b.astype(np.int32))
        assert d.max() <= 1 or set(np.unique(a[d > 1]) & 0x7f) <= {0}  # +-0 sit 0x80 apart
        assert np.mean(a == b) > 0.98
