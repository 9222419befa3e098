"""The fp8 (OCP E4M3) KV cache through the C-ABI, host side only: plugin creation / format negotiation / serialisation, the
session's quant_mode bit 64 and the engine check.  No GPU needed."""
import ctypes
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, 'trtllm-llama_amd', 'examples', 'llama_quant')
sys.path.insert(0, EX)

from tensorrt_llm.plugin import capi  # noqa: E402
from test_engine_check import TINY, edit_network, set_field, verify  # noqa: E402

i32 = lambda v: np.array(v, dtype=np.int32)
i8 = lambda v: np.array(v, dtype=np.int8)
f32 = lambda v: np.array(v, dtype=np.float32)


def attention_fields(**over):
    f = dict(num_heads=i32(32), head_size=i32(128), unidirectional=i32(1), q_scaling=f32(1.0), rotary_embedding_dim=i32(128),
             neox_rotary_style=i8(1), context_fmha_type=i8(0), multi_block_mode=i8(0), multi_query_mode=i8(0),
             int8_kv_cache=i32(0), fp8_kv_cache=i32(1), remove_input_padding=i8(0), mask_type=i32(1), paged_kv_cache=i32(0),
             type_id=i32(capi.HALF), in_flight_batching=i32(0))
    f.update(over)
    return [capi.PluginField(k, v) for k, v in f.items()]


def test_the_plugin_is_created_with_fp8_and_refuses_both_cache_types():
    assert capi.Plugin.create('GPTAttention', attention_fields()) is not None, capi.last_error()
    assert capi.Plugin.create('GPTAttention', attention_fields(int8_kv_cache=i32(1))) is None
    why = capi.last_error()
    assert 'int8_kv_cache' in why and 'fp8_kv_cache' in why, why


def test_format_negotiation_takes_fp8_cache_ports_and_the_two_scales():
    B, S, H, Dh, Smax = 2, 16, 32, 128, 48
    shapes = [[B, S, 3 * H * Dh], [B, 2, H, Smax, Dh], [B], [2], [B, Smax], [B], [S], [B, 1, Smax], [1], [1]]
    outs = [[B, S, H * Dh], shapes[1]]
    types = [capi.HALF, capi.FP8] + [capi.INT32] * 6 + [capi.FLOAT] * 2
    p = capi.Plugin.create('GPTAttention', attention_fields())
    for pos in range(len(shapes) + 2):
        assert p.supports_format(pos, shapes + outs, types + [capi.HALF, capi.FP8], len(shapes)), pos
    for bad in (capi.HALF, capi.INT8):
        t = list(types)
        t[1] = bad
        assert not p.supports_format(1, shapes + outs, t + [capi.HALF, capi.FP8], len(shapes)), bad
        assert not p.supports_format(len(shapes) + 1, shapes + outs, types + [capi.HALF, bad], len(shapes)), bad
    # without the scale inputs the node is not the fp8 node
    assert not p.supports_format(0, shapes[:8] + outs, types[:8] + [capi.HALF, capi.FP8], 8)
    # paged: the block pointers follow the scales, as for int8
    pg = capi.Plugin.create('GPTAttention', attention_fields(paged_kv_cache=i32(1)))
    T, M = 16, 3
    shapes = [[B, S, 3 * H * Dh], [B * M, 2, H, T, Dh], [B], [2], [B, M * T], [B], [S], [B, 1, M * T], [1], [1], [B, 1, 2, 2 * M]]
    types = [capi.HALF, capi.FP8] + [capi.INT32] * 6 + [capi.FLOAT] * 2 + [capi.INT32]
    for pos in range(len(shapes) + 2):
        assert pg.supports_format(pos, shapes + [[B, S, H * Dh], shapes[1]], types + [capi.HALF, capi.FP8], len(shapes)), pos


def test_serialisation_round_trip_carries_the_flag():
    p = capi.Plugin.create('GPTAttention', attention_fields())
    blob = p.serialize()
    q = capi.Plugin.deserialize('GPTAttention', blob)
    assert q is not None and q.serialize() == blob and q.clone().serialize() == blob
    assert blob != capi.Plugin.create('GPTAttention', attention_fields(fp8_kv_cache=i32(0))).serialize()
    B, S, H, Dh, Smax = 1, 4, 32, 128, 8
    shapes = [[B, S, 3 * H * Dh], [B, 2, H, Smax, Dh], [B], [2], [B, Smax], [B], [S], [B, 1, Smax], [1], [1]]
    types = [capi.HALF, capi.FP8] + [capi.INT32] * 6 + [capi.FLOAT] * 2
    assert q.clone().supports_format(1, shapes + [[B, S, H * Dh], shapes[1]], types + [capi.HALF, capi.FP8], len(shapes))


CFG = 'num_layers=1\nnum_heads=2\nhidden_size=64\ninter_size=24\nvocab_size=128\nquant_mode=%d\n'


def test_session_create_takes_bit_64_and_refuses_it_together_with_bit_32():
    lib = capi.load_library()
    lib.tllm_session_create.restype = ctypes.c_void_p
    lib.tllm_session_create.argtypes = [ctypes.c_char_p]
    lib.tllm_session_destroy.argtypes = [ctypes.c_void_p]
    assert not lib.tllm_session_create((CFG % 96).encode())
    why = capi.last_error()
    assert 'INT8_KV_CACHE' in why and 'FP8_KV_CACHE' in why, why
    h = lib.tllm_session_create((CFG % 64).encode())
    assert h, capi.last_error()
    lib.tllm_session_destroy(h)


_engines = {}


def build(flags):
    key = tuple(flags)
    if key not in _engines:
        import build as B
        d = tempfile.mkdtemp()
        B.run_build(TINY + ['--output_dir', d] + list(flags))
        _engines[key] = [open(os.path.join(d, f), 'rb').read() for f in sorted(os.listdir(d)) if f.endswith('.engine')]
    return _engines[key]


def test_engines_built_with_the_flag_are_verified():
    for flags in (['--fp8_kv_cache'], ['--use_smooth_quant', '--per_channel', '--fp8_kv_cache'],
                  ['--use_weight_only', '--fp8_kv_cache', '--paged_kv_cache']):
        for e in build(flags):
            rc, why = verify(e)
            assert rc == 0, f'{flags}: {why}'


def test_an_engine_whose_node_disagrees_with_the_configuration_is_refused():
    e = build(['--fp8_kv_cache'])[0]
    for which in (0, -1):
        rc, why = verify(edit_network(e, set_field('GPTAttention', 'fp8_kv_cache', 0, which)))
        assert rc != 0 and 'GPTAttention' in why and 'fp8_kv_cache' in why, why
    # ... and the other way round: an fp16-cache configuration with an fp8 node
    rc, why = verify(edit_network(build([])[0], set_field('GPTAttention', 'fp8_kv_cache', 1)))
    assert rc != 0 and 'fp8_kv_cache' in why, why


def test_build_refuses_both_cache_flags():
    import build as B
    import pytest
    with pytest.raises(SystemExit):
        B.parse_arguments(TINY + ['--int8_kv_cache', '--fp8_kv_cache'])
