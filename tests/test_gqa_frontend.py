"""Grouped-query attention through the front end: `build.py --n_kv_head`, the engine header and `tllm_engine_verify`, the HF -> FT
converter and both weight loaders (per-rank q / k / v slices at tp 1 and tp 2), the argument-time refusals, and the session
configuration key.  Host-only: no GPU needed (`tllm_session_create` allocates nothing on the device)."""
import ctypes
import json
import os
import struct
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, 'trtllm-llama_amd', 'examples', 'llama_quant')
sys.path.insert(0, EX)

from tensorrt_llm.plugin import capi  # noqa: E402

H, HKV, D, DH = 4, 2, 128, 32
TINY = ['--n_layer', '2', '--n_head', str(H), '--n_embd', str(D), '--inter_size', '96', '--vocab_size', '128', '--n_positions', '64',
        '--max_batch_size', '2', '--max_input_len', '16', '--max_output_len', '8', '--log_level', 'error', '--random_seed', '3']
HF_GQA = dict(hidden_size=64, num_attention_heads=4, num_key_value_heads=2, intermediate_size=128, vocab_size=96,
              num_hidden_layers=2, max_position_embeddings=64, rms_norm_eps=1e-6, attention_bias=False, tie_word_embeddings=False)


def hf_gqa_model(seed=0):
    """A seeded random HF LLaMA with grouped K/V heads: 4 heads, 2 K/V heads, hidden 64 (head size 16 is below what the attention
    plugin's front end takes, so the engine tests below use hidden 128: `hf_gqa_model_128`)."""
    import torch
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(seed)
    m = LlamaForCausalLM(LlamaConfig(**HF_GQA)).float().eval()
    with torch.no_grad():
        for p in m.parameters():
            if p.ndim == 2:
                p.mul_(2.0)
    return m


def hf_gqa_model_128(tmp_path, seed=0):
    import torch
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(seed)
    m = LlamaForCausalLM(LlamaConfig(**dict(HF_GQA, hidden_size=D))).float().eval()
    with torch.no_grad():
        for p in m.parameters():
            if p.ndim == 2:
                p.mul_(2.0)
    d = tmp_path / 'hf'
    m.save_pretrained(d, safe_serialization=True)
    return m, str(d)


def verify(engine: bytes):
    lib = capi.load_library()
    lib.tllm_engine_verify.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    lib.tllm_engine_verify.restype = ctypes.c_int32
    rc = lib.tllm_engine_verify(engine, len(engine))
    return rc, (capi.last_error() if rc else '')


def parse(engine: bytes):
    """-> (header text, {name: (dims, array bytes offset, nbytes)}, table bytes, data bytes)"""
    assert engine[:8] == b'TLLMENG1'
    hlen, = struct.unpack_from('<Q', engine, 8)
    text = engine[16:16 + hlen].decode()
    off = t0 = 16 + hlen
    nt, = struct.unpack_from('<Q', engine, off)
    off += 8
    tensors = {}
    for _ in range(nt):
        nl, = struct.unpack_from('<I', engine, off)
        name = engine[off + 4:off + 4 + nl].decode()
        off += 4 + nl
        _, nd = struct.unpack_from('<ii', engine, off)
        dims = struct.unpack_from(f'<{nd}q', engine, off + 8)
        nbytes, o = struct.unpack_from('<QQ', engine, off + 8 + 8 * nd)
        off += 8 + 8 * nd + 16
        tensors[name] = (list(dims), o, nbytes)
    data0 = (off + 63) // 64 * 64
    return text, tensors, engine[t0:off], engine[data0:]


def with_header(engine: bytes, fn) -> bytes:
    text, _, table, data = parse(engine)
    tb = fn(text).encode()
    blob = b'TLLMENG1' + struct.pack('<Q', len(tb)) + tb + table
    blob += b'\0' * ((-len(blob)) % 64)
    return blob + data


def build(extra):
    import build as B
    d = tempfile.mkdtemp()
    B.run_build(TINY + ['--output_dir', d] + extra)
    engines = [open(os.path.join(d, f), 'rb').read() for f in sorted(os.listdir(d)) if f.endswith('.engine')]
    return d, engines


def test_build_with_n_kv_head():
    d, (engine, ) = build(['--n_kv_head', str(HKV)])
    bc = json.load(open(os.path.join(d, 'config.json')))['builder_config']
    assert bc['num_heads'] == H and bc['num_kv_heads'] == HKV
    text, tensors, _, _ = parse(engine)
    assert f'num_kv_heads={HKV}' in text.split('\n')
    for i in range(2):
        assert tensors[f'layers.{i}.attention.qkv.weight'][0] == [(H + 2 * HKV) * DH, D]
        assert tensors[f'layers.{i}.attention.dense.weight'][0] == [D, D]
    assert verify(engine) == (0, '')
    # the QKV weight must be the one its configuration implies: the same engine read as multi-head (key dropped) is refused ...
    rc, why = verify(with_header(engine, lambda t: t.replace(f'num_kv_heads={HKV}\n', '')))
    assert rc != 0 and 'attention.qkv' in why and 'num_kv_heads' in why, why
    # ... and a multi-head engine (QKV cut to ... 3 * H * Dh rows) under a grouped configuration likewise
    _, (mha, ) = build([])
    rc, why = verify(with_header(mha, lambda t: t.replace(f'num_heads={H}\n', f'num_heads={H}\nnum_kv_heads={HKV}\n')))
    assert rc != 0 and 'attention.qkv' in why and 'num_kv_heads' in why, why


@pytest.mark.parametrize('extra', [['--use_weight_only'], ['--int8_kv_cache'], ['--fp8_kv_cache', '--paged_kv_cache'],
                                   ['--world_size', '2', '--remove_input_padding']])
def test_grouped_engines_of_the_other_modes_are_accepted(extra):
    _, engines = build(['--n_kv_head', str(HKV)] + extra)
    for e in engines:
        assert verify(e) == (0, '')
        text, tensors, _, _ = parse(e)
        if '--world_size' in extra:
            assert tensors['layers.0.attention.qkv.weight'][0] == [(H + 2 * HKV) * DH // 2, D]


def test_an_mha_build_is_byte_identical_with_n_kv_head_equal_to_n_head():
    _, a = build([])
    _, b = build(['--n_kv_head', str(H)])
    assert a == b and 'num_kv_heads' not in parse(a[0])[0].split('network_json=')[0]


def test_smoothquant_with_grouped_heads_fails_at_argument_time(tmp_path, capsys):
    import build as B
    with pytest.raises(SystemExit):
        B.parse_arguments(TINY + ['--n_kv_head', str(HKV), '--use_smooth_quant'])
    assert 'grouped K/V heads' in capsys.readouterr().err
    for bad in (['--n_kv_head', '3'], ['--n_kv_head', '8'], ['--n_kv_head', '2', '--world_size', '4']):
        with pytest.raises(SystemExit):
            B.parse_arguments(TINY + bad)
    import hf_llama_convert as C
    _, hf_dir = hf_gqa_model_128(tmp_path)
    with pytest.raises(SystemExit) as e:
        C.check_grouped_heads(C.ProgArgs(out_dir=str(tmp_path / 'ft'), in_file=hf_dir, smoothquant=0.5))
    assert 'grouped K/V heads' in str(e.value)


@pytest.mark.parametrize('tp', [1, 2])
def test_converter_then_build_slices_q_k_v_per_rank(tmp_path, tp):
    """hf_llama_convert (with KV-cache calibration) -> build.py --model_dir: rank r's fused QKV is rows r of q, of k and of v of the
    HF weights, in the block order q | k | v; the int8 cache scale is max|qkv output| / 127 over the calibration prompts."""
    import build as B
    import hf_llama_convert as C
    m, hf_dir = hf_gqa_model_128(tmp_path)
    ft = C.run_conversion(C.ProgArgs(out_dir=str(tmp_path / 'ft'), in_file=hf_dir, tensor_parallelism=tp, calibrate_kv_cache=True,
                                     calib_samples=2, calib_len=16))
    out = str(tmp_path / 'eng')
    B.run_build(['--model_dir', str(ft), '--world_size', str(tp), '--output_dir', out, '--max_batch_size', '2', '--max_input_len', '16',
                 '--max_output_len', '8', '--log_level', 'error', '--int8_kv_cache'])
    assert json.load(open(os.path.join(out, 'config.json')))['builder_config']['num_kv_heads'] == HKV
    sd = {k: v.detach().numpy() for k, v in m.state_dict().items()}
    files = sorted(f for f in os.listdir(out) if f.endswith('.engine'))
    assert len(files) == tp
    for rank, f in enumerate(files):
        e = open(os.path.join(out, f), 'rb').read()
        assert verify(e) == (0, '')
        text, tensors, _, data = parse(e)
        assert f'num_kv_heads={HKV}' in text.split('\n')
        for i in range(2):
            dims, o, nb = tensors[f'layers.{i}.attention.qkv.weight']
            w = np.frombuffer(data[o:o + nb], np.float16).reshape(dims)
            q, k, v = (sd[f'model.layers.{i}.self_attn.{n}_proj.weight'] for n in 'qkv')
            want = np.concatenate([np.split(x, tp, axis=0)[rank] for x in (q, k, v)], axis=0).astype(np.float16)
            assert dims == [(H + 2 * HKV) * DH // tp, D]
            np.testing.assert_array_equal(w, want)
            dims, o, nb = tensors[f'layers.{i}.attention.kv_quant_orig_scale']
            assert np.frombuffer(data[o:o + nb], np.float32)[0] > 0


def test_hf_loader_slices_q_k_v_per_rank(tmp_path):
    import build as B
    m, hf_dir = hf_gqa_model_128(tmp_path)
    out = str(tmp_path / 'eng')
    B.run_build(['--hf_model_dir', hf_dir, '--n_layer', '2', '--n_head', str(H), '--n_embd', str(D), '--inter_size', '128',
                 '--vocab_size', '96', '--n_positions', '64', '--world_size', '2', '--output_dir', out, '--max_batch_size', '2',
                 '--max_input_len', '16', '--max_output_len', '8', '--log_level', 'error'])  # n_kv_head from the HF config
    sd = {k: v.detach().numpy() for k, v in m.state_dict().items()}
    for rank, f in enumerate(sorted(f for f in os.listdir(out) if f.endswith('.engine'))):
        e = open(os.path.join(out, f), 'rb').read()
        assert verify(e) == (0, '')
        _, tensors, _, data = parse(e)
        dims, o, nb = tensors['layers.1.attention.qkv.weight']
        q, k, v = (sd[f'model.layers.1.self_attn.{n}_proj.weight'] for n in 'qkv')
        want = np.concatenate([np.split(x, 2, axis=0)[rank] for x in (q, k, v)], axis=0).astype(np.float16)
        np.testing.assert_array_equal(np.frombuffer(data[o:o + nb], np.float16).reshape(dims), want)


def session_create(**kw):
    lib = capi.load_library()
    lib.tllm_session_create.argtypes = [ctypes.c_char_p]
    lib.tllm_session_create.restype = ctypes.c_void_p
    lib.tllm_session_destroy.argtypes = [ctypes.c_void_p]
    cfg = dict(num_layers=2, num_heads=8, hidden_size=256, inter_size=96, vocab_size=128)
    cfg.update(kw)
    s = lib.tllm_session_create('\n'.join(f'{k}={v}' for k, v in cfg.items()).encode())
    if s:
        lib.tllm_session_destroy(s)
        return ''
    return capi.last_error()


def test_session_create_refuses_bad_kv_head_counts():
    assert session_create() == '' and session_create(num_kv_heads=8) == '' and session_create(num_kv_heads=2) == ''
    assert session_create(num_kv_heads=1) == '' and session_create(num_kv_heads=4, tp_size=2) == ''
    for kw in (dict(num_kv_heads=3), dict(num_kv_heads=16), dict(num_kv_heads=0), dict(num_kv_heads=2, tp_size=4),
               dict(num_kv_heads=2, quant_mode=2 | 4)):  # the last: SmoothQuant (QuantMode int8 weights 2 + activations 4)
        why = session_create(**kw)
        assert 'num_kv_heads' in why, (kw, why)
