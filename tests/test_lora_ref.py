"""LoRA adapters per row on the CPU: the float64 restatement (tensorrt_llm/runtime/lora_ref.py) against a direct product, the
oracle wrapper against merged weights, the headroom of the GPU session cases, the PEFT loader, the exported symbols."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from oracle import quant_oracle as QO
from tensorrt_llm.plugin import capi
from tensorrt_llm.runtime import lora_ref as LR
from tensorrt_llm.runtime.lora import load_peft_adapter
from test_gpu_score import synth_bounds, synth_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def h(rng, *shape, std=1.0):
    return (rng.standard_normal(shape) * std).astype(np.float16)


# ------------------------------------------------------------------------------------------------ the rule
def test_shrink_expand_equal_the_direct_product_on_a_merged_site():
    r = np.random.default_rng(0)
    M, K, N, rank, s = 5, 72, 40, 8, 2.0
    x, A, B, y = h(r, M, K), h(r, rank, K, std=K ** -0.5), h(r, N, rank, std=0.1), h(r, M, N)
    t = LR.shrink(x, A)
    got = LR.expand(y, t, B, s)
    x64, A64, B64 = x.astype(np.float64), A.astype(np.float64), B.astype(np.float64)
    np.testing.assert_allclose(t, x64 @ A64.T, rtol=1e-13, atol=1e-13)
    ref = (y.astype(np.float64) + s * (x64 @ A64.T @ B64.T)).astype(np.float16)
    assert got.dtype == np.float16
    # one rounding of the same float64 value up to its summation order: equal but for a tie that the order breaks
    assert (got != ref).mean() < 0.01
    np.testing.assert_allclose(got.astype(np.float64), ref.astype(np.float64), rtol=2 ** -10)


def test_segmented_site_with_unequal_segments_is_three_separate_adapters():
    r = np.random.default_rng(1)
    M, K, rank, s = 4, 64, 8, 0.5
    seg_n = [256, 64, 64]  # grouped heads: q has H * Dh rows, k and v Hkv * Dh
    x, y = h(r, M, K), h(r, M, sum(seg_n))
    mods = [(h(r, rank, K, std=K ** -0.5), h(r, n, rank, std=0.1)) for n in seg_n]
    A, B = LR.pack_site(mods, seg_n, K, rank)
    assert A.shape == (3 * rank, K) and B.shape == (sum(seg_n), rank)
    got = LR.expand(y, LR.shrink(x, A), B, s, seg_n)
    off = 0
    for (Ag, Bg), n in zip(mods, seg_n):
        ref = (y[:, off:off + n].astype(np.float64)
               + s * (x.astype(np.float64) @ Ag.astype(np.float64).T @ Bg.astype(np.float64).T)).astype(np.float16)
        np.testing.assert_allclose(got[:, off:off + n].astype(np.float64), ref.astype(np.float64), rtol=2 ** -10)
        assert (got[:, off:off + n] != ref).mean() < 0.01
        off += n
    # a module the adapter lacks is zeros: those columns keep their values
    A2, B2 = LR.pack_site([mods[0], None, mods[2]], seg_n, K, rank)
    got2 = LR.expand(y, LR.shrink(x, A2), B2, s, seg_n)
    np.testing.assert_array_equal(got2[:, 256:320], y[:, 256:320])
    np.testing.assert_array_equal(got2[:, :256], got[:, :256])


def test_rows_take_their_own_adapter_and_rows_of_none_keep_their_bits():
    r = np.random.default_rng(2)
    M, K, N, rank = 6, 64, 48, 8
    x, y = h(r, M, K), h(r, M, N)
    As, Bs, ss = [h(r, rank, K, std=0.1) for _ in range(2)], [h(r, N, rank, std=0.1) for _ in range(2)], [1.0, 3.0]
    rows = np.array([0, -1, 1, 1, -1, 0])
    x[rows < 0] = np.nan  # never read
    t = LR.shrink(x, As, rows)
    got = LR.expand(y, t, Bs, ss, None, rows)
    assert np.isnan(t[rows < 0]).all() and np.isfinite(got).all()
    np.testing.assert_array_equal(got[rows < 0].view(np.uint16), y[rows < 0].view(np.uint16))
    for a in range(2):
        one = LR.expand(y[rows == a], LR.shrink(x[rows == a], As[a]), Bs[a], ss[a])
        np.testing.assert_array_equal(got[rows == a], one)


def test_rank_padding_changes_nothing():
    r = np.random.default_rng(3)
    M, K, rank, rmax = 3, 64, 8, 32
    seg_n = [40, 24]
    x, y = h(r, M, K), h(r, M, sum(seg_n))
    A, B = h(r, 2 * rank, K, std=0.1), h(r, sum(seg_n), rank, std=0.1)
    Ap, Bp = LR.pad_rank(A, B, rmax, nseg=2)
    assert Ap.shape == (2 * rmax, K) and Bp.shape == (sum(seg_n), rmax)
    s = LR.scale(16, rank)  # the scale stays the adapter's own alpha / r
    np.testing.assert_array_equal(LR.expand(y, LR.shrink(x, Ap), Bp, s, seg_n), LR.expand(y, LR.shrink(x, A), B, s, seg_n))
    assert LR.scale(16, 8) == 2.0 and LR.scale(16, 16, use_rslora=True) == 4.0


# ------------------------------------------------------------------------------------------------ the oracle wrapper
def test_wrap_oracle_linear_has_the_oracles_call_convention():
    r = np.random.default_rng(4)
    K, N, rank, s = 64, 32, 8, 2.0
    W, A, B = h(r, N, K, std=0.1), h(r, rank, K, std=0.1), h(r, N, rank, std=0.1)
    base = QO._Linear('fp16', w=W.astype(np.float32))
    wrapped = LR.wrap_oracle_linear(base, A, B, s)
    x = h(r, 3, K).astype(np.float32)
    got = wrapped(x, None)
    ref = (np.asarray(base(x, None), np.float64) + s * (x.astype(np.float64) @ A.astype(np.float64).T @ B.astype(np.float64).T))
    assert got.dtype == np.float32 and wrapped.kind == 'lora'
    np.testing.assert_array_equal(got, ref.astype(np.float16).astype(np.float32))


# The inputs of the GPU session cases (tests/test_gpu_session_lora.py): synth_model(11), prompts 12 / 7 of 20 (seed 5), adapter seed
# 77, r = 8, alpha = 16, A ~ N(0, 1 / K), B ~ N(0, 0.05^2), all seven modules.
HEADROOM = 10
R, ALPHA, ADAPTER_SEED = 8, 16.0, 77


def session_case_inputs():
    cfg, w = synth_model(11)
    cfg = dict(cfg, max_position_embeddings=256)
    r = np.random.default_rng(5)
    ids = r.integers(3, cfg['vocab_size'], (2, 20)).astype(np.int32)
    lens = np.array([12, 7], np.int32)
    for b in range(2):
        ids[b, lens[b]:] = 2
    feed = r.integers(3, cfg['vocab_size'], (2, 23)).astype(np.int32)
    return cfg, w, ids, lens, feed


def merged_weights(cfg, w, adapter, s):
    """f16(W + s B A) of every adapted module, in the engine's fused layout"""
    D, I = cfg['hidden_size'], cfg['inter_size']
    out = dict(w)
    rows = {'attention.q': ('attention.qkv', 0, D), 'attention.k': ('attention.qkv', D, D), 'attention.v': ('attention.qkv', 2 * D, D),
            'attention.dense': ('attention.dense', 0, D), 'mlp.fc': ('mlp.fc', 0, I), 'mlp.gate': ('mlp.gate', 0, I),
            'mlp.proj': ('mlp.proj', 0, D)}
    for i in range(cfg['num_layers']):
        for mod, (lin, off, n) in rows.items():
            a = adapter.get(f'layers.{i}.{mod}.lora_a')
            if a is None:
                continue
            b = adapter[f'layers.{i}.{mod}.lora_b']
            k = f'layers.{i}.{lin}.weight'
            W = out[k].astype(np.float64).copy()
            W[off:off + n] += s * (b.astype(np.float64) @ a.astype(np.float64))
            out[k] = W.astype(np.float16)
    return out


def test_wrapped_fp16_oracle_equals_the_model_with_merged_weights():
    cfg, w, ids, lens, feed = session_case_inputs()
    adapter, s = LR.random_adapter(cfg, ADAPTER_SEED, R), LR.scale(ALPHA, R)
    n_new = 5
    model = LR.adapt_oracle(QO._fp16_model(cfg, w), cfg, [(adapter, s)], R)
    got, _ = QO._forward(model, ids, lens, n_new, feed)
    ref, _ = QO.run_fp16_model(cfg, merged_weights(cfg, w, adapter, s), ids, lens, n_new, feed_ids=feed)
    for i, (g, z) in enumerate(zip(got, ref)):
        bmax, bmean = synth_bounds('fp16', z)
        d = np.abs(g.astype(np.float64) - z)
        print(f'step {i}: max |d| {d.max():.3e} (bound {bmax:.3e}), mean {d.mean():.3e} (bound {bmean:.3e})')
        assert d.max() <= bmax and d.mean() <= bmean


def test_headroom_of_the_gpu_session_cases():
    """the adapter moves the oracle's logits by at least 10 x synth_bounds' max bound, at the context step and the fourth forced
    step: a session that ignores or swaps the selection cannot stay within one bound of the right oracle"""
    cfg, w, ids, lens, feed = session_case_inputs()
    adapter, s = LR.random_adapter(cfg, ADAPTER_SEED, R), LR.scale(ALPHA, R)
    base = QO._fp16_model(cfg, w)
    zb, _ = QO._forward(base, ids, lens, 5, feed)
    za, _ = QO._forward(LR.adapt_oracle(base, cfg, [(adapter, s)], R), ids, lens, 5, feed)
    for i in (0, 4):
        bmax, _ = synth_bounds('fp16', zb[i])
        move = np.abs(za[i].astype(np.float64) - zb[i]).max(axis=1)
        print(f'step {i}: the adapter moves the logits by {move / bmax} x the bound {bmax:.3e}')
        assert (move >= HEADROOM * bmax).all()
    # per-sequence selection in the oracle: sequence 1 on none is the base model's sequence 1
    zs, _ = QO._forward(LR.adapt_oracle(base, cfg, [(adapter, s), None], R), ids, lens, 5, feed)
    for i in (0, 4):
        np.testing.assert_array_equal(zs[i][1], zb[i][1])
        np.testing.assert_array_equal(zs[i][0], za[i][0])


# ------------------------------------------------------------------------------------------------ PEFT directories
HF_NAMES = {'attention.q': 'self_attn.q_proj', 'attention.k': 'self_attn.k_proj', 'attention.v': 'self_attn.v_proj',
            'attention.dense': 'self_attn.o_proj', 'mlp.fc': 'mlp.gate_proj', 'mlp.gate': 'mlp.up_proj', 'mlp.proj': 'mlp.down_proj'}


def write_peft_dir(path, adapter, r, alpha, modules, **extra):
    """HF PEFT's layout, written with safetensors + json alone"""
    from safetensors.numpy import save_file
    os.makedirs(path, exist_ok=True)
    sd = {}
    for k, v in adapter.items():
        m = re.match(r'layers\.(\d+)\.(.+)\.lora_([ab])$', k)
        sd[f'base_model.model.model.layers.{m.group(1)}.{HF_NAMES[m.group(2)]}.lora_{m.group(3).upper()}.weight'] = \
            np.ascontiguousarray(v.astype(np.float32))
    save_file(sd, os.path.join(path, 'adapter_model.safetensors'))
    cfg = dict(peft_type='LORA', r=r, lora_alpha=alpha, target_modules=[HF_NAMES[LR.MODULE_NAMES[m][0]].split('.')[1] for m in modules],
               bias='none', use_dora=False, use_rslora=False, modules_to_save=None, task_type='CAUSAL_LM')
    cfg.update(extra)
    with open(os.path.join(path, 'adapter_config.json'), 'w') as f:
        json.dump(cfg, f)
    return path


def test_peft_directory_round_trips_and_every_refusal_names_its_field(tmp_path):
    cfg, _ = synth_model(11)
    adapter = LR.random_adapter(cfg, 3, 8, modules=('q', 'v', 'down'))
    mc = dict(num_layers=cfg['num_layers'], lora_max_rank=8, lora_target_modules='q,k,v,o,down')
    got = load_peft_adapter(write_peft_dir(str(tmp_path / 'ok'), adapter, 8, 16, ('q', 'v', 'down')), mc)
    assert got['r'] == 8 and got['alpha'] == 16.0 and got['use_rslora'] is False and got['target_modules'] == ['down', 'q', 'v']
    assert sorted(got['tensors']) == sorted(adapter)
    for k in adapter:  # fp16 -> fp32 on disk -> fp16: the same bits
        assert got['tensors'][k].dtype == np.float16
        np.testing.assert_array_equal(got['tensors'][k], adapter[k])
    assert load_peft_adapter(write_peft_dir(str(tmp_path / 'rs'), adapter, 8, 16, ('q', 'v', 'down'), use_rslora=True), mc)['use_rslora']
    for name, extra, field in (('bias', dict(bias='all'), 'bias'), ('dora', dict(use_dora=True), 'use_dora'),
                               ('save', dict(modules_to_save=['lm_head']), 'modules_to_save'),
                               ('target', dict(target_modules=['q_proj', 'embed_tokens']), 'target_modules')):
        with pytest.raises(ValueError, match=field):
            load_peft_adapter(write_peft_dir(str(tmp_path / name), adapter, 8, 16, ('q', 'v', 'down'), **extra), mc)
    with pytest.raises(ValueError, match='lora_max_rank'):
        load_peft_adapter(str(tmp_path / 'ok'), dict(mc, lora_max_rank=4))
    # storage types: float32 beyond fp16's range and a bfloat16 file are refused by the tensor's name, not rounded to inf or mis-read
    big = dict(adapter)
    big['layers.0.attention.q.lora_b'] = adapter['layers.0.attention.q.lora_b'].astype(np.float32) * 1e6
    with pytest.raises(ValueError, match=r'layers\.0\.self_attn\.q_proj\.lora_B.*not finite'):
        load_peft_adapter(write_peft_dir(str(tmp_path / 'big'), big, 8, 16, ('q', 'v', 'down')), mc)
    import torch
    from safetensors.torch import save_file as save_torch
    d = write_peft_dir(str(tmp_path / 'bf16'), adapter, 8, 16, ('q', 'v', 'down'))
    from safetensors.numpy import load_file
    save_torch({k: torch.from_numpy(v).to(torch.bfloat16) for k, v in load_file(os.path.join(d, 'adapter_model.safetensors')).items()},
               os.path.join(d, 'adapter_model.safetensors'))
    with pytest.raises(ValueError, match='BF16'):
        load_peft_adapter(d, mc)
    with pytest.raises(ValueError, match='lora_target_modules'):
        load_peft_adapter(str(tmp_path / 'ok'), dict(mc, lora_target_modules='q,v'))


# ------------------------------------------------------------------------------------------------ the C ABI
NEW_SYMBOLS = ('tllm_lora_shrink', 'tllm_lora_expand', 'tllm_session_lora_set_tensor', 'tllm_session_lora_commit',
               'tllm_session_lora_clear', 'tllm_session_lora_select', 'tllm_session_graph_captures')


def test_library_exports_every_new_symbol_and_create_refuses_by_key():
    with open(os.path.join(ROOT, 'include', 'tllm_runtime_api.h')) as f:
        text = f.read()
    lib = capi.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b' + name + r'\s*\(', text), f'{name} is not declared'
        assert hasattr(lib, name), f'{name} is declared but not exported'
    lib.tllm_session_create.restype = ctypes.c_void_p
    lib.tllm_session_create.argtypes = [ctypes.c_char_p]
    lib.tllm_session_destroy.argtypes = [ctypes.c_void_p]
    base = 'num_layers=1\nnum_heads=2\nhidden_size=64\ninter_size=24\nvocab_size=128\n'
    for extra, word in (('lora_max_rank=12\n', 'lora_max_rank'), ('lora_max_rank=8\nlora_max_adapters=9\n', 'lora_max_adapters'),
                        ('lora_max_rank=8\nlora_target_modules=q,lm_head\n', 'lora_target_modules'),
                        ('lora_max_rank=8\nquant_mode=6\n', 'SmoothQuant'), ('lora_max_rank=8\ntp_size=2\n', 'tp_size')):
        assert not lib.tllm_session_create((base + extra).encode())
        assert word in capi.last_error(), capi.last_error()
    s = lib.tllm_session_create((base + 'lora_max_rank=8\nlora_max_adapters=2\nlora_target_modules=q, v,down\n').encode())
    assert s
    lib.tllm_session_destroy(s)
