"""Hugging Face PEFT LoRA adapters -> the tensors NativeSession.lora_load takes.

Reads PEFT's own layout - adapter_config.json and adapter_model.safetensors - with `safetensors` alone; `peft` is not needed.
'...layers.{i}.self_attn.q_proj.lora_A.weight' [r, in] becomes 'layers.{i}.attention.q.lora_a', '.lora_B.weight' [out, r] becomes
'.lora_b'.  hf_llama_convert.py stores q / k / v / o / gate / up / down as plain transposes for every engine an adapter can be
loaded into (its only row / column transformation, the SmoothQuant smoother, belongs to engines that refuse adapters; HF's
rotary pairing is the engine's NeoX pairing), so B's rows and A's columns are taken as they are."""
import json
import os
import re
import struct

import numpy as np

# HF module -> the engine's module name inside a layer (q, k, v are segments of the fused attention.qkv)
HF_MODULES = {'q_proj': 'attention.q', 'k_proj': 'attention.k', 'v_proj': 'attention.v', 'o_proj': 'attention.dense',
              'gate_proj': 'mlp.fc', 'up_proj': 'mlp.gate', 'down_proj': 'mlp.proj'}
# ... and its key in the session's lora_target_modules
HF_MODULE_KEYS = {'q_proj': 'q', 'k_proj': 'k', 'v_proj': 'v', 'o_proj': 'o', 'gate_proj': 'gate', 'up_proj': 'up',
                  'down_proj': 'down'}
_KEY = re.compile(r'(?:^|\.)layers\.(\d+)\.(?:self_attn|mlp)\.(\w+)\.lora_([AB])(?:\.[\w-]+)?\.weight$')


def _get(cfg, key, default=None):
    return cfg.get(key, default) if isinstance(cfg, dict) else getattr(cfg, key, default)


def _safetensors_dtypes(path):
    """tensor name -> dtype string of a safetensors file, from its header alone (8-byte length, then JSON)"""
    with open(path, 'rb') as f:
        n, = struct.unpack('<Q', f.read(8))
        header = json.loads(f.read(n))
    return {k: v['dtype'] for k, v in header.items() if k != '__metadata__'}


def load_peft_adapter(adapter_dir, model_config):
    """-> dict(tensors={engine name: fp16 array}, alpha=float, r=int, use_rslora=bool, target_modules=[session keys]).
    model_config (dict or object): num_layers, and - when present - lora_max_rank and lora_target_modules (comma list or list)
    of the session the adapter is meant for.  Refused, each naming the field: bias != "none", use_dora, modules_to_save,
    rank_pattern / alpha_pattern, target modules outside q/k/v/o/gate/up/down_proj, r above lora_max_rank.
    The matrices must be stored as float16 or float32 (F16 / F32): float32 is rounded to fp16, what the kernels read, and a value
    that does not survive that - beyond 65504, or not finite - is refused by the tensor's name; any other storage type (bfloat16:
    numpy has none) is refused by name too - save the adapter as float32 or float16."""
    from safetensors.numpy import load_file
    with open(os.path.join(adapter_dir, 'adapter_config.json')) as f:
        ac = json.load(f)
    if ac.get('peft_type', 'LORA') != 'LORA':
        raise ValueError(f"adapter_config.json: peft_type {ac.get('peft_type')!r} is not LORA")
    if ac.get('bias', 'none') != 'none':
        raise ValueError(f"adapter_config.json: bias = {ac['bias']!r} is not built (only \"none\")")
    if ac.get('use_dora'):
        raise ValueError('adapter_config.json: use_dora is not built')
    if ac.get('modules_to_save'):
        raise ValueError(f"adapter_config.json: modules_to_save = {ac['modules_to_save']!r} is not built (full-weight copies)")
    for pat in ('rank_pattern', 'alpha_pattern'):
        if ac.get(pat):
            raise ValueError(f'adapter_config.json: {pat} is not built (one rank and one alpha per adapter)')
    targets = ac.get('target_modules') or []
    if isinstance(targets, str):
        raise ValueError(f'adapter_config.json: target_modules = {targets!r} must be a list of module names')
    bad = sorted(t for t in targets if t.split('.')[-1] not in HF_MODULES)
    if bad:
        raise ValueError(f'adapter_config.json: target_modules {bad} outside {sorted(HF_MODULES)}')
    r, alpha = int(ac['r']), float(ac.get('lora_alpha', ac['r']))
    max_rank = _get(model_config, 'lora_max_rank')
    if max_rank is not None and r > int(max_rank):
        raise ValueError(f'adapter_config.json: r = {r} above the session\'s lora_max_rank {max_rank}')
    allowed = _get(model_config, 'lora_target_modules')
    if isinstance(allowed, str):
        allowed = [m.strip() for m in allowed.split(',') if m.strip()]
    num_layers = _get(model_config, 'num_layers')
    path = os.path.join(adapter_dir, 'adapter_model.safetensors')
    tensors, used = {}, set()
    other = {k: d for k, d in _safetensors_dtypes(path).items() if d not in ('F16', 'F32')}
    if other:
        k = sorted(other)[0]
        raise ValueError(f'adapter_model.safetensors: {k} is stored as {other[k]}; float16 or float32 (F16 / F32) is read - '
                         'save the adapter in one of them')
    for key, v in load_file(path).items():
        m = _KEY.search(key)
        if not m or m.group(2) not in HF_MODULES:
            raise ValueError(f'adapter_model.safetensors: {key} is not a LoRA matrix of a target module ({sorted(HF_MODULES)})')
        layer, mod, ab = int(m.group(1)), m.group(2), m.group(3)
        if num_layers is not None and layer >= int(num_layers):
            raise ValueError(f'adapter_model.safetensors: {key} names layer {layer} of a model with {num_layers}')
        if allowed is not None and HF_MODULE_KEYS[mod] not in allowed:
            raise ValueError(f"adapter_config.json: target_modules has {mod} ({HF_MODULE_KEYS[mod]}), outside the session's "
                             f"lora_target_modules {','.join(allowed)}")
        if v.ndim != 2 or v.shape[0 if ab == 'A' else 1] != r:
            raise ValueError(f'adapter_model.safetensors: {key} has shape {v.shape}, r = {r}')
        with np.errstate(over='ignore'):
            h = np.ascontiguousarray(v.astype(np.float16))
        if not np.isfinite(h).all():
            raise ValueError(f'adapter_model.safetensors: {key} has values that are not finite in float16 (|v| up to '
                             f'{float(np.abs(v[np.isfinite(v)]).max()) if np.isfinite(v).any() else float("nan"):.4g})')
        tensors[f'layers.{layer}.{HF_MODULES[mod]}.lora_{ab.lower()}'] = h
        used.add(HF_MODULE_KEYS[mod])
    if not tensors:
        raise ValueError('adapter_model.safetensors: no LoRA matrices')
    return dict(tensors=tensors, alpha=alpha, r=r, use_rslora=bool(ac.get('use_rslora', False)), target_modules=sorted(used))
