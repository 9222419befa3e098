"""LoRA through the front-end: the trained stochastic parent (tests/golden/trained_llama_stochastic) goes through
hf_llama_convert.py -> build.py --lora_max_rank 8 -> GenerationSession.load_lora(a PEFT directory the test writes) and
score(..., lora_slots=...), and is held to HF transformers on the CPU with f32(W + s B A) merged into its state dict; run.py
--lora_dir decodes and produces other text than the base run.

Bound: the one tests/test_gpu_score.py::test_trained_stochastic_parent uses for the fp16 engine, synth_bounds('fp16', z) on the
per-token log-probs.  The adapter (seed 9, r = 8, alpha = 32, all seven modules) moves HF's own log-probs by more than 10 x that
bound - asserted on the HF side - so an engine that ignored it would be far outside."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, 'trtllm-llama_amd', 'examples', 'llama_quant')
sys.path.insert(0, EX)

import trained_parents as TP  # noqa: E402
from tensorrt_llm.runtime import lora_ref as LR  # noqa: E402
from tensorrt_llm.runtime import scoring_ref as R  # noqa: E402
from test_gpu_score import _trained_prompts, synth_bounds  # noqa: E402
from test_lora_ref import HF_NAMES, write_peft_dir  # noqa: E402

pytestmark = pytest.mark.gpu
RANK, ALPHA, SEED = 8, 32.0, 9
ALL = 'q,k,v,o,gate,up,down'


def hf_position_logits(adapter, s, ids, lens):
    """[B, S, V] float64 from HF LlamaForCausalLM in fp32 on the CPU: the fixture's weights as the engine holds them (fp16 values),
    with s B A of every adapted module added in fp32"""
    import torch
    from transformers import LlamaForCausalLM
    m = LlamaForCausalLM.from_pretrained(TP.PARENTS['stochastic'], torch_dtype=torch.float32).eval()
    sd = {k: v.half().float() for k, v in m.state_dict().items()}
    if adapter is not None:
        for k in [k for k in adapter if k.endswith('.lora_a')]:
            layer, mod = k.split('.')[1], '.'.join(k.split('.')[2:-1])
            a, b = torch.from_numpy(adapter[k].astype(np.float32)), torch.from_numpy(adapter[k[:-1] + 'b'].astype(np.float32))
            sd[f'model.layers.{layer}.{HF_NAMES[mod]}.weight'] += s * (b @ a)
    m.load_state_dict(sd)
    with torch.no_grad():
        z = m(torch.from_numpy(ids.astype(np.int64))).logits.double().numpy()
    for b in range(ids.shape[0]):
        z[b, int(lens[b]) - 1:] = 0
    return z


def test_trained_parent_through_convert_build_load_lora_score_and_run(tmp_path):
    import build as Bd
    import hf_llama_convert as C
    import run as Rn
    from tensorrt_llm.runtime import GenerationSession  # noqa: F401
    cfg, _ = TP.oracle_weights('stochastic')
    ids, lens = _trained_prompts()
    adapter, s = LR.random_adapter(cfg, SEED, RANK), LR.scale(ALPHA, RANK)
    # ---- HF side: the reference and the headroom
    z_base, z = hf_position_logits(None, s, ids, lens), hf_position_logits(adapter, s, ids, lens)
    bmax, bmean = synth_bounds('fp16', z)
    lp_base, _ = R.sequence_scores(z_base, ids, lens)
    lp_ref, _ = R.sequence_scores(z, ids, lens)
    move = np.abs(lp_ref - lp_base).max()
    print(f'the adapter moves HF\'s log-probs by up to {move:.3f} = {move / bmax:.1f} x the bound {bmax:.3e}')
    assert move >= 10 * bmax
    # ---- the engine
    ft = C.run_conversion(C.ProgArgs(out_dir=str(tmp_path / 'ft'), in_file=TP.PARENTS['stochastic']))
    eng = str(tmp_path / 'eng')
    Bd.run_build(['--model_dir', str(ft), '--output_dir', eng, '--max_batch_size', '2', '--max_input_len', '64', '--max_output_len', '16',
                  '--log_level', 'error', '--lora_max_rank', str(RANK), '--lora_max_adapters', '2', '--lora_target_modules', ALL])
    peft = write_peft_dir(str(tmp_path / 'peft'), adapter, RANK, ALPHA, LR.MODULES)
    dec, _ = Rn.load_session(eng)
    got = dec.load_lora(peft, slot=1)
    assert got['r'] == RANK and got['alpha'] == ALPHA
    dec.setup(2, 64, 4)
    out = dec.score(ids, lens, lora_slots=[1, 1])
    scored = np.zeros(ids.shape, bool)
    for b in range(2):
        scored[b, 1:int(lens[b])] = True
    d = np.abs(out['log_probs'].astype(np.float64) - lp_ref)[scored]
    print(f'[score under the adapter] max |d log_prob| {d.max():.3e} (bound {bmax:.3e}), mean {d.mean():.3e} (bound {bmean:.3e})')
    assert d.max() <= bmax and d.mean() <= bmean
    base = dec.score(ids, lens, lora_slots=[-1, -1])  # the same session back on no adapter: the base model's scores
    d0 = np.abs(base['log_probs'].astype(np.float64) - lp_base)[scored]
    print(f'[score under no adapter] max |d log_prob| {d0.max():.3e}, mean {d0.mean():.3e}')
    assert d0.max() <= bmax and d0.mean() <= bmean
    dec.runtime.close()
    # ---- run.py: decodes under the adapter, and to other tokens than the base run
    prompt = str(tmp_path / 'prompt.npy')
    np.save(prompt, ids[0, :24])
    runs = {}
    for name, extra in (('base', {}), ('lora', dict(lora_dir=[peft], lora_slots='0'))):
        path = str(tmp_path / f'{name}.npy')
        Rn.generate(16, engine_dir=eng, input_file=prompt, output_npy=path, num_runs=1, **extra)
        runs[name] = np.load(path)
    assert runs['base'].shape == runs['lora'].shape == (1, 24 + 16)
    np.testing.assert_array_equal(runs['base'][:, :24], runs['lora'][:, :24])
    assert (runs['base'][:, 24:] != runs['lora'][:, 24:]).any(), 'the adapter changed none of 16 generated tokens'
