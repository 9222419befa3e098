#!/usr/bin/env python3
"""run.py of the llama_quant example (T/examples/llama_quant/run.py:29-198): load config.json + the rank's engine,
tokenise (or take --input_tokens), then 55 x (setup + decode), printing the per-run latencies and
`llama-run (mean latency: X sec)` over runs 5..54."""
import argparse
import csv
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))

import tensorrt_llm  # noqa: E402
from tensorrt_llm.runtime import GenerationSession, ModelConfig, SamplingConfig  # noqa: E402

from build import get_engine_name  # noqa: E402

EOS_TOKEN = 2
PAD_TOKEN = 2


def parse_arguments(args=None):
    p = argparse.ArgumentParser()
    p.add_argument('--max_output_len', type=int, required=True)
    p.add_argument('--log_level', type=str, default='error')
    p.add_argument('--engine_dir', type=str, default='llama_outputs')
    p.add_argument('--tokenizer_dir', type=str, default='.', help='Directory containing the tokenizer.model.')
    p.add_argument('--input_text', type=str, default='Born in north-east France, Soyer trained as a')
    p.add_argument('--input_tokens', dest='input_file', type=str, default=None,
                   help='CSV or Numpy file containing tokenized input. Alternative to text input.')
    p.add_argument('--output_csv', type=str, default=None)
    p.add_argument('--output_npy', type=str, default=None)
    p.add_argument('--num_beams', type=int, default=1)
    # device-side sampling (num_beams 1); the defaults are greedy decoding
    p.add_argument('--top_k', type=int, default=1)
    p.add_argument('--top_p', type=float, default=0.0)
    p.add_argument('--temperature', type=float, default=1.0)
    p.add_argument('--repetition_penalty', type=float, default=1.0)
    p.add_argument('--random_seed', type=int, default=None)
    p.add_argument('--num_runs', type=int, default=55)
    # greedy decoding with prompt-lookup speculation (GenerationSession.decode_lookup): the same tokens, N ids verified per pass
    p.add_argument('--prompt_lookup_tokens', type=int, default=0,
                   help='N in [2, 32]: draft from earlier n-gram matches of the text and verify N ids per pass; 0 = off.')
    p.add_argument('--prompt_lookup_ngram', type=int, default=3, help='longest n-gram the lookup matches, 1 to 8')
    p.add_argument('--prompt_lookup_sampling', action='store_true',
                   help='let --prompt_lookup_tokens combine with --top_k / --top_p / --temperature / --repetition_penalty / '
                   '--random_seed: a draft is kept where it equals the token the sampler draws (the same tokens as without lookup).')
    # LoRA adapters (an engine built with --lora_max_rank): HF PEFT directories go into slots 0, 1, ... in the order given
    p.add_argument('--lora_dir', type=str, nargs='+', default=None, help='HF PEFT adapter directories (adapter_config.json + '
                   'adapter_model.safetensors)')
    p.add_argument('--lora_slots', type=str, default=None, help='comma list, one slot per sequence of the batch, -1 = no adapter '
                   '(default: slot 0 for every sequence when --lora_dir is given)')
    return p.parse_args(args)


def load_session(engine_dir):
    with open(Path(engine_dir) / 'config.json') as f:
        config = json.load(f)
    bc = config['builder_config']
    dtype, world_size = bc['precision'], bc['tensor_parallel']
    assert world_size == tensorrt_llm.mpi_world_size(), \
        f'Engine world size ({world_size}) != Runtime world size ({tensorrt_llm.mpi_world_size()})'
    runtime_rank = tensorrt_llm.mpi_rank()
    mapping = tensorrt_llm.Mapping(world_size, runtime_rank)
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.set_device(runtime_rank % max(torch.cuda.device_count(), 1))
    except ImportError:
        pass
    model_config = ModelConfig(num_heads=bc['num_heads'] // world_size, hidden_size=bc['hidden_size'] // world_size,
                               vocab_size=bc['vocab_size'], num_layers=bc['num_layers'],
                               gpt_attention_plugin=bool(config['plugin_config']['gpt_attention_plugin']),
                               multi_query_mode=bc.get('multi_query_mode', False),
                               remove_input_padding=config['plugin_config']['remove_input_padding'],
                               paged_kv_cache=bool(config['plugin_config'].get('paged_kv_cache', False)),
                               tokens_per_block=int(config['plugin_config'].get('tokens_per_block', 64)),
                               num_kv_heads=bc.get('num_kv_heads', bc['num_heads']) // world_size,
                               lora_max_rank=int(bc.get('lora_max_rank') or 0), lora_target_modules=bc.get('lora_target_modules'))
    path = Path(engine_dir) / get_engine_name('llama', dtype, world_size, runtime_rank)
    with open(path, 'rb') as f:
        engine_buffer = f.read()
    return GenerationSession(model_config, engine_buffer, mapping), runtime_rank


def generate(max_output_len, log_level='error', engine_dir='llama_outputs', input_text=None, input_file=None,
             output_csv=None, output_npy=None, tokenizer_dir=None, num_beams=1, num_runs=55, top_k=1, top_p=0.0,
             temperature=1.0, repetition_penalty=1.0, random_seed=None, prompt_lookup_tokens=0, prompt_lookup_ngram=3,
             prompt_lookup_sampling=False, lora_dir=None, lora_slots=None):
    tensorrt_llm.logger.set_level(log_level)
    decoder, runtime_rank = load_session(engine_dir)
    for slot, d in enumerate(lora_dir or []):
        decoder.load_lora(d, slot)
    if isinstance(lora_slots, str):
        lora_slots = [int(v) for v in lora_slots.split(',')]
    if lora_slots is None and lora_dir:
        lora_slots = [0]  # one prompt per run
    sampling_config = SamplingConfig(end_id=EOS_TOKEN, pad_id=PAD_TOKEN, num_beams=num_beams, top_k=top_k, top_p=top_p,
                                     temperature=temperature, repetition_penalty=repetition_penalty)
    sampling_config.random_seed = random_seed
    tokenizer = None
    if input_file is None:
        from transformers import LlamaTokenizer
        tokenizer = LlamaTokenizer.from_pretrained(tokenizer_dir, legacy=False)
    total = []
    output_ids = None
    for _ in range(num_runs):
        tensorrt_llm.profiler.reset()
        tensorrt_llm.profiler.start('llama-run')
        if input_file is None:
            ids = np.array([tokenizer.encode(input_text, add_special_tokens=False)], dtype=np.int32)
        elif input_file.endswith('.csv'):
            with open(input_file) as f:
                ids = np.array([[int(v) for v in next(csv.reader(f))]], dtype=np.int32)
        else:
            ids = np.load(input_file).astype(np.int32).reshape(1, -1)
        input_lengths = np.array([ids.shape[1]], dtype=np.int32)
        if prompt_lookup_tokens:
            # the last verify pass writes prompt_lookup_tokens cache rows from the current length: that much room behind the output
            decoder.setup(ids.shape[0], int(input_lengths.max()), max_output_len + prompt_lookup_tokens)
            output_ids = decoder.decode_lookup(ids, input_lengths, sampling_config, num_draft_tokens=prompt_lookup_tokens,
                                               max_ngram=prompt_lookup_ngram, max_new_tokens=max_output_len,
                                               speculative_sampling=prompt_lookup_sampling, lora_slots=lora_slots)
            output_ids = output_ids[:, :, :ids.shape[1] + max_output_len]
        else:
            decoder.setup(ids.shape[0], int(input_lengths.max()), max_output_len)
            output_ids = decoder.decode(ids, input_lengths, sampling_config, lora_slots=lora_slots)
        if tokenizer is not None and runtime_rank == 0:
            outputs = output_ids[0, 0, ids.shape[1]:].tolist()
            tokenizer.decode(outputs)
        tensorrt_llm.profiler.stop('llama-run')
        total.append(tensorrt_llm.profiler.elapsed_time_in_sec('llama-run'))
    if runtime_rank == 0:
        out = np.asarray(output_ids)[0]
        if tokenizer is not None:
            print(f'Input: "{input_text}"')
            for b in range(out.shape[0]):
                print(f'Output: "{tokenizer.decode(out[b, ids.shape[1]:].tolist())}"')
        if output_csv is not None:
            with open(output_csv, 'w') as f:
                csv.writer(f, delimiter=',').writerows(out.tolist())
        if output_npy is not None:
            np.save(output_npy, out.astype(np.int32))
        print(total)
        if prompt_lookup_tokens:
            print(f'prompt lookup: {decoder.lookup_stats}')
        warm = total[5:] if len(total) > 5 else total
        print(f'llama-run (mean latency: {np.mean(warm)} sec)')
    return output_ids


if __name__ == '__main__':
    args = parse_arguments()
    generate(**vars(args))
