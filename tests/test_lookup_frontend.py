"""What GenerationSession.decode_lookup / verify and run.py refuse before anything reaches the device, and the exported symbols of
speculative greedy decoding.  No GPU needed."""
import os
import re
import sys

import numpy as np
import pytest

from tensorrt_llm.runtime import GenerationSession, SamplingConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def session():
    gs = GenerationSession.__new__(GenerationSession)
    gs.batch_size, gs.max_input_length, gs.max_new_tokens, gs.beam_width = 2, 8, 24, 1
    gs.runtime = None  # nothing may reach the device
    return gs


def test_decode_lookup_refuses_beams_and_sampling():
    gs = session()
    ids, lens = np.zeros((2, 8), np.int32), np.array([8, 3], np.int32)
    with pytest.raises(ValueError, match='num_beams 1'):
        gs.decode_lookup(ids, lens, SamplingConfig(end_id=2, pad_id=0, num_beams=2))
    with pytest.raises(NotImplementedError, match='speculative sampling is not built'):
        gs.decode_lookup(ids, lens, SamplingConfig(end_id=2, pad_id=0, top_k=40))
    for field in (dict(temperature=0.7), dict(repetition_penalty=1.2), dict(presence_penalty=0.5), dict(min_length=4)):
        with pytest.raises(NotImplementedError, match='arg-max'):
            gs.decode_lookup(ids, lens, SamplingConfig(end_id=2, pad_id=0, **field))
    greedy = SamplingConfig(end_id=2, pad_id=0)
    for n, g in ((1, 3), (33, 3), (8, 0), (8, 9)):
        with pytest.raises(ValueError, match='num_draft_tokens'):
            gs.decode_lookup(ids, lens, greedy, num_draft_tokens=n, max_ngram=g)
    with pytest.raises(ValueError, match='max_new_tokens'):  # 17 + 8 > 24: no room for the last verify pass
        gs.decode_lookup(ids, lens, greedy, max_new_tokens=17)
    gs.beam_width = 2
    with pytest.raises(ValueError, match='beam_width 1'):
        gs.decode_lookup(ids, lens, greedy)


def test_run_py_takes_the_prompt_lookup_flags():
    sys.path.insert(0, os.path.join(ROOT, 'trtllm-llama_amd', 'examples', 'llama_quant'))
    import run
    a = run.parse_arguments(['--max_output_len', '8'])
    assert a.prompt_lookup_tokens == 0 and a.prompt_lookup_ngram == 3
    a = run.parse_arguments(['--max_output_len', '8', '--prompt_lookup_tokens', '8', '--prompt_lookup_ngram', '2'])
    assert (a.prompt_lookup_tokens, a.prompt_lookup_ngram) == (8, 2)


def test_library_exports_the_speculative_symbols():
    from tensorrt_llm.plugin import capi
    from tensorrt_llm.runtime import native
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'tllm_runtime_api.h')).read(), flags=re.S)
    lib = capi.load_library()
    for name in ('tllm_session_verify', 'tllm_session_verify_top1', 'tllm_session_generate_lookup', 'tllm_spec_accept',
                 'tllm_prompt_lookup'):
        assert re.search(r'\b' + name + r'\s*\(', text), f'{name} is not declared'
        assert hasattr(lib, name), f'{name} is declared but not exported'
    assert int(re.search(r'#define\s+TLLM_VERIFY_MAX_TOKENS\s+(\d+)', text).group(1)) == native.VERIFY_MAX_TOKENS == 32
