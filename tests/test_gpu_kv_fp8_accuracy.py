"""The accuracy criterion of tests/test_gpu_trained_accuracy.py for the fp8 (OCP E4M3) KV cache, on the same trained parent and
through the same command-line flow

    hf_llama_convert.py -> build.py --fp8_kv_cache -> summarize.py --check_accuracy --rougeL_delta_threshold 1

once UNCALIBRATED (the converted directory holds no KV scale: kv_orig_quant = kv_quant_orig = 1.0 - what the cache type is
for) and once with the calibrated scale of hf_llama_convert.py --calibrate-kv-cache.  Criterion: |ROUGE-L(engine vs highlights) -
ROUGE-L(HF vs highlights)| <= 1, the project's own."""
import concurrent.futures
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_trained_accuracy import EX, FIX, build, load_eval, summarize_cmd

RUNS = {'fp8_kv_uncalibrated': False, 'fp8_kv_calibrated': True}


@pytest.fixture(scope='module')
def rouge_runs(tmp_path_factory):
    base = tmp_path_factory.mktemp('trained_fp8')
    e = load_eval()
    np.save(base / 'calib.npy', e['calib'])
    for k, f in (('prompts', 'prompts'), ('lengths', 'lengths'), ('reference', 'reference'), ('hf_tokens', 'hf_tokens')):
        np.save(base / f'{f}.npy', e[k])

    def run(item):
        name, calibrated = item
        try:
            d = base / f'ft_{name}'
            cmd = [sys.executable, os.path.join(EX, 'hf_llama_convert.py'), '-i', FIX, '-o', str(d)]
            if calibrated:
                cmd += ['--calibrate-kv-cache', '--calib-ids', str(base / 'calib.npy')]
            r = subprocess.run(cmd, cwd=EX, timeout=900, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-3000:]
            ft = d / '1-gpu'
            has_scale = any(ft.glob('*attention.query_key_value.scale_y_quant_orig.bin'))
            assert has_scale == calibrated, 'the uncalibrated run must find no KV scale, the calibrated one must'
            eng = build(base, str(ft), name, ['--fp8_kv_cache'])
            assert b'quant_mode=64' in open(eng / 'llama_float16_tp1_rank0.engine', 'rb').read(4096)
            out = base / f'rouge_{name}.json'
            r = subprocess.run(summarize_cmd(base, eng, out, live_hf=False), cwd=EX, timeout=1800, capture_output=True, text=True)
            return name, (r.returncode, r.stderr[-3000:], json.load(open(out)) if out.exists() else None)
        except BaseException as ex:
            return name, (-1, repr(ex), None)

    with concurrent.futures.ThreadPoolExecutor(len(RUNS)) as ex:
        return dict(ex.map(run, RUNS.items()))


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(RUNS))
def test_rouge_l_delta_vs_hf_within_one(rouge_runs, name):
    rc, err, res = rouge_runs[name]
    print(f'[trained parent, {name}] ' + (json.dumps({k: res[k] for k in ('rougeL_delta_vs_hf', 'token_match_rate')}
                                                     | {'rougeL': res['tensorrt_llm']['rougeL'], 'hf_rougeL': res['hf']['rougeL']})
                                          if res else err))
    assert rc == 0, err
    assert abs(res['rougeL_delta_vs_hf']) <= 1.0, res
