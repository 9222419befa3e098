"""bench.py's plain run (no --full): the headline keys only, and --dump-outputs writes what the timed path's last step hands its
caller (fp32 logits, the token record as float64)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_bench_plain_run_dumps_outputs(tmp_path):
    K, W, ctx = 4, 1, 1024
    out = tmp_path / 'outputs'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(K), '--warmup', str(W),
                        '--layers', '2', '--context', str(ctx), '--dump-outputs', str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert k in d, k
    assert d['steps'] == K and d['value'] > 0 and d['ms_per_step'] > 0 and d['step']['outputs_finite']
    assert abs(d['value'] * d['ms_per_step'] - 1e3) < 1e-6 * d['value'] * d['ms_per_step']
    for k in ('roofline', 'cpu_baseline', 'parity', 'prefill', 'fp16_tokens_per_s', 'tp_rank_prediction'):  # --full only
        assert k not in d, k
    logits, ids = np.load(out / 'logits.npy'), np.load(out / 'output_ids.npy')
    assert logits.dtype == np.float32 and logits.shape == (1, 32000) and np.isfinite(logits).all()
    # the record holds the prompt slots and the new tokens of a session set up for 2 K + W + 4 of them (bench.run_config)
    assert ids.dtype == np.float64 and ids.shape == (1, ctx + 2 * K + W + 4)
    assert (ids[0, :ctx] == 3).all()  # the synthetic prompt (tllm_session_fake_context)
    assert ((ids >= 0) & (ids < 32000) & (ids == np.round(ids))).all()
