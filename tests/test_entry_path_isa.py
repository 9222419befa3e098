"""The entry contract of the decode step's kernels, held against their gfx950 assembly - no GPU needed, only
hipcc: tools/entry_path_report.py compiles the decode translation units with the flags csrc/Makefile gives them and reads, for the
SmoothQuant instances a generation step launches (bench.py step_launches names them),

  * the kernarg preload length of the kernel descriptor: the leading parameters really are preloaded (a by-value struct alone
    gives 0), and
  * the s_waitcnt instructions naming lgkmcnt between the preloaded entry and the first weight load (the sampler: its first logits
    load): none - the stream starts without a scalar round trip to the kernarg segment or to a device word.

Before the contract these were 0 dwords and 1 / 1 / 8 waits (gate|up and head / down / front), profiles/entry_path.txt."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import entry_path_report as EP  # noqa: E402

pytestmark = pytest.mark.skipif(EP.hipcc() is None, reason='needs hipcc')

KERNELS = {'front': 'qkv_attn_fused_kernel<3, true, 0>', 'gate_up': 'gemv_kernel<3, 1, 1, 1, 2, 4>', 'down': 'gemv_ksplit_kernel<3, 3>',
           'head': 'gemv_kernel<0, 1, 0, 1, 2, 4>', 'sampler': 'greedy_step_kernel'}


@pytest.fixture(scope='module')
def rows():
    got = {r['key']: r for r in EP.report()}
    for r in got.values():
        print('%-8s %-36s preload %2d dwords, %d scalar waits before the %s load at instruction %d (first vector load at %d)'
              % (r['key'], r['kernel'], r['preload'], r['waits'], r['kind'], r['pos'], r['first']))
    return got


def test_the_report_covers_the_steps_launches(rows):
    assert {k: r['kernel'] for k, r in rows.items()} == KERNELS
    import bench
    names = [ln['kernel'] for ln in bench.step_launches(bench.LLAMA_7B, 'sq', 1, 3, 1024.0, 1, 1156)]
    for key in ('front', 'gate_up', 'down'):
        assert KERNELS[key] in names, (key, names)
    assert any(n.startswith('gemv_kernel<0, 1, 0') for n in names)  # the head GEMV, named by its family there


@pytest.mark.parametrize('key', list(KERNELS))
def test_leading_parameters_are_preloaded(rows, key):
    assert 0 < rows[key]['preload'] <= 14, rows[key]


@pytest.mark.parametrize('key', list(KERNELS))
def test_no_scalar_wait_precedes_the_first_loads(rows, key):
    r = rows[key]
    assert r['kind'] == ('first' if key == 'sampler' else 'weight'), r
    assert r['waits'] <= 0 and r['waits_first'] <= 0, r
    assert r['first'] <= r['pos']
