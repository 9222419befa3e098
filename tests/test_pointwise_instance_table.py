"""No GPU: the case table of tests/test_gpu_pointwise_instances.py (tests/pointwise_cases.py) against the dispatch of
launch_rmsnorm as the library states it - tllm_rmsnorm_kernel is the launcher's own rule, host only, so every RMSNorm case is
asked of it on fake pointers with the case's alignments.  Every value that rule can return must have a case, and the constants
the table relies on (the grid cap of the grid-stride kernels, the register kernel's bounds, the LDS limit) are read from
pointwise.hip and fail here when they move."""
import ctypes
import os
import re

import pytest

import pointwise_cases as PC
from helpers import RmsnormParams
from tensorrt_llm.plugin import capi

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'trtllm-llama_amd', 'csrc', 'kernels', 'pointwise.hip')
BASE = 0x7f0000100000  # fake, 16-byte aligned; never followed


@pytest.fixture(scope='module')
def lib():
    lib = capi.load_library()
    lib.tllm_rmsnorm_kernel.argtypes = [ctypes.POINTER(RmsnormParams)]
    lib.tllm_rmsnorm_kernel.restype = ctypes.c_int32
    return lib


def fake_params(c, out):
    """the struct of case `c` asking for output combination `out`, every buffer 1 MiB apart"""
    at = lambda i: BASE + (i << 20)
    q = RmsnormParams()
    q.M, q.N, q.eps = c.M, c.N, 1e-6
    q.x = at(0) + 2 * c.x_off
    q.gamma = at(1)
    if c.residual:
        q.residual = at(2)
        q.sum_out = None if c.drop == 'sum_out' else at(3)
    if 'y' in out:
        q.y = at(4)
    if 'q' in out:
        q.q = at(5) + c.q_off
        if c.drop != 'scale':
            if out.endswith('s'):
                q.static_scale = at(6)
            else:
                q.dyn_scale_out = at(7)
    q.layernorm, q.use_diff_of_squares = c.ln, c.diff_sq
    if c.ln and c.drop != 'beta':
        q.beta = at(8)
    return q


def asked(lib, c, out):
    return lib.tllm_rmsnorm_kernel(ctypes.byref(fake_params(c, out)))


def test_the_constants_are_the_sources():
    s = open(SRC).read()
    g = s[s.index('inline int grid_for(int64_t n)'):]
    g = g[:g.index('\n}\n')]
    assert f'int64_t b = (n + {PC.BLOCK - 1}) / {PC.BLOCK};' in g
    assert f'(b > {PC.GRID_CAP} ? {PC.GRID_CAP} : b)' in g
    # every grid-stride kernel is launched with grid_for(..) workgroups of 256 threads
    launches = re.findall(r'hipLaunchKernelGGL\((\w+)(?:<[^>]*>)?, dim3\(grid_for\(([^)]*)\)\), dim3\((\d+)\)', s)
    assert {k for k, _, _ in launches} == {'quantize_tensor_kernel', 'swiglu_kernel', 'swiglu_quant_kernel', 'add_kernel',
                                           'fill_random_kernel', 'fill_i32_kernel'}
    assert {b for _, _, b in launches} == {str(PC.BLOCK)}
    assert {(k, n) for k, n, _ in launches if k in ('swiglu_kernel', 'swiglu_quant_kernel', 'add_kernel')} \
        == {(k, n) for k in ('swiglu_kernel', 'swiglu_quant_kernel', 'add_kernel') for n in ('n / 8', 'n')}
    assert PC.SECOND_TRIP_VEC8 == 4194304 and PC.SECOND_TRIP_VEC1 == 524288
    r = s[s.index('int rmsnorm_kernel_for(const RmsnormParams& p, int kernel)'):]
    r = r[:r.index('\n}\n')]
    assert 'const size_t smem = 128 + (size_t) p.N * 2;' in r and 'if (smem > 64 * 1024)' in r
    assert PC.LDS_HEAD == 128 and PC.LDS_BYTES == 64 * 1024 and PC.N_MAX == 32704
    assert 'const bool reg = vec && !p.layernorm && p.N >= 8 && p.N <= 2048 * 4;' in r
    assert 'return 3 + 8 * (p.N <= 2048 ? 1 : (p.N <= 4096 ? 2 : 4));' in r
    assert PC.REG_N == (2048, 4096, 2048 * 4)
    # one dispatch rule: the launcher launches what that function names
    la = s[s.index('int launch_rmsnorm_kernel(const RmsnormParams& p, int kernel, hipStream_t stream)'):]
    la = la[:la.index('\n}\n')]
    assert 'const int k = rmsnorm_kernel_for(p, kernel);' in la
    lr = s[s.index('int launch_rmsnorm(const RmsnormParams& p, hipStream_t stream)'):]
    assert 'return launch_rmsnorm_kernel(p, 0, stream);' in lr[:lr.index('\n}\n')]


@pytest.mark.parametrize('c', PC.RMS_CASES, ids=PC.rms_id)
def test_every_rmsnorm_case_reaches_the_kernel_it_names(c, lib):
    aligned = not c.x_off and not (c.q_off and any('q' in o for o in c.outs))
    for out in c.outs:
        got = asked(lib, c, out)
        if c.kernel == 0:
            assert got == c.expect, (out, PC.KERNEL_NAME.get(got, got), capi.last_error())
            if c.expect == -1:
                assert capi.last_error()
        else:
            # a forced case: the arguments themselves are complete, the launcher's own choice is what the mirror says
            assert not c.drop and got == PC.rule(c.N, c.M, c.ln, aligned) and got > 0
    # the Python mirror says the same for complete argument sets (the forced kernel included)
    if not c.drop:
        assert PC.rule(c.N, c.M, c.ln, aligned, c.kernel) == c.expect, c


def covered(cases):
    return {c.expect for c in cases if c.kernel == 0}


def test_every_value_the_rule_returns_has_a_case():
    want = {0, -1, PC.K_LDS1, PC.K_LDS8, PC.REG1, PC.REG2, PC.REG4}
    assert covered(PC.RMS_CASES) == want
    # forced: rmsnorm_kernel<8> on every register-kernel row, and every forced refusal
    reg_n = {c.N for c in PC.RMS_CASES if c.kernel == 0 and c.expect in (PC.REG1, PC.REG2, PC.REG4) and not c.residual}
    assert reg_n == {8, 64, 2040, 2048, 2056, 4096, 4104, 5120, 6152, 8192}
    assert {c.N for c in PC.RMS_CASES if c.kernel == PC.K_LDS8 and c.expect == 2 and not c.residual} == reg_n
    assert {c.drop for c in PC.RMS_CASES if c.expect == -1} >= {'sum_out', 'scale', 'beta'}
    assert any(c.expect == -1 and c.N == PC.N_MAX + 8 for c in PC.RMS_CASES) and any(c.expect == 2 and c.N == PC.N_MAX for c in PC.RMS_CASES)
    ids = [PC.rms_id(c) for c in PC.RMS_CASES]
    assert len(ids) == len(set(ids))
    # a partly populated last vector slot for every NV, and both sides of each bound
    for k, ns in ((PC.REG1, {2040, 2048}), (PC.REG2, {2056, 4096}), (PC.REG4, {4104, 5120, 6152, 8192})):
        assert {c.N for c in PC.RMS_CASES if c.kernel == 0 and c.expect == k} >= ns
    # every output combination on every kernel, the residual on every kernel, both LayerNorm variance forms on both LDS kernels
    for k in (PC.K_LDS1, PC.K_LDS8, PC.REG1, PC.REG2, PC.REG4):
        mine = [c for c in PC.RMS_CASES if c.expect == k]
        assert {o for c in mine for o in c.outs} == set(PC.OUTS), k
        assert any(c.residual for c in mine), k
    for k in (PC.K_LDS1, PC.K_LDS8):
        assert {c.diff_sq for c in PC.RMS_CASES if c.ln and c.expect == k} == {0, 1}


def test_deleting_the_sole_case_of_a_kernel_fails_the_table():
    for k in (0, PC.REG1, PC.REG2, PC.REG4, PC.K_LDS1, PC.K_LDS8, -1):
        without = [c for c in PC.RMS_CASES if not (c.kernel == 0 and c.expect == k)]
        assert k not in covered(without)


def test_the_elementwise_table_holds_the_edges():
    for op in ('swiglu', 'swiglu_quant', 'add'):
        mine = [c for c in PC.EW_CASES if c.op == op]
        ns = {c.n for c in mine}
        assert ns >= {8, 2048 * 8, 33024, 4194304 + 24, 524288 + 3, 13, 4096}
        # the second trip of the grid-stride loop in both forms, and VEC = 1 by size and by each pointer
        assert any(PC.ew_vec(c) == 8 and c.n > PC.SECOND_TRIP_VEC8 for c in mine)
        assert any(PC.ew_vec(c) == 1 and c.n > PC.SECOND_TRIP_VEC1 for c in mine)
        assert {c.off for c in mine if PC.ew_vec(c) == 1} >= {'', 'a', 'b', 'y'}
    assert any(c.op == 'add' and c.inplace for c in PC.EW_CASES)
    assert PC.QT_N > PC.SECOND_TRIP_VEC1 and PC.QT_N % 8
    assert {(t, h, v) for t, h, v, o in PC.EMB_CASES} == {(5, 8, 11), (5, 4096, 11), (3, 2056, 7), (4, 100, 9), (4, 264, 9)}
    assert any(h == 4096 and o == 1 for _, h, _, o in PC.EMB_CASES)
    for t, h, v, o in PC.EMB_CASES:
        assert set(PC.emb_ids(t, v).tolist()) >= {0, v - 1, -1}
    assert any({v, 2 ** 31 - 1} <= set(PC.emb_ids(t, v).tolist()) for t, h, v, o in PC.EMB_CASES)
    seen = set()
    for b, s, hs in PC.GLT_CASES:
        seen |= {{s: 'seq', s + 5: 'seq+5'}.get(int(i), int(i)) for i in PC.glt_ids(b, s, hs)}
    assert seen == {0, 1, 'seq', 'seq+5', -3}
    assert len(set(PC.GR_ROWS.tolist())) < len(PC.GR_ROWS) and list(PC.GR_ROWS) != sorted(PC.GR_ROWS)
    assert PC.SCAN_N == [0, 1, 64, 65, 300]
