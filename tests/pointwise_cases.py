"""The case table of the row-wise and element-wise kernels (kernels/pointwise.hip) - importable without a GPU.

launch_rmsnorm picks one of five kernels; tllm_rmsnorm_kernel (the launcher's own rule, host only) names it as
    1 = rmsnorm_kernel<1>   scalar, row in LDS: any N, any fp16 alignment
    2 = rmsnorm_kernel<8>   16-byte accesses, row in LDS: N % 8 == 0, aligned pointers; LayerNorm, or N > 8192
    3 + 8 NV = rmsnorm_reg_kernel<NV>   row in registers, RMSNorm only: NV = 1 (N <= 2048), 2 (<= 4096), 4 (<= 8192)
    0 = empty problem, -1 = refused.
tests/test_pointwise_instance_table.py holds every RMSNorm case against that rule and the constants below against the source
text; tests/test_gpu_pointwise_instances.py runs every case against oracle/pointwise_oracle.py."""
import zlib
from collections import namedtuple

import numpy as np

# pointwise.hip (held against the source text by test_pointwise_instance_table.py)
GRID_CAP, BLOCK = 2048, 256            # grid_for(): at most 2048 workgroups of 256 threads; a larger n takes grid-stride trips
REG_N = (2048, 4096, 8192)             # the register kernel's NV = 1 / 2 / 4 bounds
LDS_BYTES, LDS_HEAD = 64 * 1024, 128   # both LDS kernels: 128 + 2 N <= 64 KiB
N_MAX = (LDS_BYTES - LDS_HEAD) // 2    # 32704
SECOND_TRIP_VEC8 = GRID_CAP * BLOCK * 8  # 4 194 304 halfs
SECOND_TRIP_VEC1 = GRID_CAP * BLOCK      # 524 288 elements
DT_FLOAT, DT_HALF, DT_INT8, DT_INT32, DT_FP8 = 0, 1, 2, 3, 6

K_LDS1, K_LDS8, K_REG = 1, 2, 3
REG1, REG2, REG4 = 3 + 8 * 1, 3 + 8 * 2, 3 + 8 * 4
KERNEL_NAME = {0: 'empty', -1: 'refused', 1: 'lds<1>', 2: 'lds<8>', REG1: 'reg<1>', REG2: 'reg<2>', REG4: 'reg<4>'}
OUTS = ('y', 'qs', 'qd', 'yqs', 'yqd')  # y; q static; q dynamic; y + q static; y + q dynamic

_R = dict(name='', N=0, M=3,
          kernel=0,        # the `kernel` argument of tllm_rmsnorm (0 = the launcher's choice)
          expect=0,        # what runs: tllm_rmsnorm_kernel's value (kernel = 0), or the forced kernel
          outs=('y', 'qs', 'qd'),
          ln=0, diff_sq=1,  # LayerNorm flavour (x mean 0.5, beta set)
          residual=0,      # residual + sum_out (a buffer of its own)
          x_off=0,         # x viewed from an offset of this many fp16 elements
          q_off=0,         # q viewed from an offset of this many bytes
          drop='')         # a refusal case leaves this out: 'sum_out', 'scale', 'beta'
RCase = namedtuple('RCase', list(_R), defaults=list(_R.values()))


def rule(N, M=3, ln=0, aligned=True, kernel=0):
    """Python mirror of rmsnorm_kernel_for() for a complete argument set (nothing dropped)"""
    if M <= 0 or N <= 0:
        return 0
    if LDS_HEAD + 2 * N > LDS_BYTES:
        return -1
    vec = N % 8 == 0 and aligned
    reg = vec and not ln and 8 <= N <= REG_N[2]
    if kernel in (K_LDS8, K_REG) and not vec:
        return -1
    if kernel == K_REG and not reg:
        return -1
    if kernel == K_LDS1 or (kernel == 0 and not vec):
        return 1
    if kernel == K_LDS8 or not reg:
        return 2
    return REG1 if N <= REG_N[0] else (REG2 if N <= REG_N[1] else REG4)


def _rms_cases():
    cs = []
    both = ('yqs', 'yqd')
    # the register kernel by dispatch, and rmsnorm_kernel<8> forced on the same rows; y + q at one N per kernel
    for n in (8, 64, 2040, 2048, 2056, 4096, 4104, 5120, 6152, 8192):
        extra = both if n in (64, 4096, 5120) else ()
        cs.append(RCase('reg', n, expect=rule(n), outs=OUTS[:3] + extra))
        cs.append(RCase('lds8-forced', n, kernel=K_LDS8, expect=2, outs=OUTS[:3] + (both if n == 4096 else ())))
    # rmsnorm_kernel<8> by dispatch: N > 8192 up to the LDS limit, and LayerNorm
    cs.append(RCase('lds8', 8200, expect=2))
    cs.append(RCase('lds8', 11008, expect=2, outs=OUTS))
    cs.append(RCase('lds8', N_MAX, M=1, expect=2))
    # rmsnorm_kernel<1>: N % 8 != 0 (one element, less than a vector, several elements per thread), or a pointer off 16 bytes
    for n in (1, 7, 100, 257, 4097):
        cs.append(RCase('lds1', n, expect=1, outs=OUTS if n == 257 else OUTS[:3]))
    cs.append(RCase('lds1-xoff', 4096, expect=1, x_off=1))
    cs.append(RCase('lds1-qoff', 4096, expect=1, q_off=4, outs=('qs', 'qd', 'yqd')))
    # residual + sum_out: one N per kernel
    for n in (64, 4096, 5120, 11008, 257):
        cs.append(RCase('residual', n, expect=rule(n), outs=('y', 'yqd'), residual=1))
    for n in (64, 4096, 5120):
        cs.append(RCase('residual-lds8-forced', n, kernel=K_LDS8, expect=2, outs=('y', 'yqd'), residual=1))
    # LayerNorm, both variance forms, on the LDS kernels
    for n in (8, 100, 768, 4096):
        for d in (0, 1):
            cs.append(RCase('layernorm', n, expect=rule(n, ln=1), outs=OUTS, ln=1, diff_sq=d))
    # refusals: nothing is launched, no buffer byte changes
    cs.append(RCase('refuse-lds-limit', N_MAX + 8, M=1, expect=-1, outs=('y', )))
    cs.append(RCase('refuse-residual-without-sum_out', 64, expect=-1, outs=('y', ), residual=1, drop='sum_out'))
    cs.append(RCase('refuse-q-without-scale', 64, expect=-1, outs=('qs', ), drop='scale'))
    cs.append(RCase('refuse-layernorm-without-beta', 768, expect=-1, outs=('yqs', ), ln=1, drop='beta'))
    cs.append(RCase('refuse-forced-lds8-odd-N', 100, kernel=K_LDS8, expect=-1, outs=('y', )))
    cs.append(RCase('refuse-forced-lds8-xoff', 4096, kernel=K_LDS8, expect=-1, outs=('y', ), x_off=1))
    cs.append(RCase('refuse-forced-reg-qoff', 4096, kernel=K_REG, expect=-1, outs=('qs', ), q_off=4))
    cs.append(RCase('refuse-forced-reg-N', 8200, kernel=K_REG, expect=-1, outs=('y', )))
    cs.append(RCase('refuse-forced-reg-layernorm', 768, kernel=K_REG, expect=-1, outs=('yqs', ), ln=1))
    cs.append(RCase('empty', 64, M=0, expect=0, outs=('y', )))
    return cs


RMS_CASES = _rms_cases()


def rms_id(c):
    s = f'{c.name}-N{c.N}-M{c.M}'
    if c.ln:
        s += f'-ln{c.diff_sq}'
    return s


def crc(s):
    return zlib.crc32(s.encode())


def rms_inputs(c):
    """numpy operands of an RMSNorm / LayerNorm case, seeded by its id.  Row 0 zeros (eps, the f16(1e-6) amax floor), row 1
    ~1.7 N(0, 1), row 2 values of that size x 2^-10 - a mixed-up row shows; LayerNorm: + 0.5 on rows 1 and 2 (row 2 before its
    scaling); gamma in [0.5, 1.5]."""
    r = np.random.default_rng(crc(rms_id(c)))
    M, N = max(c.M, 1), c.N
    x = np.zeros((M, N), np.float64)
    for m in range(1, M):
        x[m] = 1.7 * r.standard_normal(N) + (0.5 if c.ln else 0.0)
    if M > 2:
        x[2] *= 2.0 ** -10
    d = dict(x=x.astype(np.float16), gamma=r.uniform(0.5, 1.5, N).astype(np.float16))
    d['beta'] = (0.1 * r.standard_normal(N)).astype(np.float16)
    res = r.standard_normal((M, N))
    if M > 2:
        res[2] *= 2.0 ** -10
    d['residual'] = res.astype(np.float16)
    d['scale'] = np.float32(23.5)
    d['eps'] = np.float32(1e-5 if c.ln else 1e-6)
    return d


def within_ulp16(got, ref, ulps=2):
    """Stage A of the instance sweeps: `got` (fp16 values) within `ulps` fp16 ulp of the oracle's `ref` (the spacing at the
    oracle's value), at most max(2, 1 %) of the elements differing at all.  Non-finite values must agree in kind and sign.
    Returns (worst error in ulp, number of differing elements, the cap on that number); asserts nothing."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    fin = np.isfinite(ref)
    same_kind = np.where(fin, np.isfinite(got), (np.isnan(ref) & np.isnan(got)) | (got == ref))
    with np.errstate(invalid='ignore'):
        err = np.where(fin & np.isfinite(got), np.abs(got - ref), 0.0) / (2.0 ** (np.floor(np.log2(np.maximum(np.abs(np.where(fin, ref, 1.0)), 2.0 ** -14))) - 10))
    err = np.where(same_kind, err, np.inf)
    differ = int((err != 0).sum())
    return float(err.max()) if err.size else 0.0, differ, max(2, got.size // 100)


# ---------------------------------------------------------------------------------------------- element-wise
# op: 'swiglu' | 'swiglu_quant' | 'add'; off: which operand is viewed from an offset of one element ('' none)
ECase = namedtuple('ECase', 'op n off inplace', defaults=('', 0))
EW_N = (8, 2048 * 8, 33024, SECOND_TRIP_VEC8 + 24, SECOND_TRIP_VEC1 + 3, 13)


def _ew_cases():
    cs = []
    for op in ('swiglu', 'swiglu_quant', 'add'):
        for n in EW_N:
            cs.append(ECase(op, n))
        cs.append(ECase(op, 4096, off='a'))
        cs.append(ECase(op, 4096, off='b'))
        cs.append(ECase(op, 4096, off='y'))  # (swiglu_quant: q from an offset of 4 bytes)
    cs.append(ECase('add', 33024, inplace=1))
    cs.append(ECase('add', 13, inplace=1))
    cs.append(ECase('add', SECOND_TRIP_VEC8 + 24, inplace=1))
    return cs


EW_CASES = _ew_cases()


def ew_id(c):
    return f'{c.op}-n{c.n}' + (f'-off_{c.off}' if c.off else '') + ('-inplace' if c.inplace else '')


def ew_vec(c):
    """the VEC the launcher picks"""
    return 8 if c.n % 8 == 0 and not c.off else 1


PIN_G = [0.0, -0.0, 65504.0, -65504.0, -20.0, 20.0, 2.0 ** -24, np.nan]


def ew_inputs(n, seed):
    """a ~ 3 N(0, 1), b ~ N(0, 1); the first 16 elements (as many as fit) pin a to PIN_G twice, against b = 1 and b = -0.75;
    for add, element 16 and 17 hold 60000 + 60000 and -60000 - 60000 (-> +-inf)"""
    r = np.random.default_rng(seed)
    a = (3.0 * r.standard_normal(n)).astype(np.float16)
    b = r.standard_normal(n).astype(np.float16)
    pa = np.array(PIN_G + PIN_G, np.float16)
    pb = np.array([1.0] * 8 + [-0.75] * 8, np.float16)
    k = min(n, 16)
    a[:k], b[:k] = pa[:k], pb[:k]
    if n >= 18:
        a[16:18] = [60000.0, -60000.0]
        b[16:18] = [60000.0, -60000.0]
    return a, b


QT_N = SECOND_TRIP_VEC1 + 5     # quantize_tensor, fill_i32, fill_random: the second grid-stride trip and a ragged end
EMB_CASES = [(5, 8, 11, 0), (5, 4096, 11, 0), (3, 2056, 7, 0), (4, 100, 9, 0), (4, 264, 9, 0),
             (5, 4096, 11, 1)]  # (tokens, hidden, vocab, table viewed from an offset of this many elements)


def emb_ids(tokens, vocab):
    ids = [0, vocab - 1, -1, vocab, 2 ** 31 - 1, 1, vocab // 2]
    return np.array(ids[:tokens], np.int32)


GLT_CASES = [(4, 5, 8), (4, 5, 300), (2, 3, 4096)]  # (batch, seq, hs)


def glt_ids(batch, seq, hs):
    """last_token_ids drawn from {0, 1, seq, seq + 5, -3}: all five over the three cases"""
    ids = {8: [0, 1, seq, seq + 5], 300: [-3, seq + 5, 1, seq], 4096: [-3, seq]}[hs]
    assert len(ids) == batch
    return np.array(ids, np.int32)


GR_CASES = [8, 300, 4096]     # hs; 6 source rows, 7 gathered
GR_ROWS = np.array([5, 0, 3, 3, 1, 5, 0], np.int32)
SCAN_N = [0, 1, 64, 65, 300]
FILL_DTYPES = (DT_HALF, DT_FLOAT, DT_INT8, DT_FP8)
