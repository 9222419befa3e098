"""The case table of the prefill GEMMs (kernels/gemm.hip launch_gemm and what it chooses among: gemm_glds.hip, gemm_sqp.hip,
gemm_woq.hip, gemm_mfma.hip, 8-row GEMV slabs) - importable without a GPU.

instance(case, cus) is a Python mirror of the host code, evaluated for a device with `cus` compute units:

    kernel > 0   tllm_gemm_kernel: exactly that kernel or a refusal
                   ('lockstep', wt, id)            gemm_glds.hip gemm_glds_kernel, ids 1..12, 36, 37
                   ('phased' | 'persist' | 'splitk', wt, id)   gemm_sqp.hip, SmoothQuant ids 15..65, fp16 ids 50..58
                   ('woq', wt, tile)               gemm_woq.hip, ids 101..106 -> tile 1..6
                   ('regstaged', wt)               gemm_mfma.hip, id REGISTER_STAGED
    kernel == 0  tllm_gemm / tllm_gemm_epi: (branch of the fall-back chain, the instance it ends in, the pointwise pass behind it)
    kernel == -1 tllm_gemm_swiglu_quant: ('dual', 'persist' | 'one')
    anything     ('refused', reason)

tests/test_gemm_instance_table.py holds the mirror's constants and conditions against the source text and checks, without a GPU,
that every kernel id a `case` label can launch and every branch of the chain has a case; tests/test_gpu_gemm_instances.py runs
every case against oracle/gemm_oracle.py.

Pointers are 256-byte aligned in the tests, so the mirror leaves the pointer-alignment terms of the conditions out.  The table is
evaluated at 256 CUs (TABLE_CUS); the GPU test evaluates the mirror at the device's own count.  What depends on the number: the
persistent cases named `*x2` / `*x3` (two / three tiles per workgroup only where tiles > CUs / 2 CUs), the split-K cases named
`*full` / `*two-per-cu` / `*1056-tiles` (2 x tiles against CUs x workgroups per CU) and the `static-*` cases (workgroup rounds)."""
from collections import namedtuple

from gemv_cases import (DT_FLOAT, DT_HALF, DT_INT8, DT_INT32, DT_NAME, W_FP16, W_INT4_WOQ, W_INT8_SQ, W_INT8_WOQ, WT_NAME, WTS,
                        round_up, row_bytes)

TABLE_CUS = 256
REGISTER_STAGED = 200  # TLLM_GEMM_KERNEL_REGISTER_STAGED
DUAL = -1
ABLATIONS = tuple(range(21, 28)) + (31, 32, 33)

# gemm_glds.hip launch_wt: id -> (WM, WN, MT, NT, KG, BKB, S, LW); BM = WM MT 32, BN = WN NT 32
GLDS = {1: (2, 2, 2, 2, 1, 64, 4, 0), 2: (2, 4, 4, 2, 1, 64, 4, 0), 3: (4, 2, 2, 3, 1, 64, 5, 0), 4: (2, 2, 2, 4, 1, 64, 4, 0),
        5: (2, 2, 2, 2, 1, 128, 2, 0), 6: (4, 2, 2, 3, 1, 128, 2, 0), 7: (2, 4, 2, 1, 1, 64, 4, 0), 8: (2, 2, 2, 2, 1, 128, 4, 0),
        9: (2, 2, 4, 3, 1, 128, 2, 0), 10: (2, 2, 4, 4, 1, 128, 2, 0), 11: (2, 2, 4, 3, 2, 128, 2, 0), 12: (2, 2, 2, 2, 2, 128, 2, 0),
        36: (4, 2, 2, 3, 1, 64, 5, 4), 37: (4, 2, 2, 3, 1, 128, 2, 4)}
NUM_CFG = 12
PHASED_256x128 = 42
# kShapes: (id, BM, BN, f fp16, f SmoothQuant)
SHAPES = ((8, 128, 128, 1.40, 1.80), (6, 256, 192, 1.0, 1.0), (2, 256, 256, 1.04, 1.30), (4, 128, 256, 1.39, 1.60),
          (PHASED_256x128, 256, 128, 1.08, 1.37))
# gemm_sqp.hip launch_gemm_sqp / launch_gemm_f16p: id -> (WR, WC, MTH, NTH, persistent, split-K); BM = 32 WR MTH, BN = 32 WC NTH
SQP = {15: (2, 2, 2, 2, 0, 0), 20: (4, 2, 2, 3, 0, 0), 18: (4, 2, 1, 2, 0, 0), 42: (4, 2, 2, 2, 0, 0), 60: (4, 2, 2, 3, 1, 0),
       62: (4, 2, 2, 2, 1, 0), 64: (4, 2, 2, 2, 0, 1), 65: (4, 2, 1, 2, 0, 1), 63: (4, 2, 2, 3, 1, 0)}
F16P = {50: (4, 2, 2, 3, 0, 0), 51: (4, 2, 1, 2, 0, 0), 52: (2, 2, 2, 2, 0, 0), 53: (4, 2, 2, 3, 0, 0), 54: (4, 2, 2, 2, 0, 0),
        55: (4, 2, 2, 3, 1, 0), 56: (4, 2, 2, 2, 1, 0), 57: (4, 2, 2, 2, 0, 1), 58: (4, 2, 1, 2, 0, 1)}
PERSIST_MIN_K = {W_INT8_SQ: 256, W_FP16: 128}
SPLITK_MIN_KTILES = 4
SPLITK_FLAG_BYTES = 8192
# workgroups per CU the split-K forms are built for (LDS: 97.5 KiB -> 1, 65 - 66.5 KiB -> 2; the launcher asks the occupancy
# query, which also counts registers: if it answers less, the `two-per-cu` cases are refused and the GPU test says so)
SPLITK_PER_CU = {64: 1, 57: 1, 65: 2, 58: 2}
# gemm_woq.hip launch_woq_bits: tile -> (WM, WN, MT, NT, S); the cost rule's candidates (tile, BM, BN, f int8, f int4)
WOQ = {1: (4, 2, 2, 3, 2), 2: (2, 2, 2, 2, 4), 3: (4, 2, 2, 3, 3), 4: (2, 2, 4, 3, 2), 5: (4, 2, 2, 2, 3), 6: (4, 2, 2, 2, 2)}
WOQ_CANDS = ((1, 256, 192, 1.0, 1.0), (6, 256, 128, 1.08, 1.08), (2, 128, 128, 1.28, 1.15))
# gemm_tactics.hip
SQ_CANDIDATES = (63, 20, 8, 62, 64, 65, 42, 6, 15, 18, 1, 3, 2, 4)
FP16_CANDIDATES = (55, 6, 8, 50, 56, 57, 58, 54, 51, 52, 53, 1, 3, 2, 4, 5, 7)
SQ_STATIC = (8, 2, 4, 63, 20, 62, 42)
FP16_STATIC = (8, 2, 4, 55, 50, 56, 54)

EPI_NONE, EPI_RES, EPI_GATE = 'none', 'res', 'gate'

_FIELDS = dict(name='', wt=0, M=0, N=0, K=0, out=DT_HALF, per_channel=1, per_token=1,
               kernel=0,       # tllm_gemm_kernel id; 0: tllm_gemm / tllm_gemm_epi; DUAL: tllm_gemm_swiglu_quant
               epi=EPI_NONE,   # 'res': fused residual, 'gate': fused SwiGLU gate
               strided=0,      # lda > K, ldw > row bytes, ldc > N (16-byte multiples); every padding byte 0xFF
               ldc_odd=0,      # ldc odd (the scalar epilogue's addressing)
               inplace=0,      # also run with residual == c: the bits must equal the out-of-place run
               force=0,        # tllm_gemm_set_tile_cfg before a dispatch call (-2 for the dual form: one tile per workgroup)
               table=0,        # a tactic-table entry naming this id for the case's shape before a dispatch call
               repeat=1)       # launches back to back on one stream (the split-K forms reuse flags and workspace)
Case = namedtuple('Case', list(_FIELDS), defaults=list(_FIELDS.values()))


def case_id(c):
    k = {0: 'dispatch', DUAL: 'dual', REGISTER_STAGED: 'regstaged'}.get(c.kernel, f'id{c.kernel}')
    return f'{c.name}-{k}-{WT_NAME[c.wt]}-{c.M}x{c.N}x{c.K}-{DT_NAME[c.out]}-{c.epi}'


def es_of(wt):
    return 1 if wt == W_INT8_SQ else 2


def strides(c):
    """(lda elements, ldw bytes, ldc elements)"""
    rb = row_bytes(c.wt, c.K)
    lda, ldw = (c.K + 16, rb + 32) if c.strided else (c.K, rb)
    if c.ldc_odd:
        ldc = c.N + 3 if c.N % 2 == 0 else c.N + 2
    else:
        ldc = round_up(c.N, 16) + 16 if c.strided else c.N
    return lda, ldw, ldc


def _cdiv(a, b):
    return (a + b - 1) // b


def glds_tile(i):
    wm, wn, mt, nt = GLDS[i][:4]
    return wm * mt * 32, wn * nt * 32


def sqp_tile(t):
    return 32 * t[0] * t[2], 32 * t[1] * t[3]


def woq_tile(i):
    wm, wn, mt, nt = WOQ[i][:4]
    return wm * mt * 32, wn * nt * 32


def _vec_rows_bad(c):
    """the vector epilogue's terms: fp16 output on 16-byte rows"""
    ldc = strides(c)[2]
    return c.out != DT_HALF or ldc & 7 or c.N & 7


# ---------------------------------------------------------------------------------------------- gemm_glds.hip
def glds_serves(c):
    sq = c.wt == W_INT8_SQ
    if not sq and c.wt != W_FP16:
        return False
    es = es_of(c.wt)
    lda, ldw, _ = strides(c)
    if (lda * es) & 15 or ldw & 15 or (c.K * es) % 128 or c.K <= 0 or c.M < 32:
        return False
    if not sq and c.out == DT_INT32:
        return False
    if c.epi == EPI_RES and _vec_rows_bad(c):
        return False
    if c.epi == EPI_GATE and (sq or _vec_rows_bad(c)):
        return False
    return True


def static_shape_cfg(c, cus, phased_ok=True):
    best, cfg = 1e30, 8
    for sid, bm, bn, f, f_sq in SHAPES:
        if sid == PHASED_256x128 and not phased_ok:
            continue
        tiles = _cdiv(c.M, bm) * _cdiv(c.N, bn)
        if sid == PHASED_256x128 and tiles > 2 * cus:
            continue
        cost = float(_cdiv(tiles, cus)) * bm * bn * (f_sq if c.wt == W_INT8_SQ else f)
        if cost < best:
            best, cfg = cost, sid
    return cfg


def static_cfg(c, cus):
    """gemm_static_cfg (tllm_gemm_static_cfg): no epilogue operands"""
    c = c._replace(epi=EPI_NONE)
    if not glds_serves(c):
        return 0
    cfg = static_shape_cfg(c, cus)
    sq = c.wt == W_INT8_SQ
    persist = not _vec_rows_bad(c) and c.K >= PERSIST_MIN_K[c.wt]
    if cfg == PHASED_256x128:
        return (62 if persist else 42) if sq else (56 if persist else 54)
    if cfg == 6:
        return (63 if persist else 20) if sq else (55 if persist else 50)
    return cfg


def persist_grid(tiles, cus):
    rounds = _cdiv(tiles, cus)
    return _cdiv(tiles, rounds)


def phased(c, cfg, cus):
    """launch_gemm_sqp / launch_gemm_f16p"""
    sq = c.wt == W_INT8_SQ
    table = SQP if sq else F16P
    es = es_of(c.wt)
    lda, ldw, ldc = strides(c)
    if c.wt not in (W_INT8_SQ, W_FP16):
        return ('refused', 'weight type')
    if sq and c.epi == EPI_GATE:
        return ('refused', 'SmoothQuant has no fused gate')
    if not sq and c.out == DT_INT32:
        return ('refused', 'int32 output needs SmoothQuant')
    if (lda * es) & 15 or ldw & 15 or (c.K * es) % 128 or c.K <= 0 or c.M < 32:
        return ('refused', 'alignment / K / M')
    if c.M * lda * es >= 1 << 31 or c.N * ldw >= 1 << 31:
        return ('refused', '32-bit DMA offsets')
    if c.epi in (EPI_RES, EPI_GATE) and _vec_rows_bad(c):
        return ('refused', 'the fused epilogue operand lives in the vector epilogue')
    if cfg in ABLATIONS or cfg not in table:
        return ('refused', 'no such id for this weight type')
    t = table[cfg]
    bm, bn = sqp_tile(t)
    tiles = _cdiv(c.M, bm) * _cdiv(c.N, bn)
    if t[4]:
        if _vec_rows_bad(c) or c.K < PERSIST_MIN_K[c.wt]:
            return ('refused', 'persistent: fp16 output on 16-byte rows, K >= %d' % PERSIST_MIN_K[c.wt])
        return ('persist', c.wt, cfg)
    if t[5]:
        if _vec_rows_bad(c):
            return ('refused', 'split-K: fp16 output on 16-byte rows')
        if 2 * tiles > cus * SPLITK_PER_CU[cfg] or c.K * es // 128 < SPLITK_MIN_KTILES:
            return ('refused', 'split-K: both workgroups of every tile resident, at least 4 K-tiles')
        if tiles * 2 * 4 > SPLITK_FLAG_BYTES:
            return ('refused', 'split-K: flag words')
        return ('splitk', c.wt, cfg)
    return ('phased', c.wt, cfg)


def persist_walk(c, cus):
    """(tiles_m, tiles, grid) of a persistent id for the case"""
    t = (SQP if c.wt == W_INT8_SQ else F16P)[c.kernel]
    bm, bn = sqp_tile(t)
    tiles = _cdiv(c.M, bm) * _cdiv(c.N, bn)
    return _cdiv(c.M, bm), tiles, persist_grid(tiles, cus)


def launch_gemm_cfg(c, cfg, cus):
    if not glds_serves(c):
        return ('refused', 'glds_serves')
    if cfg in GLDS:
        return ('lockstep', c.wt, cfg)
    return phased(c, cfg, cus)


def _served(i):
    return i[0] != 'refused'


def glds_dispatch(c, cus):
    """launch_gemm_glds: (branch, instance) or None (not served: the caller goes on)"""
    if not glds_serves(c):
        return None
    cfg, from_table = c.force, False
    if cfg <= 0:
        cfg = c.table
        from_table = cfg > 0
    branch = 'forced' if c.force > 0 else ('table' if from_table else 'static')
    if cfg > NUM_CFG and cfg not in GLDS:
        i = phased(c, cfg, cus)
        if _served(i):
            return (branch + ':phased', i)
        cfg, branch = 0, branch + '-refused>static'
    if cfg <= 0 or cfg not in GLDS:
        cfg = static_shape_cfg(c, cus)
        if cfg == PHASED_256x128:
            sq = c.wt == W_INT8_SQ
            i = phased(c, 62 if sq else 56, cus)
            if _served(i):
                return (branch + ':256x128-persist', i)
            i = phased(c, 42 if sq else 54, cus)
            if _served(i):
                return (branch + ':256x128-one-tile', i)
            cfg = static_shape_cfg(c, cus, False)
    if cfg == 6 and c.force <= 0 and not from_table:
        sq = c.wt == W_INT8_SQ
        i = phased(c, 63 if sq else 55, cus)
        if _served(i):
            return (branch + ':256x192-persist', i)
        i = phased(c, 20 if sq else 50, cus)
        if _served(i):
            return (branch + ':256x192-one-tile', i)
    return (branch + ':lockstep', ('lockstep', c.wt, cfg))


# ---------------------------------------------------------------------------------------------- gemm_woq.hip, gemm_mfma.hip
def woq_serves(c):
    if c.wt not in (W_INT8_WOQ, W_INT4_WOQ):
        return False
    lda, ldw, _ = strides(c)
    if (lda * 2) & 15 or ldw & 15 or c.K % 64 or c.K <= 0 or c.M < 32:
        return False
    if c.out not in (DT_HALF, DT_FLOAT):
        return False
    if c.epi == EPI_RES and c.out != DT_HALF:
        return False
    if c.epi == EPI_GATE and _vec_rows_bad(c):
        return False
    return True


def woq_rule(c, cus):
    best, cfg = 1e30, 0
    for tid, bm, bn, f8, f4 in WOQ_CANDS:
        t = _cdiv(c.M, bm) * _cdiv(c.N, bn)
        if tid == 6 and t > 2 * cus:
            continue
        cost = float(_cdiv(t, cus)) * bm * bn * (f8 if c.wt == W_INT8_WOQ else f4)
        if cost < best:
            best, cfg = cost, tid
    return cfg


def mfma_serves(c):
    """launch_gemm_mfma (epilogue operands are the caller's business)"""
    es = es_of(c.wt)
    lda, ldw, _ = strides(c)
    if (lda * es) & 15 or ldw & 15 or (c.K * es) % 16:
        return False
    if c.wt == W_INT8_WOQ and c.K % 16:
        return False
    if c.wt == W_INT4_WOQ and c.K % 32:
        return False
    if c.wt != W_INT8_SQ and c.out == DT_INT32:
        return False
    return True


# ---------------------------------------------------------------------------------------------- the entry points
def kernel_instance(c, cus):
    """tllm_gemm_kernel"""
    k = c.kernel
    if c.M <= 0 or c.N <= 0 or c.K <= 0:
        return ('refused', 'empty')
    if k in ABLATIONS:
        return ('refused', 'ablation')
    if 1 <= k <= 65:
        return launch_gemm_cfg(c, k, cus)
    if 101 <= k <= 106:
        return ('woq', c.wt, k - 100) if woq_serves(c) else ('refused', 'woq_serves')
    if k == REGISTER_STAGED:
        if c.epi != EPI_NONE:
            return ('refused', 'the register-staged kernel fuses no epilogue operand')
        return ('regstaged', c.wt) if mfma_serves(c) else ('refused', 'launch_gemm_mfma')
    return ('refused', 'no such kernel id')


def dual_instance(c):
    """launch_gemm_swiglu behind tllm_gemm_swiglu_quant"""
    lda, ldw, ldc = strides(c)
    if c.wt != W_INT8_SQ or c.per_token or c.epi != EPI_NONE:
        return ('refused', 'SmoothQuant with static scales only')
    if lda & 15 or ldw & 15 or c.K % 128 or c.K <= 0 or c.M < 32:
        return ('refused', 'alignment / K / M')
    if c.M * lda >= 1 << 31 or c.N * ldw >= 1 << 31:
        return ('refused', '32-bit DMA offsets')
    if not ldc & 15 and not c.N & 15 and c.K >= 256 and c.force != -2:
        return ('dual', 'persist')
    return ('dual', 'one')


def dispatch(c, cus, inplace=False):
    """launch_gemm: (branch, instance, pass behind it) or ('refused', reason)"""
    _, _, ldc = strides(c)
    if c.epi != EPI_NONE and c.out != DT_HALF:
        return ('refused', 'epilogue operands need fp16 output')
    if c.epi == EPI_GATE and c.wt == W_INT8_SQ:
        if ldc != c.N:
            return ('refused', 'strided gate with SmoothQuant')
        i = dispatch(c._replace(epi=EPI_NONE), cus)
        return ('sq-gate>' + i[0], i[1], 'swiglu')
    if c.M > 8:
        if c.wt in (W_INT8_WOQ, W_INT4_WOQ) and woq_serves(c):
            tile = c.force - 100 if c.force > 100 else woq_rule(c, cus)
            return ('woq', ('woq', c.wt, tile if 2 <= tile <= 6 else 1), None)
        g = glds_dispatch(c, cus)
        if g:
            return (g[0], g[1], None)
    if c.epi == EPI_GATE and ldc != c.N:
        return ('refused', 'strided gate behind a kernel that does not fuse it')
    if c.epi == EPI_RES and (ldc != c.N or inplace):
        return ('refused', 'strided / in-place residual behind a kernel that does not fuse it')
    post = {EPI_NONE: None, EPI_RES: 'add', EPI_GATE: 'swiglu'}[c.epi]
    if c.M > 8 and mfma_serves(c):
        return ('regstaged', ('regstaged', c.wt), post)
    if c.M <= 8:
        return ('gemv', ('gemv', c.wt), post)
    return ('slabs', ('slabs', c.wt, tuple(min(8, c.M - m0) for m0 in range(0, c.M, 8))), post)


def instance(c, cus=TABLE_CUS, inplace=False):
    if c.kernel == DUAL:
        return dual_instance(c)
    if c.kernel == 0:
        return dispatch(c, cus, inplace)
    return kernel_instance(c, cus)


def key(i):
    """what the completeness check counts: the kernel instance (dispatch results: the instance they end in), slabs by weight type"""
    if i[0] in ('refused', 'dual'):
        return i
    if isinstance(i[1], tuple):
        i = i[1]
    return i[:2] if i[0] in ('slabs', 'gemv') else i


def reachable_kernels():
    """every instance a `case` label can launch (the ablations left out), the weight-only tiles, the register-staged kernel,
    both dual forms, the GEMV slabs of the weight types whose K can miss the register-staged kernel's vectors"""
    out = {('lockstep', wt, i) for wt in (W_INT8_SQ, W_FP16) for i in GLDS}
    for wt, table in ((W_INT8_SQ, SQP), (W_FP16, F16P)):
        out |= {('persist' if t[4] else ('splitk' if t[5] else 'phased'), wt, i) for i, t in table.items()}
    out |= {('woq', wt, i) for wt in (W_INT8_WOQ, W_INT4_WOQ) for i in WOQ}
    out |= {('regstaged', wt) for wt in WTS}
    out |= {('dual', 'persist'), ('dual', 'one')}
    out |= {('slabs', W_INT8_WOQ), ('slabs', W_INT4_WOQ)}
    return out


# the branches of launch_gemm / launch_gemm_glds a dispatch case can end in.  (`*:256x128*` falling through to a lock-step shape
# needs the phased launcher to refuse what glds_serves took: only the 32-bit DMA offsets, 2 GiB operands - not run.)
BRANCHES = ('woq', 'regstaged', 'slabs', 'gemv', 'sq-gate>static:lockstep', 'static:lockstep', 'static:256x128-persist',
            'static:256x128-one-tile', 'static:256x192-persist', 'static:256x192-one-tile', 'forced:lockstep', 'forced:phased',
            'forced-refused>static:lockstep', 'table:lockstep', 'table:phased', 'table-refused>static:lockstep')
POSTS = (('regstaged', 'add'), ('regstaged', 'swiglu'), ('slabs', 'add'), ('slabs', 'swiglu'))


# ---------------------------------------------------------------------------------------------- the cases
SQ, F16, W8, W4 = W_INT8_SQ, W_FP16, W_INT8_WOQ, W_INT4_WOQ


def _ktile(wt, n):
    """K of n 128-byte K-tiles"""
    return n * 128 // es_of(wt)


def _one_tile_family(wt, ids, fam):
    """ids x two cases each: A = 300 x 456, 9 K-tiles, every stride padded; B = one 128-byte K-tile, M = 32 / 33.  The variants
    rotate over the ids so that every family (4+ ids) sees the four scale combinations, float32 / int32 output, the scalar
    epilogue (N = 453, odd ldc), and the residual out of place, in place and strided; fp16: the gate."""
    sq = wt == SQ
    out = []
    for n, i in enumerate(ids):
        a = [dict(per_channel=1, per_token=1),
             dict(per_channel=0, per_token=1, epi=EPI_RES, inplace=1),
             dict(per_channel=1, per_token=0, out=DT_FLOAT),
             dict(per_channel=0, per_token=0, out=DT_INT32) if sq else dict(epi=EPI_GATE)][n % 4]
        out.append(Case(f'{fam}-A{n % 4}', wt, 300, 456, _ktile(wt, 9), kernel=i, strided=1, **a))
        b = [dict(M=32, N=453, ldc_odd=1, per_channel=0, per_token=0),
             dict(M=33, N=456, epi=EPI_RES, inplace=1),
             dict(M=33, N=453, ldc_odd=1, out=DT_FLOAT, per_channel=0, per_token=1),
             dict(M=32, N=456, out=DT_INT32, per_channel=1, per_token=0) if sq else dict(M=32, N=456, epi=EPI_GATE)][(n + 1) % 4]
        out.append(Case(f'{fam}-B{(n + 1) % 4}', wt, K=_ktile(wt, 1), kernel=i, **b))
    return out


def _persistent():
    out = []
    for wt, ids in ((SQ, (60, 62, 63)), (F16, (55, 56))):
        kmin = PERSIST_MIN_K[wt]
        for n, i in enumerate(ids):
            bm, bn = sqp_tile((SQP if wt == SQ else F16P)[i])
            # tiles_m 1, 2, 5, 6, 7 (bands of 4 row tiles: a short last band), grids that are no multiples of 8, the shortest K
            for tm, tn, extra in ((1, 3, {}), (2, 5, dict(epi=EPI_RES, inplace=1, strided=1)), (5, 3, {}),
                                  (6, 3, dict(epi=EPI_GATE) if wt == F16 else dict(per_channel=0, per_token=0)),
                                  (7, 5, dict(strided=1))):
                out.append(Case(f'persist-tm{tm}', wt, tm * bm - 37, tn * bn - 8, kmin if tm != 2 else 3 * kmin, kernel=i, **extra))
            # two and three tiles per workgroup at 256 CUs: 5 x 54 = 270 tiles -> 135 workgroups, 5 x 103 = 515 -> 172
            out.append(Case('persist-x2', wt, 5 * bm - 100, 54 * bn - 8, kmin, kernel=i, epi=EPI_RES if n % 2 else EPI_NONE))
            if i in (63, 55):
                out.append(Case('persist-x3', wt, 5 * bm - 100, 103 * bn - 8, kmin, kernel=i))
            # refusals
            out.append(Case('persist-no-f32', wt, 300, 456, 2 * kmin, kernel=i, out=DT_FLOAT))
            out.append(Case('persist-no-n453', wt, 300, 453, 2 * kmin, kernel=i, ldc_odd=0))
            out.append(Case('persist-no-odd-ldc', wt, 300, 456, 2 * kmin, kernel=i, ldc_odd=1))
            out.append(Case('persist-no-short-k', wt, 300, 456, kmin // 2, kernel=i))
    out.append(Case('persist-no-gate', SQ, 300, 456, 512, kernel=63, epi=EPI_GATE))
    return out


def _split_k():
    out = []
    for wt, ids in ((SQ, (64, 65)), (F16, (57, 58))):
        for i in ids:
            bm, bn = sqp_tile((SQP if wt == SQ else F16P)[i])
            per_cu = SPLITK_PER_CU[i]
            mk = lambda name, tm, tn, kt, **kw: Case(name, wt, tm * bm - 19, tn * bn - 8, _ktile(wt, kt), kernel=i, repeat=3, **kw)
            out.append(mk('splitk-one-tile', 1, 1, 4))
            out.append(mk('splitk-few', 2, 3, 5, epi=EPI_RES, inplace=1, strided=1))
            out.append(mk('splitk-few13', 3, 2, 13, **(dict(epi=EPI_GATE) if wt == F16 else dict(per_channel=0, per_token=0))))
            out.append(mk('splitk-full', 8, 16, 4))                                    # 128 tiles: one workgroup per CU at 256 CUs
            if per_cu == 2:
                out.append(mk('splitk-two-per-cu', 16, 16, 5, epi=EPI_RES))            # 256 tiles: needs two per CU
            out.append(mk('splitk-no-3-ktiles', 2, 2, 3))
            out.append(mk('splitk-no-f32', 2, 2, 4, out=DT_FLOAT))
            out.append(mk('splitk-no-1056-tiles', 33, 32, 4))                                 # 1056 tiles: beyond the flag words, any occupancy
    # the certainly refused problem through the dispatch with the id forced: the fall-back's result
    out.append(Case('splitk-beyond-forced', SQ, 33 * 128 - 19, 32 * 128 - 8, 512, force=65))
    out.append(Case('splitk-beyond-forced', F16, 33 * 128 - 19, 32 * 128 - 8, 256, force=58))
    return out


def _dual():
    mk = lambda name, m, n, k, **kw: Case(name, SQ, m, n, k, out=DT_INT8, per_token=0, kernel=DUAL, **kw)
    return [mk('dual-one-k128', 32, 96, 128), mk('dual-persist', 300, 96, 256), mk('dual-one-forced', 300, 96, 256, force=-2),
            mk('dual-one-n104', 300, 104, 256), mk('dual-one-ragged', 300, 205, 256, strided=1),
            mk('dual-one-odd-ldc', 32, 200, 384, ldc_odd=1), mk('dual-persist-strided', 300, 208, 384, strided=1),
            mk('dual-persist-m32', 32, 208, 256), mk('dual-no-per-token', 300, 96, 256)._replace(per_token=1),
            mk('dual-no-k64', 300, 96, 192)]


def _weight_only():
    out = []
    for wt in (W8, W4):
        for n, tile in enumerate(WOQ):
            a = [dict(), dict(epi=EPI_RES, inplace=1), dict(out=DT_FLOAT), dict(epi=EPI_GATE)][n % 4]
            out.append(Case(f'woq-A{n % 4}', wt, 300, 456, 704, kernel=100 + tile, strided=1, **a))
            b = [dict(M=32, N=453, ldc_odd=1), dict(M=33, N=456, epi=EPI_RES, inplace=1), dict(M=33, N=453, ldc_odd=1, out=DT_FLOAT),
                 dict(M=32, N=456, epi=EPI_GATE)][(n + 1) % 4]
            out.append(Case(f'woq-B{(n + 1) % 4}', wt, K=64, kernel=100 + tile, **b))
        out.append(Case('woq-res-scalar', wt, 300, 453, 128, kernel=102, epi=EPI_RES, inplace=1, ldc_odd=1))
        out.append(Case('woq-no-gate-n453', wt, 300, 453, 128, kernel=101, epi=EPI_GATE))
        out.append(Case('woq-no-res-f32', wt, 300, 456, 128, kernel=101, epi=EPI_RES, out=DT_FLOAT))
        out.append(Case('woq-no-k96', wt, 300, 456, 96, kernel=101))
        out.append(Case('woq-no-m31', wt, 31, 456, 128, kernel=101))
    return out


_RAGGED_K = {SQ: 80, F16: 40, W8: 48, W4: 96}   # one full 64-byte slab and a short one
_MIN_K = {SQ: 16, F16: 8, W8: 16, W4: 32}


def _register_staged():
    out = []
    for wt in WTS:
        outs = (DT_HALF, DT_FLOAT, DT_INT32) if wt == SQ else (DT_HALF, DT_FLOAT)
        for n, m in enumerate((9, 31, 130)):
            out.append(Case('regstaged-ragged-k', wt, m, 131, _RAGGED_K[wt], kernel=REGISTER_STAGED, out=outs[n % len(outs)],
                            strided=n % 2, per_channel=n % 2, per_token=(n + 1) % 2))
        out.append(Case('regstaged-min-k', wt, 31, 77, _MIN_K[wt], kernel=REGISTER_STAGED, out=outs[-1]))
        out.append(Case('regstaged-3-slabs', wt, 130, 257, 2 * _RAGGED_K[wt] - _MIN_K[wt], kernel=REGISTER_STAGED, strided=1))
        out.append(Case('regstaged-no-res', wt, 31, 80, _RAGGED_K[wt], kernel=REGISTER_STAGED, epi=EPI_RES))
        # through the dispatch: the pointwise pass behind it, and what that pass cannot take
        out.append(Case('regstaged-add', wt, 31, 80, _RAGGED_K[wt], epi=EPI_RES))
        out.append(Case('regstaged-no-strided-res', wt, 31, 80, _RAGGED_K[wt], epi=EPI_RES, strided=1))
        out.append(Case('regstaged-add-not-in-place', wt, 9, 80, _RAGGED_K[wt], epi=EPI_RES, inplace=1))
        if wt != SQ:
            out.append(Case('regstaged-swiglu', wt, 9, 80, _RAGGED_K[wt], epi=EPI_GATE))
            out.append(Case('regstaged-no-strided-gate', wt, 31, 80, _RAGGED_K[wt], epi=EPI_GATE, strided=1))
    out.append(Case('regstaged-sq-gate', SQ, 31, 80, 80, epi=EPI_GATE))
    return out


def _slabs():
    """what misses the register-staged kernel's vectors and still suits the GEMV: weight-only K that is a multiple of 8 but not
    of 16 (int8) / 32 (int4).  (fp16 / SmoothQuant K off their 16-byte vectors is refused by the GEMV as well.)"""
    out = []
    for wt, k in ((W8, 24), (W8, 72), (W4, 40), (W4, 80)):
        out.append(Case('slabs-m9', wt, 9, 67, k, out=DT_FLOAT if k > 60 else DT_HALF))
        out.append(Case('slabs-m20', wt, 20, 67, k, epi=EPI_RES if k > 60 else EPI_NONE))
    out.append(Case('slabs-swiglu', W8, 20, 64, 24, epi=EPI_GATE))
    out.append(Case('boundary-m8', W8, 8, 67, 24))
    out.append(Case('boundary-m8', W8, 8, 67, 48))   # M = 9 at this K: the register-staged kernel ('regstaged-ragged-k')
    return out


# the smallest M x N (multiples of 64 less a ragged edge) at which the static rule answers each id it can at 256 CUs: the wide
# tiles only win once the 128 x 128 tile needs a second round of workgroups, hence the long N.  (id, M, N, K bytes, fp16 output)
_STATIC = ((8, 59, 56, 512, 1), (2, 315, 24632, 512, 1), (4, 59, 49208, 512, 1), (62, 187, 16440, 512, 1), (42, 187, 16440, 128, 0),
           (63, 59, 32824, 512, 1), (20, 59, 32824, 128, 0)), \
          ((8, 59, 56, 512, 1), (2, 315, 24632, 512, 1), (4, 59, 32824, 512, 1), (56, 187, 16440, 512, 1), (54, 187, 16440, 128, 0),
           (55, 187, 32824, 512, 1), (50, 187, 32824, 128, 0))


def _dispatch():
    out = []
    for wt, rows in zip((SQ, F16), _STATIC):
        for i, m, n, kb, half in rows:
            out.append(Case(f'static-{i}', wt, m, n, kb // es_of(wt), out=DT_HALF if half else DT_FLOAT))
    # forced and table-driven ids: a serving one, and one that refuses the problem (the split-K forms take no float32 output)
    for wt, lock, ph, no in ((SQ, 3, 18, 65), (F16, 7, 52, 58)):
        k = _ktile(wt, 3)
        out.append(Case('forced-lockstep', wt, 300, 456, k, force=lock))
        out.append(Case('forced-phased', wt, 300, 456, k, force=ph, epi=EPI_RES))
        out.append(Case('forced-refused', wt, 300, 456, k, force=no, out=DT_FLOAT))
        out.append(Case('table-lockstep', wt, 300, 456, k, table=lock))
        out.append(Case('table-phased', wt, 300, 456, k, table=ph))
        out.append(Case('table-refused', wt, 300, 456, k, table=no, out=DT_FLOAT))
    out.append(Case('sq-gate-pass', SQ, 300, 456, 384, epi=EPI_GATE))
    out.append(Case('sq-gate-no-strided', SQ, 300, 456, 384, epi=EPI_GATE, strided=1))
    out.append(Case('woq-rule', W8, 300, 456, 128, epi=EPI_GATE))
    out.append(Case('woq-rule', W4, 700, 200, 192, epi=EPI_RES, inplace=1, strided=1))
    out.append(Case('woq-forced', W4, 300, 456, 128, force=105))
    return out


def _grid():
    cases = []
    cases += _one_tile_family(SQ, sorted(GLDS), 'lockstep')
    cases += _one_tile_family(F16, sorted(GLDS), 'lockstep')
    cases += _one_tile_family(SQ, (15, 18, 20, 42), 'phased')
    cases += _one_tile_family(F16, (50, 51, 52, 53, 54), 'phased')
    cases += [Case('ablation', SQ, 300, 456, 1152, kernel=i) for i in ABLATIONS]
    cases += [Case('wrong-type', F16, 300, 456, 576, kernel=20), Case('wrong-type', SQ, 300, 456, 1152, kernel=50),
              Case('no-such-id', SQ, 300, 456, 1152, kernel=13), Case('lockstep-no-m31', SQ, 31, 456, 1152, kernel=8),
              Case('lockstep-no-res-n453', F16, 300, 453, 576, kernel=8, epi=EPI_RES),
              Case('lockstep-no-s32', F16, 300, 456, 576, kernel=8, out=DT_INT32)]
    cases += _persistent() + _split_k() + _dual() + _weight_only() + _register_staged() + _slabs() + _dispatch()
    ids = [case_id(c) for c in cases]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return cases


CASES = _grid()
