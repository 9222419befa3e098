"""The case table of the decode GEMV (kernels/gemv.hip launch_gemv and the kernels it chooses among) - importable without a GPU.

launch_gemv picks one of about 170 compiled kernels by weight type, prologue family, epilogue family, row bucket, activation
register bucket, the 2-chunk int4 form, the K-split one-shot kernel, the matrix-pipe kernel and the LDS slab split.  instance()
below is a Python mirror of that choice:

    instance(case) -> ('valu', WT, PK, EK, MB, NXV, UU)      gemv_impl.h gemv_kernel<WT, PK, EK, MB, NXV, UU>
                    | ('ksplit', WT, NC)                     gemv_ksplit.hip gemv_ksplit_kernel<WT, NC>
                    | ('mfma', depth, swiglu)                gemv_mfma_sq.hip gemv_mfma_sq_kernel<.., SWIGLU, D>
                    | ('slab', fit, [inner instances])       the call is served in slabs of `fit` rows
                    | ('refused', reason)

tests/test_gemv_instance_table.py holds the mirror's constants against the source text and checks, without a GPU, that every
reachable instance has a case; tests/test_gpu_gemv_instances.py runs every case against oracle/gemv_oracle.py."""
from collections import namedtuple

# kernels.h
W_FP16, W_INT8_WOQ, W_INT4_WOQ, W_INT8_SQ = 0, 1, 2, 3
PRO_NONE, PRO_RMSNORM, PRO_RMSNORM_QSTATIC, PRO_RMSNORM_QDYN, PRO_QSTATIC, PRO_QDYN = 0, 1, 2, 3, 4, 5
EPI_NONE, EPI_RESIDUAL, EPI_SWIGLU, EPI_SWIGLU_QSTATIC = 0, 1, 2, 3
DT_FLOAT, DT_HALF, DT_INT8, DT_INT32 = 0, 1, 2, 3
WTS = (W_FP16, W_INT8_WOQ, W_INT4_WOQ, W_INT8_SQ)
WT_NAME = {W_FP16: 'fp16', W_INT8_WOQ: 'woq8', W_INT4_WOQ: 'woq4', W_INT8_SQ: 'sq'}
PRO_NAME = {0: 'copy', 1: 'rms', 2: 'rms+qs', 3: 'rms+qd', 4: 'qs', 5: 'qd'}
EPI_NAME = {0: 'none', 1: 'res', 2: 'swiglu', 3: 'swiglu+q'}
DT_NAME = {DT_FLOAT: 'f32', DT_HALF: 'f16', DT_INT8: 's8', DT_INT32: 's32'}

# gemv_args.h / gemv_impl.h / gemv_ksplit.hip / gemv_mfma_sq.hip (held against the source text by test_gemv_instance_table.py)
R, U = 2, 4
RED_BYTES = 384
NXV_SMALL, NXV_MAX, NXV_LARGE = 2, 6, 12
LDS_LIMIT = 160 * 1024
PK_COPY, PK_NORM, PK_QUANT = 0, 1, 2
EK_PLAIN, EK_SWIGLU = 0, 1
VEC = {W_FP16: 8, W_INT8_WOQ: 16, W_INT4_WOQ: 32, W_INT8_SQ: 16}  # weights per 16-byte vector
KSPLIT_RW = {W_FP16: 4, W_INT8_WOQ: 4, W_INT4_WOQ: 4, W_INT8_SQ: 2}
KSPLIT_NCMAX = {W_FP16: 6, W_INT8_WOQ: 3, W_INT4_WOQ: 2, W_INT8_SQ: 3}
KSPLIT_NMAX = 8192
MFMA_ROWS_DEFAULT, MFMA_KROWS = 5, 8

_FIELDS = dict(name='', wt=0, pro=0, epi=0, M=1, N=0, K=0, out=DT_HALF, per_channel=1, per_token=0,
               mfma_rows=-1,      # tllm_gemv_set_mfma_rows (-1 = the default, 0 = never)
               blocks_per_cu=0,   # tllm_gemv_set_blocks_per_cu (0 = the occupancy query)
               strided=0,         # ldx > K, ldy > N, ldw > row bytes; every padding byte 0xFF
               inplace=0,         # also run with residual == y: the bits must equal the out-of-place run
               dc=0,              # x = 3 + N(0, 1) instead of 1.7 N(0, 1)
               side=None)         # x_pro_out / dyn_scale_out passed (None: whenever the call has a prologue)
Case = namedtuple('Case', list(_FIELDS), defaults=list(_FIELDS.values()))


def has_side(c):
    return (c.pro != PRO_NONE) if c.side is None else bool(c.side)


def is_swiglu(c):
    return c.epi in (EPI_SWIGLU, EPI_SWIGLU_QSTATIC)


def out_dtype(c):
    return DT_INT8 if c.epi == EPI_SWIGLU_QSTATIC else (DT_HALF if c.epi in (EPI_RESIDUAL, EPI_SWIGLU) else c.out)


def round_up(v, m):
    return (v + m - 1) // m * m


def row_bytes(wt, K):
    """weight_layout.h row_bytes"""
    return {W_FP16: 2 * K, W_INT8_WOQ: round_up(K, 16), W_INT8_SQ: round_up(K, 16), W_INT4_WOQ: round_up(K, 32) // 2}[wt]


def strides(c):
    """(ldx elements, ldy elements, ldw bytes)"""
    rb = row_bytes(c.wt, c.K)
    return (c.K + 16, c.N + 8, rb + 32) if c.strided else (c.K, c.N, rb)


def nchunks(wt, K):
    return (round_up(K, VEC[wt]) + 64 * VEC[wt] - 1) // (64 * VEC[wt])


def pro_kind(pro):
    return {PRO_NONE: PK_COPY, PRO_RMSNORM: PK_NORM, PRO_RMSNORM_QSTATIC: PK_NORM, PRO_RMSNORM_QDYN: PK_NORM,
            PRO_QSTATIC: PK_QUANT, PRO_QDYN: PK_QUANT}[pro]


def mfma_depth(K, swiglu):
    """launch_depth: the deepest weight ring the LDS holds next to the activation rows (0 = none fits)"""
    slot = (8 if swiglu else 4) * 1024
    fixed = RED_BYTES + 2 * (2 if swiglu else 1) * 4 * 64 * 16 + (MFMA_KROWS + 1) * (K + 16)
    for d in ((3, 2) if swiglu else (4, 3, 2)):
        if fixed + 4 * d * slot <= LDS_LIMIT:
            return d
    return 0


def _mfma(c):
    """launch_gemv_mfma_sq: the instance, or None where the call goes on to the vector-ALU kernels.  (Pointers are 256-byte
    aligned in the tests; scale_col is always passed.)"""
    rows = MFMA_ROWS_DEFAULT if c.mfma_rows < 0 else c.mfma_rows
    if rows <= 0 or c.M < rows or c.M > MFMA_KROWS or c.wt != W_INT8_SQ:
        return None
    norm = c.pro == PRO_RMSNORM_QSTATIC
    if not norm and c.pro != PRO_NONE:
        return None
    if c.per_token or has_side(c):
        return None
    ldx, ldy, ldw = strides(c)
    if c.N % 16 or c.K % 256 or ldw % 16 or ldy % 4:
        return None
    if c.epi == EPI_RESIDUAL and out_dtype(c) != DT_HALF:
        return None
    if norm and (ldx % 8 or c.K > 256 * 8 * NXV_MAX):
        return None
    if not norm and ldx % 16:
        return None
    d = mfma_depth(c.K, is_swiglu(c))
    return ('mfma', d, is_swiglu(c)) if d else None


def _ksplit(c):
    """gemv_ksplit_applies + launch_gemv_ksplit: NC, or 0"""
    if c.M != 1 or c.pro != PRO_NONE or c.epi not in (EPI_NONE, EPI_RESIDUAL) or has_side(c) or c.per_token:
        return 0
    if not (out_dtype(c) in (DT_HALF, DT_FLOAT) or (out_dtype(c) == DT_INT32 and c.wt == W_INT8_SQ)):
        return 0
    nc = nchunks(c.wt, c.K)
    if not (nc > 4 and nc <= 4 * KSPLIT_NCMAX[c.wt] and c.K % VEC[c.wt] == 0 and c.N <= KSPLIT_NMAX):
        return 0
    return (nc + 3) // 4


def instance(c):
    if c.M < 1 or c.M > 8 or c.N <= 0 or c.K <= 0:
        return ('refused', 'shape')
    sq = c.wt == W_INT8_SQ
    if sq and c.M >= 2:
        m = _mfma(c)
        if m:
            return m
    es = 1 if sq else 2
    kp = round_up(c.K, 32)
    mb = 1 if c.M <= 1 else (2 if c.M <= 2 else (4 if c.M <= 4 else 8))
    fit = mb
    while fit > 1 and RED_BYTES + fit * kp * es > LDS_LIMIT:
        fit >>= 1
    if fit < mb:
        inner = [instance(c._replace(M=min(fit, c.M - m0))) for m0 in range(0, c.M, fit)]
        bad = [i for i in inner if i[0] == 'refused']
        return bad[0] if bad else ('slab', fit, inner)
    swiglu = is_swiglu(c)
    if not sq and c.pro in (PRO_RMSNORM_QSTATIC, PRO_RMSNORM_QDYN, PRO_QSTATIC, PRO_QDYN):
        return ('refused', 'quantising prologue needs SmoothQuant weights')
    pk = pro_kind(c.pro)
    if sq and c.pro == PRO_RMSNORM:
        return ('refused', 'SmoothQuant needs a quantising prologue')
    raw_s8 = sq and c.pro == PRO_NONE
    xvec = 16 if raw_s8 else 8
    lim = NXV_LARGE if (pk in (PK_COPY, PK_QUANT) and not swiglu) else NXV_MAX
    if c.K % xvec or c.K > 256 * xvec * lim:
        return ('refused', 'K')
    nc = _ksplit(c)
    if nc:
        return ('ksplit', c.wt, nc)
    if swiglu and pk == PK_QUANT:
        return ('refused', 'SwiGLU is built with the copy / RMSNorm prologues only')
    ek = EK_SWIGLU if swiglu else EK_PLAIN
    if c.K <= 256 * xvec * NXV_SMALL:
        nxv = NXV_SMALL
    elif c.K <= 256 * xvec * NXV_MAX:
        nxv = NXV_MAX
    else:
        nxv = NXV_LARGE  # (lim has refused the others)
    uu = 2 if (c.wt == W_INT4_WOQ and c.M <= 1 and nchunks(c.wt, c.K) <= 2) else U
    return ('valu', c.wt, pk, ek, mb, nxv, uu)


def families(wt):
    """the (PK, EK) pairs launch_wt builds for a weight type"""
    f = [(PK_COPY, EK_PLAIN), (PK_NORM, EK_PLAIN), (PK_COPY, EK_SWIGLU), (PK_NORM, EK_SWIGLU)]
    return f + [(PK_QUANT, EK_PLAIN)] if wt == W_INT8_SQ else f


def buckets(pk, ek):
    """the activation-register buckets launch_nxv builds for a family"""
    return (NXV_SMALL, NXV_MAX, NXV_LARGE) if (pk in (PK_COPY, PK_QUANT) and ek == EK_PLAIN) else (NXV_SMALL, NXV_MAX)


def bucket_k(wt, pk, nxv):
    """(lowest, highest) K of a bucket"""
    xvec = 16 if (wt == W_INT8_SQ and pk == PK_COPY) else 8
    prev = {NXV_SMALL: 0, NXV_MAX: NXV_SMALL, NXV_LARGE: NXV_MAX}[nxv]
    return 256 * xvec * prev + xvec, 256 * xvec * nxv


def reachable_valu():
    """every (WT, PK, EK, MB, NXV, UU) launch_wt -> launch_nxv -> launch_mb can be asked for: the bucket's smallest K must fit
    the LDS with MB rows (else launch_gemv has cut the call into slabs of a smaller bucket); int4 single rows of at most two
    chunks take the 2-chunk form, and K <= 4096 is at most two int4 chunks"""
    out = set()
    for wt in WTS:
        for pk, ek in families(wt):
            for nxv in buckets(pk, ek):
                lo, hi = bucket_k(wt, pk, nxv)
                for mb in (1, 2, 4, 8):
                    if RED_BYTES + mb * round_up(lo, 32) * (1 if wt == W_INT8_SQ else 2) > LDS_LIMIT:
                        continue
                    uus = {2 if (wt == W_INT4_WOQ and mb == 1 and nchunks(wt, k) <= 2) else U for k in (lo, hi)}
                    out |= {('valu', wt, pk, ek, mb, nxv, uu) for uu in uus}
    return out


def reachable_ksplit():
    return {('ksplit', wt, nc) for wt in WTS for nc in range(2, KSPLIT_NCMAX[wt] + 1)}


def reachable_mfma():
    return {('mfma', d, sw) for sw in (False, True) for d in ((3, 2) if sw else (4, 3, 2))}


# ---------------------------------------------------------------------------------------------- the grid: one case per instance
_M_OF = {1: (1, ), 2: (2, ), 4: (3, 4), 8: (5, 7, 8)}  # every bucket entered full and part-filled


def _edges(wt, pk, nxv):
    """K at the edges of a bucket: 64 (one partial chunk), 4096 | 4104, 12288 | 12296 (twice that for raw s8 activations, whose
    vectors hold 16 values).  4104 = 8 * 513 and 12296 = 8 * 1537 are 8 * odd: Kp > K for int8 (16) and int4 (32) weights."""
    lo, hi = bucket_k(wt, pk, nxv)
    return (64, hi) if nxv == NXV_SMALL else ((lo, hi) if nxv == NXV_MAX else (lo, ))


def _grid():
    cases, i = [], 0
    for wt in WTS:
        sq = wt == W_INT8_SQ
        for pk, ek in families(wt):
            for nxv in buckets(pk, ek):
                for mb in (1, 2, 4, 8):
                    i += 1
                    if pk == PK_COPY:
                        pro = PRO_NONE
                    elif pk == PK_NORM:
                        pro = (PRO_RMSNORM_QSTATIC, PRO_RMSNORM_QDYN)[i % 2] if sq else PRO_RMSNORM
                    else:
                        pro = (PRO_QSTATIC, PRO_QDYN)[i % 2]
                    if ek == EK_SWIGLU:
                        epi = (EPI_SWIGLU, EPI_SWIGLU_QSTATIC)[(i // 2) % 2] if sq else EPI_SWIGLU
                    else:
                        epi = (EPI_NONE, EPI_RESIDUAL, EPI_NONE)[i % 3]
                    out = (DT_HALF, DT_FLOAT, DT_INT32 if sq else DT_HALF)[(i // 3) % 3] if epi == EPI_NONE else DT_HALF
                    n = 66 + (i * 7) % 64
                    n += 1 if n % 8 == 0 else 0
                    static = sq and pro in (PRO_NONE, PRO_RMSNORM_QSTATIC, PRO_QSTATIC)
                    base = Case(wt=wt, pro=pro, epi=epi, N=n, out=out, per_channel=(i // 2) % 2 if sq else 1,
                                per_token=1 if (static and i % 3 == 0) else 0,
                                dc=1 if (wt in (W_INT8_WOQ, W_INT4_WOQ) and nxv == NXV_MAX and mb == 4) else 0)
                    ks, ms = _edges(wt, pk, nxv), _M_OF[mb]
                    j = i // 4 + (i // 4) // 3  # the rows and the edge change from bucket to bucket and from family to family
                    tries = [base._replace(M=ms[(j + a) % len(ms)], K=ks[(j + mb.bit_length() + b) % len(ks)], side=s)
                             for s in (None, 1) for b in range(len(ks)) for a in range(len(ms))]
                    for c in tries:
                        t = instance(c)
                        if t[0] == 'valu' and t[1:6] == (wt, pk, ek, mb, nxv):
                            cases.append(c._replace(name='grid'))
                            break
    return cases


GRID = _grid()

# ---------------------------------------------------------------------------------------------- the cases named by purpose
_C = Case
SQ, F16, W8, W4 = W_INT8_SQ, W_FP16, W_INT8_WOQ, W_INT4_WOQ

# several row groups per wave (tllm_gemv_set_blocks_per_cu(1): 256 CUs x 4 waves, 3075 / 6150 row groups): the persistent grid
# and the look-ahead of the next group's epilogue operands (scales, residual); K = 256 keeps the weights at a few MB
GROUPS = [
    _C('groups', F16, PRO_NONE, EPI_RESIDUAL, 3, 6150, 256, blocks_per_cu=1, inplace=1),
    _C('groups', F16, PRO_RMSNORM, EPI_SWIGLU, 2, 6150, 256, blocks_per_cu=1),
    _C('groups', W8, PRO_RMSNORM, EPI_RESIDUAL, 4, 6150, 256, blocks_per_cu=1, inplace=1),
    _C('groups', W4, PRO_NONE, EPI_SWIGLU, 1, 6150, 256, blocks_per_cu=1),
    _C('groups', SQ, PRO_RMSNORM_QSTATIC, EPI_SWIGLU_QSTATIC, 5, 6150, 256, blocks_per_cu=1),
    _C('groups', SQ, PRO_QDYN, EPI_RESIDUAL, 7, 6150, 256, blocks_per_cu=1, inplace=1),
]


def _ksplit_k(wt, nc, upper):
    """a K of nchunks = 4 nc (the deepest a wave of this NC goes) or 4 (nc - 1) + 1 with a partial last chunk"""
    chunk = 64 * VEC[wt]
    return chunk * 4 * nc if upper else chunk * 4 * (nc - 1) + 3 * VEC[wt]


# K-split: every NC of every weight type, N = 67 leaves the last workgroup 3 rows of 4 (SmoothQuant: 1 of 2); N = 1; the largest N
# it serves and the first it does not
KSPLIT = [_C('ksplit', wt, PRO_NONE, (EPI_NONE, EPI_RESIDUAL)[nc % 2], 1, 67, _ksplit_k(wt, nc, (nc + wt) % 2),
             out=(DT_HALF, DT_FLOAT)[(nc // 2) % 2], dc=1 if wt in (W8, W4) else 0, inplace=nc % 2)
          for wt in WTS for nc in range(2, KSPLIT_NCMAX[wt] + 1)] + [
    _C('ksplit', F16, PRO_NONE, EPI_NONE, 1, 1, 2568),
    _C('ksplit', W4, PRO_NONE, EPI_RESIDUAL, 1, 1, 8224),
    _C('ksplit', SQ, PRO_NONE, EPI_NONE, 1, 67, 4112, out=DT_INT32, per_channel=0),
    _C('ksplit', SQ, PRO_NONE, EPI_RESIDUAL, 1, 8192, 4112),
    _C('ksplit-refused', SQ, PRO_NONE, EPI_RESIDUAL, 1, 8193, 4112),
]

# strides: ldx > K, ldy > N, ldw > row bytes with every padding byte 0xFF (fp16 NaN) - K = 72 = 8 * 9 leaves a Kp - K tail in the
# int8 (80) and int4 (96) rows
STRIDES = [
    _C('strides', F16, PRO_RMSNORM, EPI_RESIDUAL, 3, 69, 72, strided=1, inplace=1),
    _C('strides', F16, PRO_NONE, EPI_NONE, 2, 69, 4104, strided=1, out=DT_FLOAT),
    _C('strides', F16, PRO_NONE, EPI_SWIGLU, 5, 69, 72, strided=1),
    _C('strides', W8, PRO_RMSNORM, EPI_SWIGLU, 3, 69, 72, strided=1),
    _C('strides', W8, PRO_NONE, EPI_RESIDUAL, 8, 69, 4104, strided=1),
    _C('strides', W4, PRO_RMSNORM, EPI_RESIDUAL, 4, 69, 72, strided=1),
    _C('strides', W4, PRO_NONE, EPI_NONE, 1, 69, 4104, strided=1, side=1),
    _C('strides', SQ, PRO_RMSNORM_QDYN, EPI_RESIDUAL, 3, 69, 72, strided=1),
    _C('strides', SQ, PRO_NONE, EPI_SWIGLU_QSTATIC, 2, 69, 80, strided=1),
    _C('strides', F16, PRO_NONE, EPI_RESIDUAL, 1, 67, 2568, strided=1),             # K-split
    _C('strides', W4, PRO_NONE, EPI_NONE, 1, 67, 8224, strided=1),                  # K-split, a Kp - K tail of 0xFF nibbles
    _C('strides', SQ, PRO_NONE, EPI_RESIDUAL, 1, 67, 4112, strided=1),              # K-split
    _C('strides', SQ, PRO_RMSNORM_QSTATIC, EPI_RESIDUAL, 6, 80, 512, strided=1, side=0),   # matrix pipe
    _C('strides', SQ, PRO_NONE, EPI_SWIGLU, 8, 96, 256, strided=1),                 # matrix pipe
    _C('strides', SQ, PRO_RMSNORM_QSTATIC, EPI_RESIDUAL, 6, 80, 512, strided=1, side=0, mfma_rows=0),  # (the same two without it)
    _C('strides', SQ, PRO_NONE, EPI_SWIGLU, 8, 96, 256, strided=1, mfma_rows=0),
]

# slabs: 8 fp16 rows of K = 11008 (176 KB) and 4 of K = 22016 exceed the LDS, 8 int8 rows of K = 22016 too; scale_row,
# dyn_scale_out, x_pro_out, x, y and residual are re-offset per slab
SLABS = [
    _C('slab', F16, PRO_RMSNORM, EPI_RESIDUAL, 7, 69, 11008, inplace=1),
    _C('slab', F16, PRO_NONE, EPI_NONE, 5, 77, 11008, out=DT_FLOAT),
    _C('slab', F16, PRO_RMSNORM, EPI_SWIGLU, 8, 69, 11008),
    _C('slab', F16, PRO_NONE, EPI_RESIDUAL, 3, 69, 22016),
    _C('slab', F16, PRO_NONE, EPI_NONE, 4, 75, 22016),
    _C('slab', W8, PRO_RMSNORM, EPI_RESIDUAL, 8, 69, 11008, inplace=1),
    _C('slab', W8, PRO_NONE, EPI_NONE, 6, 69, 11008, dc=1),
    _C('slab', W4, PRO_RMSNORM, EPI_SWIGLU, 5, 69, 11008),
    _C('slab', W4, PRO_NONE, EPI_RESIDUAL, 7, 69, 11008, dc=1),
    _C('slab', SQ, PRO_QDYN, EPI_RESIDUAL, 7, 69, 22016, inplace=1),      # dyn_scale_out and x_pro_out across the slab boundary
    _C('slab', SQ, PRO_QDYN, EPI_NONE, 8, 69, 22016, out=DT_FLOAT, per_channel=0),
    _C('slab', SQ, PRO_QSTATIC, EPI_NONE, 5, 69, 22016, per_token=1),
    _C('slab', SQ, PRO_QSTATIC, EPI_RESIDUAL, 8, 69, 22016),
    _C('slab', SQ, PRO_NONE, EPI_NONE, 8, 69, 22016, per_token=1, out=DT_INT32),  # per-token scale_row[8] through a slab
]

# per-token scale_row[M], distinct per row (M = 8: SLABS)
PER_TOKEN = [
    _C('per-token', SQ, PRO_NONE, EPI_NONE, 3, 69, 64, per_token=1),
    _C('per-token', SQ, PRO_RMSNORM_QSTATIC, EPI_RESIDUAL, 5, 69, 4096, per_token=1, per_channel=0),
    _C('per-token', SQ, PRO_QSTATIC, EPI_NONE, 5, 80, 512, per_token=1, out=DT_FLOAT),  # (N, K) fit the matrix pipe; per-token does not
]


def _mfma_pair(**kw):
    """a SmoothQuant static call of 5 - 8 rows at the default (the matrix pipe) and with tllm_gemv_set_mfma_rows(0)"""
    return [_C('mfma', SQ, side=0, **kw), _C('mfma-off', SQ, side=0, mfma_rows=0, **kw)]


# the matrix-pipe kernel: every ring depth x SwiGLU form, raw int8 rows and the RMSNorm + static quantiser prologue (6 - vector and
# 2 - vector buckets), every epilogue and output type, 5 / 7 / 8 rows (2 / 3 with the threshold lowered)
MFMA = sum([
    _mfma_pair(pro=PRO_NONE, epi=EPI_NONE, M=6, N=80, K=256),
    _mfma_pair(pro=PRO_RMSNORM_QSTATIC, epi=EPI_RESIDUAL, M=5, N=96, K=4096, inplace=1),
    _mfma_pair(pro=PRO_RMSNORM_QSTATIC, epi=EPI_NONE, M=8, N=80, K=4352, out=DT_FLOAT, per_channel=0),
    _mfma_pair(pro=PRO_NONE, epi=EPI_NONE, M=7, N=112, K=9984, out=DT_INT32),           # depth 3
    _mfma_pair(pro=PRO_RMSNORM_QSTATIC, epi=EPI_RESIDUAL, M=8, N=80, K=11776),         # depth 2, RMSNorm bucket of 6
    _mfma_pair(pro=PRO_NONE, epi=EPI_RESIDUAL, M=5, N=80, K=13568, inplace=1),         # depth 2, the longest K it serves
    _mfma_pair(pro=PRO_RMSNORM_QSTATIC, epi=EPI_SWIGLU_QSTATIC, M=8, N=80, K=512),     # SwiGLU depth 3
    _mfma_pair(pro=PRO_NONE, epi=EPI_SWIGLU, M=7, N=96, K=5376, per_channel=0),
    _mfma_pair(pro=PRO_RMSNORM_QSTATIC, epi=EPI_SWIGLU, M=5, N=80, K=5632),            # SwiGLU depth 2
    _mfma_pair(pro=PRO_NONE, epi=EPI_SWIGLU_QSTATIC, M=8, N=112, K=8960),
], []) + [
    _C('mfma-rows2', SQ, PRO_RMSNORM_QSTATIC, EPI_NONE, 2, 80, 768, side=0, mfma_rows=2),
    _C('mfma-rows2', SQ, PRO_NONE, EPI_SWIGLU, 3, 80, 1024, side=0, mfma_rows=2),
    # not served at the default: N % 16, K % 256, a K whose ring does not fit, the first K past the SwiGLU ring
    _C('mfma-unserved', SQ, PRO_NONE, EPI_NONE, 6, 72, 256),
    _C('mfma-unserved', SQ, PRO_NONE, EPI_RESIDUAL, 6, 80, 272),
    _C('mfma-unserved', SQ, PRO_RMSNORM_QSTATIC, EPI_NONE, 8, 80, 264, side=0),
    _C('mfma-unserved', SQ, PRO_NONE, EPI_NONE, 8, 80, 13824),
    _C('mfma-unserved', SQ, PRO_RMSNORM_QSTATIC, EPI_SWIGLU, 8, 80, 9216, side=0),
]

# refusals at the far edge of the middle bucket: the normalising prologue and the SwiGLU epilogue stop at K = 12288
REFUSED = [
    _C('refused', F16, PRO_RMSNORM, EPI_NONE, 1, 69, 12296),
    _C('refused', W8, PRO_NONE, EPI_SWIGLU, 2, 69, 12296),
    _C('refused', W4, PRO_RMSNORM, EPI_SWIGLU, 8, 69, 12296),     # (through the slab split: every slab is refused)
    _C('refused', SQ, PRO_RMSNORM_QDYN, EPI_RESIDUAL, 3, 69, 12296),
    _C('refused', SQ, PRO_NONE, EPI_SWIGLU_QSTATIC, 4, 69, 24592),
    _C('refused', SQ, PRO_QSTATIC, EPI_SWIGLU, 1, 69, 64),         # SwiGLU behind the quantiser alone is not built
    _C('refused', F16, PRO_NONE, EPI_NONE, 1, 69, 24584),          # past the third bucket
]

CASES = GRID + GROUPS + KSPLIT + STRIDES + SLABS + PER_TOKEN + MFMA + REFUSED


def case_id(c):
    s = f'{c.name}-{WT_NAME[c.wt]}-{PRO_NAME[c.pro]}-{EPI_NAME[c.epi]}-{DT_NAME[out_dtype(c)]}-M{c.M}-N{c.N}-K{c.K}'
    s += ('' if c.per_channel else '-pertensor') + ('-tok' if c.per_token else '') + ('-dc' if c.dc else '')
    s += ('-strided' if c.strided else '') + ('-inplace' if c.inplace else '')
    s += ('' if c.side is None else f'-side{int(c.side)}') + ('' if c.mfma_rows < 0 else f'-mfma{c.mfma_rows}')
    return s
