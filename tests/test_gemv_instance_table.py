"""No GPU: the case table of tests/test_gpu_gemv_instances.py (tests/gemv_cases.py) against the dispatch of the decode GEMV as the
source states it - the constants and conditions the Python mirror gemv_cases.instance() depends on are read from the source text
(gemv_args.h, gemv.hip, gemv_impl.h, gemv_ksplit.hip, gemv_mfma_sq.hip) and fail here when they move; then every instance the
dispatch can reach must have a case.  An instance added to the dispatch without a case fails here."""
import os
import re

import gemv_cases as GC

KDIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'trtllm-llama_amd', 'csrc', 'kernels')


def src(name):
    return open(os.path.join(KDIR, name)).read()


def _body(text, head):
    """the text of the function whose definition starts with `head`, up to its closing brace at column 0"""
    i = text.index(head)
    return text[i:text.index('\n}\n', i)]


def _squash(s):
    return re.sub(r'\s+', ' ', s)


def test_the_mirror_constants_are_the_sources():
    a = src('gemv_args.h')
    assert re.search(r'constexpr int R = (\d+), U = (\d+);', a).groups() == (str(GC.R), str(GC.U))
    for name, v in (('kRedBytes', GC.RED_BYTES), ('kNXVMax', GC.NXV_MAX), ('kNXVSmall', GC.NXV_SMALL), ('kNXVLarge', GC.NXV_LARGE)):
        assert int(re.search(rf'constexpr int {name} = (\d+);', a).group(1)) == v, name
    assert re.search(r'PK_COPY = (\d),.*\n\s*PK_NORM = (\d),.*\n\s*PK_QUANT = (\d)', a).groups() == ('0', '1', '2')
    assert re.search(r'EK_PLAIN = (\d),.*\n\s*EK_SWIGLU = (\d)', a).groups() == ('0', '1')
    k = src('kernels.h')
    for name, v in (('W_FP16', 0), ('W_INT8_WOQ', 1), ('W_INT4_WOQ', 2), ('W_INT8_SQ', 3), ('PRO_NONE', 0), ('PRO_RMSNORM', 1),
                    ('PRO_RMSNORM_QSTATIC', 2), ('PRO_RMSNORM_QDYN', 3), ('PRO_QSTATIC', 4), ('PRO_QDYN', 5), ('EPI_NONE', 0),
                    ('EPI_RESIDUAL', 1), ('EPI_SWIGLU', 2), ('EPI_SWIGLU_QSTATIC', 3), ('DT_FLOAT', 0), ('DT_HALF', 1), ('DT_INT8', 2),
                    ('DT_INT32', 3)):
        assert re.search(rf'\b{name} = {v}\b', k), name
    impl = src('gemv_impl.h')
    for wt, vec in (('W_FP16', 8), ('W_INT8_WOQ', 16), ('W_INT4_WOQ', 32), ('W_INT8_SQ', 16)):
        m = re.search(rf'struct WTraits<{wt}>\s*\{{\s*static constexpr int VEC = (\d+);', impl)
        assert int(m.group(1)) == vec == GC.VEC[getattr(GC, wt)]


def test_launch_gemv_is_what_the_mirror_restates():
    """gemv.hip launch_gemv: the order matrix pipe -> slab split -> refusals -> K-split -> the kernel of the weight type, the slab
    rule with its 160 KiB and what it re-offsets, the K limits"""
    g = _squash(_body(src('gemv.hip'), 'int launch_gemv(const GemvParams& p, hipStream_t stream)'))
    order = ['if (p.M < 1 || p.M > 8 || p.N <= 0 || p.K <= 0)', 'if (sq && p.M >= 2)', 'launch_gemv_mfma_sq(p, stream)',
             'const int es = sq ? 1 : 2;', 'const int64_t kp = (p.K + 31) / 32 * 32;',
             'int mb = p.M <= 1 ? 1 : (p.M <= 2 ? 2 : (p.M <= 4 ? 4 : 8));',
             'while (fit > 1 && kRedBytes + (int64_t) fit * kp * es > 160 * 1024) fit >>= 1;', 'if (fit < mb)',
             'for (int m0 = 0; m0 < p.M; m0 += fit)', 'q.M = p.M - m0 < fit ? p.M - m0 : fit;',
             'q.x = static_cast<const char*>(p.x) + (int64_t) m0 * p.ldx * (raw_s8 ? 1 : 2);',
             'q.y = static_cast<char*>(p.y) + (int64_t) m0 * p.ldy * yes;',
             'q.residual = static_cast<const char*>(p.residual) + (int64_t) m0 * p.ldy * 2;',
             'q.scale_row = p.scale_row + m0;', 'q.dyn_scale_out = p.dyn_scale_out + m0;',
             'q.x_pro_out = static_cast<char*>(p.x_pro_out) + (int64_t) m0 * p.K * es;', 'if (launch_gemv(q, stream))',
             'if (!sq && quant_pro)', 'if (sq && p.pro == PRO_RMSNORM)', 'const int xvec = raw_s8 ? 16 : 8;',
             'const int nxv_lim = ((pk == PK_COPY || pk == PK_QUANT) && !swiglu) ? kNXVLarge : kNXVMax;',
             'if ((p.K % xvec) || p.K > 256 * xvec * nxv_lim)', 'a.Kp = (int32_t) layout::round_up(p.K, vec);',
             'a.nchunks = (a.Kp + 64 * vec - 1) / (64 * vec);', 'a.ngroups = swiglu ? p.N : (p.N + R - 1) / R;',
             'if (gemv_ksplit_applies(a)) return launch_gemv_ksplit(a, stream);', 'launch_gemv_fp16(a, pk, swiglu, stream)',
             'launch_gemv_woq8(a, pk, swiglu, stream)', 'launch_gemv_woq4(a, pk, swiglu, stream)', 'launch_gemv_sq(a, pk, swiglu, stream)']
    at = -1
    for piece in order:
        nxt = g.find(piece, at + 1)
        assert nxt > at, f'launch_gemv no longer reads (in this order): {piece}'
        at = nxt
    assert GC.LDS_LIMIT == 160 * 1024
    for tu, wt in (('gemv_fp16.hip', 'W_FP16'), ('gemv_woq8.hip', 'W_INT8_WOQ'), ('gemv_woq4.hip', 'W_INT4_WOQ'), ('gemv_sq.hip', 'W_INT8_SQ')):
        assert f'launch_wt<{wt}>(a, pk, swiglu, stream)' in src(tu), tu


def arms():
    """the instances gemv_impl.h builds, from the text of launch_wt / launch_nxv / launch_mb:
    (families {(PK, EK)} every weight type has, families only SmoothQuant has, the NXV of launch_nxv in order with the condition of
    the last, the (MB, UU) of launch_mb)"""
    impl = src('gemv_impl.h')
    wt = _body(impl, 'int launch_wt(const GemvArgs& a, int pk, bool swiglu, hipStream_t stream)')
    fam = re.findall(r'(if constexpr \(SQ\)\s*)?return launch_nxv<WT, (PK_\w+), (EK_\w+)>\(a, stream\);', wt)
    everyone = {(getattr(GC, pk), getattr(GC, ek)) for sq, pk, ek in fam if not sq}
    sq_only = {(getattr(GC, pk), getattr(GC, ek)) for sq, pk, ek in fam if sq}
    nxv = _squash(_body(impl, 'int launch_nxv(const GemvArgs& a, hipStream_t stream)'))
    assert 'const int xvec = (WT == W_INT8_SQ && PK == PK_COPY) ? 16 : 8;' in nxv
    steps = re.findall(r'(if \(a\.p\.K <= 256 \* xvec \* (kNXV\w+)\)|if constexpr \(\(PK == PK_COPY \|\| PK == PK_QUANT\) && EK == EK_PLAIN\)) '
                       r'return launch_mb<WT, PK, EK, (kNXV\w+)>\(a, stream\);', nxv)
    assert len(steps) == len(re.findall(r'launch_mb<', nxv))
    mb = _squash(_body(impl, 'int launch_mb(const GemvArgs& a, hipStream_t stream)'))
    insts = re.findall(r'launch_inst<WT, PK, EK, (\d), NXV(?:, (\d))?>\(a, stream\)', mb)
    return everyone, sq_only, steps, insts, mb


def test_the_arms_of_the_kernel_dispatch_are_what_the_mirror_restates():
    everyone, sq_only, steps, insts, mb = arms()
    assert everyone == set(GC.families(GC.W_FP16)) == set(GC.families(GC.W_INT8_WOQ)) == set(GC.families(GC.W_INT4_WOQ))
    assert everyone | sq_only == set(GC.families(GC.W_INT8_SQ)) and sq_only == {(GC.PK_QUANT, GC.EK_PLAIN)}
    # launch_nxv: K <= 256 xvec kNXVSmall, then <= 256 xvec kNXVMax, then kNXVLarge for the plain copy / quantiser families only
    assert [(s[1], s[2]) for s in steps] == [('kNXVSmall', 'kNXVSmall'), ('kNXVMax', 'kNXVMax'), ('', 'kNXVLarge')]
    assert GC.buckets(GC.PK_COPY, GC.EK_PLAIN) == GC.buckets(GC.PK_QUANT, GC.EK_PLAIN) == (GC.NXV_SMALL, GC.NXV_MAX, GC.NXV_LARGE)
    assert GC.buckets(GC.PK_NORM, GC.EK_PLAIN) == GC.buckets(GC.PK_COPY, GC.EK_SWIGLU) == GC.buckets(GC.PK_NORM, GC.EK_SWIGLU) \
        == (GC.NXV_SMALL, GC.NXV_MAX)
    # launch_mb: 1 (int4 rows of at most two chunks: the 2-chunk form) / 2 / 4 / 8
    assert insts == [('1', '2'), ('1', ''), ('2', ''), ('4', ''), ('8', '')]
    for piece in ('if (a.p.M <= 1)', 'if constexpr (WT == W_INT4_WOQ) if (a.nchunks <= 2) return launch_inst<WT, PK, EK, 1, NXV, 2>',
                  'if (a.p.M <= 2) return launch_inst<WT, PK, EK, 2, NXV>', 'if (a.p.M <= 4) return launch_inst<WT, PK, EK, 4, NXV>'):
        assert piece in mb, piece
    assert 'const size_t smem = kRedBytes + (size_t) MB * a.Kp * (WT == W_INT8_SQ ? 1 : 2);' in src('gemv_impl.h')


def test_the_ksplit_conditions_are_what_the_mirror_restates():
    k = src('gemv_ksplit.hip')
    assert 'static constexpr int RW = WT == W_INT8_SQ ? 2 : 4;' in k
    assert 'static constexpr int NCMAX = WT == W_FP16 ? 6 : (WT == W_INT4_WOQ ? 2 : 3);' in k
    for wt in GC.WTS:
        assert GC.KSPLIT_RW[wt] == (2 if wt == GC.W_INT8_SQ else 4)
        assert GC.KSPLIT_NCMAX[wt] == (6 if wt == GC.W_FP16 else (2 if wt == GC.W_INT4_WOQ else 3))
    assert ('return a.nchunks > 4 && a.nchunks <= 4 * KSplit<WT>::NCMAX && (a.p.K % KSplit<WT>::VEC) == 0 && a.p.N <= '
            f'{GC.KSPLIT_NMAX};') in k
    ap = _squash(_body(k, 'bool gemv_ksplit_applies(const GemvArgs& a)'))
    assert ('if (p.M != 1 || p.pro != PRO_NONE || !(p.epi == EPI_NONE || p.epi == EPI_RESIDUAL) || p.x_pro_out || p.dyn_scale_out '
            '|| p.per_token) return false;') in ap
    assert ('if (!(p.out_dtype == DT_HALF || p.out_dtype == DT_FLOAT || (p.out_dtype == DT_INT32 && p.wtype == W_INT8_SQ))) '
            'return false;') in ap
    la = _squash(_body(k, 'int launch_gemv_ksplit(const GemvArgs& a, hipStream_t stream)'))
    assert 'const int per_wave = (a.nchunks + 3) / 4;' in la
    assert 'if (per_wave < NC) return launch_nc<WT, NC - 1>(a, per_wave, stream);' in _squash(k)
    for wt in ('W_FP16', 'W_INT8_WOQ', 'W_INT4_WOQ', 'W_INT8_SQ'):
        assert f'launch_nc<{wt}, KSplit<{wt}>::NCMAX>(a, per_wave, stream)' in la


def test_the_matrix_pipe_conditions_are_what_the_mirror_restates():
    m = src('gemv_mfma_sq.hip')
    assert f'constexpr int kRows = {GC.MFMA_KROWS};' in m
    la = _squash(_body(m, 'int launch_gemv_mfma_sq(const GemvParams& p, hipStream_t stream)'))
    for piece in (f'gemv_mfma_min_rows = {GC.MFMA_ROWS_DEFAULT};',
                  'if (gemv_mfma_min_rows <= 0 || p.M < gemv_mfma_min_rows || p.M > kRows || p.wtype != W_INT8_SQ) return 1;',
                  'const bool norm = p.pro == PRO_RMSNORM_QSTATIC;', 'if (!norm && p.pro != PRO_NONE) return 1;',
                  'if (p.per_token || p.x_pro_out || p.dyn_scale_out || !p.scale_col) return 1;',
                  'if ((p.N & 15) || (p.K & 255) || (p.ldw & 15) || (reinterpret_cast<uintptr_t>(p.w) & 15) || (p.ldy & 3)) return 1;',
                  'if (p.epi == EPI_RESIDUAL && (!p.residual || p.out_dtype != DT_HALF',
                  '|| ((p.ldx * 2) & 15)', '|| p.K > 256 * 8 * kNXVMax) return 1;', 'else if ((reinterpret_cast<uintptr_t>(p.x) & 15) || (p.ldx & 15)) return 1;',
                  'const int pitch = p.K + 16;', 'const int ngroups = p.N / 16;'):
        assert piece in la, piece
    de = _squash(_body(m, 'int launch_depth(const GemvParams& p, int pitch, int ngroups, int cus, hipStream_t stream)'))
    for piece in ('constexpr int SLOT = (SWIGLU ? 8 : 4) * 1024;',
                  'const size_t fixed = kRedBytes + 2 * (SWIGLU ? 2 : 1) * 4 * 64 * 16 + (size_t) (kRows + 1) * pitch;',
                  'if constexpr (!SWIGLU) { if (fixed + 4 * 4 * SLOT <= 160 * 1024) return go(std::integral_constant<int, 4>()); }',
                  'if (fixed + 4 * 3 * SLOT <= 160 * 1024) return go(std::integral_constant<int, 3>());',
                  'if (fixed + 4 * 2 * SLOT <= 160 * 1024) return go(std::integral_constant<int, 2>());', 'return 1;'):
        assert piece in de, piece
    # the depths the mirror derives from that: the K at which each ring stops fitting
    assert [GC.mfma_depth(k, False) for k in (9728, 9984, 11520, 11776, 13568, 13824)] == [4, 3, 3, 2, 2, 0]
    assert [GC.mfma_depth(k, True) for k in (5376, 5632, 8960, 9216)] == [3, 2, 2, 0]


def _flat(inst):
    return [i for s in inst[2] for i in _flat(s)] if inst[0] == 'slab' else [inst]


def covered(cases):
    return {i for c in cases for i in _flat(GC.instance(c))}


def missing(cases):
    have = covered(cases)
    return sorted((GC.reachable_valu() | GC.reachable_ksplit() | GC.reachable_mfma()) - have, key=str)


def test_the_reachable_instances_are_the_arms_that_fit_the_lds():
    """reachable_valu() against the arms: every (WT, family, bucket, MB) of the source except those whose smallest K does not fit
    the LDS with MB rows (launch_gemv cuts those calls into slabs), with the 2-chunk form where int4 K <= 4096.  And the mirror
    reaches each of them at that smallest K (N > 8192 and no matrix pipe, so that neither one-shot kernel takes the call)."""
    everyone, sq_only, steps, insts, _ = arms()
    reach = GC.reachable_valu()
    n_arms = 0
    for wt in GC.WTS:
        for pk, ek in sorted(everyone | (sq_only if wt == GC.W_INT8_SQ else set())):
            for nxv in GC.buckets(pk, ek):
                for mb in sorted({int(m) for m, _ in insts}):
                    n_arms += 1
                    lo, hi = GC.bucket_k(wt, pk, nxv)
                    es = 1 if wt == GC.W_INT8_SQ else 2
                    fits = GC.RED_BYTES + mb * GC.round_up(lo, 32) * es <= GC.LDS_LIMIT
                    mine = {i for i in reach if i[1:6] == (wt, pk, ek, mb, nxv)}
                    assert bool(mine) == fits, (wt, pk, ek, mb, nxv)
                    if not fits:
                        continue
                    pro = {GC.PK_COPY: GC.PRO_NONE, GC.PK_NORM: GC.PRO_RMSNORM_QDYN if es == 1 else GC.PRO_RMSNORM, GC.PK_QUANT: GC.PRO_QDYN}[pk]
                    c = GC.Case(wt=wt, pro=pro, epi=GC.EPI_SWIGLU if ek else GC.EPI_NONE, M=mb, N=8200, K=lo, mfma_rows=0)
                    assert GC.instance(c) in mine, (c, GC.instance(c))
    # 4 weight types x (3 + 2 + 2 + 2 [+ 3 SmoothQuant quantiser]) buckets x 4 row buckets = 156 arms; MB = 8 of the third bucket of
    # the copy family (fp16 activations: 8 x 12296 x 2 bytes; raw s8: 8 x 24592) does not fit: 152 reachable
    assert n_arms == 156 and len(reach) == 152
    assert {i[6] for i in reach if i[1] == GC.W_INT4_WOQ and i[4] == 1 and i[5] == GC.NXV_SMALL} == {2}
    assert {i[6] for i in reach if not (i[1] == GC.W_INT4_WOQ and i[4] == 1 and i[5] == GC.NXV_SMALL)} == {GC.U}


def test_every_reachable_instance_has_a_case():
    """every (WT, PK, EK, MB, NXV, UU) the kernel dispatch can produce, every NC of every K-split weight type, every matrix-pipe
    depth x SwiGLU form, and a slab case per weight type"""
    assert not missing(GC.CASES), f'instances without a case: {missing(GC.CASES)}'
    slabs = {c.wt for c in GC.CASES if GC.instance(c)[0] == 'slab'}
    assert slabs == set(GC.WTS)
    ids = [GC.case_id(c) for c in GC.CASES]
    assert len(ids) == len(set(ids))


def test_deleting_the_sole_case_of_an_instance_fails_the_table():
    """the check above has teeth: without the only case of an instance, that instance is reported"""
    sole = {}
    for c in GC.CASES:
        for i in _flat(GC.instance(c)):
            sole.setdefault(i, []).append(c)
    only = {i: cs[0] for i, cs in sole.items() if len(cs) == 1 and i[0] != 'refused'}
    assert len(only) >= 20
    for i, c in only.items():
        assert missing([x for x in GC.CASES if x != c]) == [i], (i, c)


def test_the_table_holds_the_edges_the_kernels_can_get_wrong():
    cases = GC.CASES
    inst = {c: GC.instance(c) for c in cases}
    ok = [c for c in cases if inst[c][0] != 'refused']
    for wt in GC.WTS:
        mine = [c for c in ok if c.wt == wt]
        assert {c.M for c in mine} >= {1, 2, 3, 4, 5, 7, 8}, wt
        ks = {c.K for c in mine}
        assert ks >= {64, 11008 if wt != GC.W_INT8_SQ else 22016}, (wt, sorted(ks))
        # both sides of the bucket boundaries (raw s8 activations: 16 per vector, so twice the K)
        assert ks >= {4096, 4104, 12288, 12296}, (wt, sorted(ks))
        assert {c.epi for c in mine} >= {GC.EPI_NONE, GC.EPI_RESIDUAL, GC.EPI_SWIGLU}
        assert {GC.out_dtype(c) for c in mine} >= {GC.DT_HALF, GC.DT_FLOAT}
        assert any(c.strided for c in mine) and any(inst[c][0] == 'slab' for c in mine)
        assert any(c.blocks_per_cu == 1 and c.N > 6000 for c in mine)
        if wt in (GC.W_INT8_WOQ, GC.W_INT4_WOQ):
            # a DC offset in the activations for every family of the weight-only kernels, and K = 8 * odd (Kp > K)
            fam = {i[2:4] for c in mine if c.dc for i in _flat(inst[c]) if i[0] == 'valu'}
            assert fam == set(GC.families(wt)), (wt, fam)
            assert any((c.K // 8) % 2 == 1 and GC.round_up(c.K, GC.VEC[wt]) > c.K for c in mine)
    # several row groups per wave: the plain and the SwiGLU form
    assert {GC.is_swiglu(c) for c in ok if c.blocks_per_cu == 1 and c.N > 6000} == {False, True}
    sqc = [c for c in ok if c.wt == GC.W_INT8_SQ]
    assert {c.K for c in sqc if c.pro == GC.PRO_NONE} >= {8192, 8208, 24576, 24592}
    assert {c.per_channel for c in sqc} == {0, 1} and {GC.out_dtype(c) for c in sqc} >= {GC.DT_INT32, GC.DT_INT8}
    assert {c.pro for c in sqc} == {GC.PRO_NONE, GC.PRO_RMSNORM_QSTATIC, GC.PRO_RMSNORM_QDYN, GC.PRO_QSTATIC, GC.PRO_QDYN}
    # per-token scale_row[M] at 3, 5 and 8 rows, the last through a slab
    tok = {(c.M, inst[c][0]) for c in sqc if c.per_token}
    assert {m for m, _ in tok} >= {3, 5, 8} and (8, 'slab') in tok
    # side outputs across a slab boundary: 7 rows of K = 22016 behind the per-token quantiser
    assert any(c.M == 7 and c.K == 22016 and c.pro == GC.PRO_QDYN and inst[c][0] == 'slab' and GC.has_side(c) for c in sqc)
    assert any(c.M in (3, 4) and c.K == 22016 and inst[c][0] == 'slab' for c in ok if c.wt == GC.W_FP16)
    # SmoothQuant static from 5 rows: at the default (matrix pipe) and with it switched off; what the pipe does not serve stays VALU
    on = {c._replace(name='', mfma_rows=0) for c in sqc if inst[c][0] == 'mfma' and c.mfma_rows < 0}
    off = {c._replace(name='') for c in sqc if c.mfma_rows == 0}
    assert on and on <= off
    assert all(GC.instance(c)[0] == 'valu' for c in off)
    assert {c.M for c in sqc if inst[c][0] == 'mfma' and c.mfma_rows < 0} >= {5, 7, 8}
    for c in ok:
        if c.wt == GC.W_INT8_SQ and c.mfma_rows < 0 and (c.N % 16 or c.K % 256):
            assert 'mfma' not in {i[0] for i in _flat(inst[c])}, c
    assert any(c.M >= 5 and c.N % 16 == 0 and c.K % 256 and inst[c][0] == 'valu' for c in sqc if c.mfma_rows < 0)
    assert any(c.M >= 5 and c.N % 16 and c.K % 256 == 0 and inst[c][0] == 'valu' for c in sqc if c.mfma_rows < 0 and c.pro == GC.PRO_NONE)
    # residual in place: several groups per wave, K-split, matrix pipe, slab
    inp = {('groups' if c.blocks_per_cu else inst[c][0]) for c in ok if c.inplace}
    assert inp >= {'groups', 'ksplit', 'mfma', 'slab'}, inp
    assert all(c.epi == GC.EPI_RESIDUAL for c in ok if c.inplace)
    # K-split: a ragged last workgroup for every instance, N = 1, the largest N and the first that is not served
    for wt in GC.WTS:
        for nc in range(2, GC.KSPLIT_NCMAX[wt] + 1):
            assert any(inst[c] == ('ksplit', wt, nc) and c.N % GC.KSPLIT_RW[wt] for c in ok), (wt, nc)
    assert any(inst[c][0] == 'ksplit' and c.N == 1 for c in ok) and any(inst[c][0] == 'ksplit' and c.N == GC.KSPLIT_NMAX for c in ok)
    assert any(inst[c][0] == 'valu' and c.N == GC.KSPLIT_NMAX + 1 and GC.instance(c._replace(N=GC.KSPLIT_NMAX))[0] == 'ksplit' for c in ok)
    # refusals past the middle bucket for the normalising prologue and the SwiGLU epilogue
    ref = [c for c in cases if inst[c][0] == 'refused']
    assert any(c.K == 12296 and GC.pro_kind(c.pro) == GC.PK_NORM for c in ref) and any(c.K == 12296 and GC.is_swiglu(c) for c in ref)
    # shapes: N ragged against the 2-row groups x 4 waves unless the matrix pipe needs 16
    for c in ok:
        if c.name == 'grid':
            assert 66 <= c.N <= 130 and c.N % 8, c
