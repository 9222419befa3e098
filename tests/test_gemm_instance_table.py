"""No GPU: the case table of tests/test_gpu_gemm_instances.py (tests/gemm_cases.py) against the host code of the prefill GEMMs as
the source states it - the constants and conditions the Python mirror gemm_cases.instance() depends on are read from the source
text (gemm.hip, gemm_glds.hip, gemm_sqp.hip, gemm_woq.hip, gemm_mfma.hip, gemm_tactics.hip, runtime/kernel_api.cpp) and fail here
when they move; then every kernel id a `case` label can launch and every branch of the fall-back chain must have a case."""
import os
import re

import gemm_cases as GC

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'trtllm-llama_amd', 'csrc')


def src(name):
    text = open(os.path.join(CSRC, name if '/' in name else os.path.join('kernels', name))).read()
    return re.sub(r'//[^\n]*', '', text)  # without the comments


def _body(text, head):
    """the text of the function whose definition starts with `head`, up to its closing brace at column 0"""
    i = text.index(head)
    return text[i:text.index('\n}\n', i)]


def _squash(s):
    return re.sub(r'\s+', ' ', s)


def _ints(s):
    """template arguments: integers, sums of integers, true / false"""
    return tuple(int(eval(t, {'__builtins__': {}}, {'true': 1, 'false': 0})) for t in s.split(','))


def _in_order(text, pieces, what):
    at = -1
    for piece in pieces:
        nxt = text.find(piece, at + 1)
        assert nxt > at, f'{what} no longer reads (in this order): {piece}'
        at = nxt


def _case_groups(body, call):
    """[(labels, [template argument tuples])] of a switch: consecutive `case N:` labels and the `call<...>` launches behind them"""
    groups, labels, launches = [], [], []
    for m in re.finditer(r'case (\d+):|' + call + r'<([^>]*)>\(|default:', body):
        if m.group(0) == 'default:':
            break
        if m.group(1):
            if launches:
                groups.append((labels, launches))
                labels, launches = [], []
            labels.append(int(m.group(1)))
        elif labels:
            launches.append(m.group(2))
    if launches:
        groups.append((labels, launches))
    return groups


# ---------------------------------------------------------------------------------------------- gemm_glds.hip
def test_the_lock_step_table_and_the_static_rule_are_what_the_mirror_restates():
    g = src('gemm_glds.hip')
    wt = _squash(_body(g, 'int launch_wt(const GemmParams& p, int cfg, hipStream_t stream)'))
    table = {}
    for labels, launches in _case_groups(wt, 'launch_cfg'):
        assert len(labels) == 1 and len(launches) == 1
        a = _ints(launches[0].replace('WT,', '', 1))
        table[labels[0]] = a + (0, ) * (8 - len(a))
    assert table == GC.GLDS, 'the case labels of launch_wt moved'
    assert 'default: return launch_cfg<WT, 2, 2, 2, 2, 1, 128, 4>(p, stream);' in wt and GC.GLDS[8][:7] == (2, 2, 2, 2, 1, 128, 4)
    assert 'constexpr int BM = WM * MT * 32, BN = WN * NT * 32;' in g
    assert f'constexpr int kNumCfg = {GC.NUM_CFG};' in g and f'constexpr int kPhased256x128 = {GC.PHASED_256x128};' in g
    shapes = re.search(r'constexpr Shape kShapes\[\] = \{(.*?)\};', _squash(g)).group(1)
    got = tuple((GC.PHASED_256x128 if i == 'kPhased256x128' else int(i), int(bm), int(bn), float(f), float(fs))
                for i, bm, bn, f, fs in re.findall(r'\{(\w+), (\d+), (\d+), ([\d.]+), ([\d.]+)\}', shapes))
    assert got == GC.SHAPES, 'kShapes moved'
    for i, bm, bn, _, _ in GC.SHAPES:  # the rule's tile sizes are the kernels'
        assert (bm, bn) == (GC.glds_tile(i) if i in GC.GLDS else GC.sqp_tile(GC.SQP[i]))
    sv = _squash(_body(g, 'static bool glds_serves(const GemmParams& p)'))
    _in_order(sv, ['if (!sq && p.wtype != W_FP16) return false;', 'const int es = sq ? 1 : 2;',
                   '((p.lda * es) & 15)', '(p.ldw & 15) || ((p.K * es) % 128) || p.K <= 0 || p.M < 32) return false;',
                   'if (!sq && p.out_dtype == DT_INT32) return false;',
                   'if (p.residual && (p.out_dtype != DT_HALF || (p.ldc & 7) || (p.N & 7)',
                   'if (p.silu_gate && (sq || p.residual || p.out_dtype != DT_HALF || (p.ldc & 7) || (p.N & 7)', 'return true;'], 'glds_serves')
    st = _squash(_body(g, 'static int static_shape_cfg(const GemmParams& p, bool phased_ok = true)'))
    _in_order(st, ['int cfg = 8;', 'if (s.id == kPhased256x128 && !phased_ok) continue;',
                   'const int64_t tiles = (int64_t) ((p.M + s.bm - 1) / s.bm) * ((p.N + s.bn - 1) / s.bn);',
                   'if (s.id == kPhased256x128 && tiles > 2 * cus) continue;',
                   'const double cost = (double) ((tiles + cus - 1) / cus) * s.bm * s.bn * (p.wtype == W_INT8_SQ ? s.f_sq : s.f);',
                   'if (cost < best)'], 'static_shape_cfg')
    sc = _squash(_body(g, 'int gemm_static_cfg(const GemmParams& p)'))
    _in_order(sc, ['if (!glds_serves(p)) return 0;', 'const int cfg = static_shape_cfg(p);',
                   'const bool persist = p.out_dtype == DT_HALF && !(p.ldc & 7) && !(p.N & 7)',
                   f'&& p.K >= (p.wtype == W_INT8_SQ ? {GC.PERSIST_MIN_K[GC.W_INT8_SQ]} : {GC.PERSIST_MIN_K[GC.W_FP16]});',
                   'if (cfg == kPhased256x128) return p.wtype == W_INT8_SQ ? (persist ? 62 : 42) : (persist ? 56 : 54);',
                   'return cfg == 6 ? (p.wtype == W_INT8_SQ ? (persist ? 63 : 20) : (persist ? 55 : 50)) : cfg;'], 'gemm_static_cfg')
    lc = _squash(_body(g, 'int launch_gemm_cfg(const GemmParams& p, int cfg, hipStream_t stream)'))
    _in_order(lc, ['if (!glds_serves(p)) return 1;', 'if ((cfg >= 1 && cfg <= kNumCfg) || cfg == 36 || cfg == 37)',
                   'return sq ? launch_wt<W_INT8_SQ>(p, cfg, stream) : launch_wt<W_FP16>(p, cfg, stream);',
                   'return sq ? launch_gemm_sqp(p, cfg, stream) : launch_gemm_f16p(p, cfg, stream);'], 'launch_gemm_cfg')
    assert set(GC.GLDS) == set(range(1, GC.NUM_CFG + 1)) | {36, 37}


def test_launch_gemm_glds_is_the_chain_the_mirror_restates():
    lg = _squash(_body(src('gemm_glds.hip'), 'int launch_gemm_glds(const GemmParams& p, hipStream_t stream)'))
    _in_order(lg, ['if (!glds_serves(p)) return 1;', 'int cfg = gemm_tune_cfg;', 'if (cfg <= 0)',
                   'cfg = gemm_tactic_lookup(p.wtype, p.M, p.N, p.K);', 'from_table = cfg > 0;',
                   'const bool glds_id = (cfg >= 1 && cfg <= kNumCfg) || cfg == 36 || cfg == 37;', 'if (cfg > kNumCfg && !glds_id)',
                   'const int r = sq ? launch_gemm_sqp(p, cfg, stream) : launch_gemm_f16p(p, cfg, stream);', 'if (r <= 0) return r;', 'cfg = 0;',
                   'if (cfg <= 0 || !((cfg >= 1 && cfg <= kNumCfg) || cfg == 36 || cfg == 37))', 'cfg = static_shape_cfg(p);',
                   'if (cfg == kPhased256x128)', 'int r = sq ? launch_gemm_sqp(p, 62, stream) : launch_gemm_f16p(p, 56, stream);',
                   'if (r > 0) r = sq ? launch_gemm_sqp(p, 42, stream) : launch_gemm_f16p(p, 54, stream);', 'if (r <= 0) return r;',
                   'cfg = static_shape_cfg(p, false);', 'if (!sq && cfg == 6 && gemm_tune_cfg <= 0 && !from_table)',
                   'int r = launch_gemm_f16p(p, 55, stream);', 'if (r > 0) r = launch_gemm_f16p(p, 50, stream);',
                   'if (sq && cfg == 6 && gemm_tune_cfg <= 0 && !from_table)', 'int r = launch_gemm_sqp(p, 63, stream);',
                   'if (r > 0) r = launch_gemm_sqp(p, 20, stream);',
                   'return sq ? launch_wt<W_INT8_SQ>(p, cfg, stream) : launch_wt<W_FP16>(p, cfg, stream);'], 'launch_gemm_glds')


def test_launch_gemm_is_the_chain_the_mirror_restates():
    lg = _squash(_body(src('gemm.hip'), 'int launch_gemm(const GemmParams& pin, hipStream_t stream)'))
    _in_order(lg, ['if (pin.M <= 0) return 0;', 'if (pin.residual && pin.out_dtype != DT_HALF)',
                   'if (pin.silu_gate && (pin.residual || pin.out_dtype != DT_HALF))', 'if (pin.silu_gate && pin.wtype == W_INT8_SQ)',
                   'if (pin.ldc != pin.N)', 'q.silu_gate = nullptr;', 'const int rc = launch_gemm(q, stream);',
                   'return rc ? rc : launch_swiglu(pin.c, pin.silu_gate, pin.c, (int64_t) pin.M * pin.N, stream);', 'if (pin.M > 8)',
                   'const bool woq = pin.wtype == W_INT8_WOQ || pin.wtype == W_INT4_WOQ;', 'const int r = launch_gemm_woq(pin, stream);',
                   'if (r <= 0) return r;', 'const int r = launch_gemm_glds(pin, stream);', 'if (r <= 0) return r;',
                   'if (pin.silu_gate && pin.ldc != pin.N)', 'if (pin.residual && (pin.ldc != pin.N || pin.residual == pin.c))',
                   'return launch_add(pin.c, pin.c, pin.residual, (int64_t) pin.M * pin.N, stream);',
                   'return launch_swiglu(pin.c, pin.silu_gate, pin.c, (int64_t) pin.M * pin.N, stream);', 'if (p.M > 8)',
                   'const int r = launch_gemm_mfma(p, stream);', 'if (r <= 0) return finish(r);', 'for (int m0 = 0; m0 < p.M; m0 += 8)',
                   'const int rows = p.M - m0 < 8 ? p.M - m0 : 8;', 'if (gemv_slab(p, m0, rows, stream))', 'return finish(0);'], 'launch_gemm')


# ---------------------------------------------------------------------------------------------- gemm_sqp.hip
_SQP_DEFAULTS = (0, 0, 0, 1, 0, 0, 0)  # ABL, RSP, DUAL, SCL, F16, PERSIST, KSPLIT


def _sqp_table(body):
    """id -> the 14 template arguments of launch_sqp"""
    out = {}
    for labels, launches in _case_groups(body, 'launch_sqp'):
        assert len(labels) == len(launches), (labels, launches)  # `case 60: case 62: ... cfg == 60 ? A : B`
        for i, l in zip(labels, launches):
            a = _ints(l)
            out[i] = a + _SQP_DEFAULTS[len(a) - 7:]
    return out


def test_the_phased_tables_are_what_the_mirror_restates():
    s = src('gemm_sqp.hip')
    assert 'constexpr int BM = 2 * WR * MTH * 16, BN = 2 * WC * NTH * 16;' in s
    sq = _sqp_table(_squash(_body(s, 'int launch_gemm_sqp(const GemmParams& pin, int cfg, hipStream_t stream)')))
    f16 = _sqp_table(_squash(_body(s, 'int launch_gemm_f16p(const GemmParams& pin, int cfg, hipStream_t stream)')))
    # the ablations (wrong results on purpose) are the ids whose ABL is not one of 0 / 16 (16 = non-temporal stores): exactly 21-27, 31-33
    assert tuple(sorted(i for i, a in sq.items() if a[7] not in (0, 16))) == GC.ABLATIONS
    assert all(a[7] in (0, 16) for a in f16.values())
    pick = lambda a: a[:4] + (a[12], a[13])
    assert {i: pick(a) for i, a in sq.items() if i not in GC.ABLATIONS} == GC.SQP, 'the case labels of launch_gemm_sqp moved'
    assert {i: pick(a) for i, a in f16.items()} == GC.F16P, 'the case labels of launch_gemm_f16p moved'
    assert all(a[11] == 0 and a[9] == 0 for a in sq.values()) and all(a[11] == 1 and a[9] == 0 for a in f16.values())
    assert not (set(GC.SQP) | set(GC.F16P) | set(GC.ABLATIONS)) & set(GC.GLDS)
    assert max(set(GC.SQP) | set(GC.F16P)) <= 65  # tllm_gemm_kernel hands 1..65 to launch_gemm_cfg


def test_the_phased_serve_conditions_are_what_the_mirror_restates():
    s = src('gemm_sqp.hip')
    vec = "(p.out_dtype != DT_HALF || (p.ldc & 7) || (p.N & 7) || (reinterpret_cast<uintptr_t>(p.c) & 15) || (reinterpret_cast<uintptr_t>(p.residual) & 15)"
    sq = _squash(_body(s, 'int launch_gemm_sqp(const GemmParams& pin, int cfg, hipStream_t stream)'))
    _in_order(sq, ['if (p.wtype != W_INT8_SQ || p.silu_gate) return 1;',
                   '(p.lda & 15)', '(p.ldw & 15) || (p.K % 128) || p.K <= 0 || p.M < 32) return 1;',
                   'if ((int64_t) p.M * p.lda >= (1ll << 31) || (int64_t) p.N * p.ldw >= (1ll << 31)) return 1;',
                   'if (p.residual && ' + vec + ')) return 1;', 'switch (cfg)',
                   'case 60: case 62: if ' + vec + f' || p.K < {GC.PERSIST_MIN_K[GC.W_INT8_SQ]}) return 1;',
                   'case 64: if ' + vec + ') return 1;', 'case 65: if ' + vec + ') return 1;',
                   'case 63: if ' + vec + f' || p.K < {GC.PERSIST_MIN_K[GC.W_INT8_SQ]}) return 1;', 'default: return 1;'], 'launch_gemm_sqp')
    vg = vec + ' || (reinterpret_cast<uintptr_t>(p.silu_gate) & 15)'
    f16 = _squash(_body(s, 'int launch_gemm_f16p(const GemmParams& pin, int cfg, hipStream_t stream)'))
    _in_order(f16, ['if (p.wtype != W_FP16 || p.out_dtype == DT_INT32) return 1;', '((p.lda * 2) & 15)',
                    '(p.ldw & 15) || ((p.K * 2) % 128) || p.K <= 0 || p.M < 32) return 1;',
                    'if ((int64_t) p.M * p.lda * 2 >= (1ll << 31) || (int64_t) p.N * p.ldw >= (1ll << 31)) return 1;',
                    'if (p.residual && ' + vec + ')) return 1;',
                    'if (p.silu_gate && (p.residual || p.out_dtype != DT_HALF || (p.ldc & 7) || (p.N & 7)', 'switch (cfg)',
                    'case 55: case 56: if ' + vg + f' || p.K < {GC.PERSIST_MIN_K[GC.W_FP16]}) return 1;',
                    'case 57: if ' + vg + ') return 1;', 'case 58: if ' + vg + ') return 1;', 'default: return 1;'], 'launch_gemm_f16p')
    la = _squash(s[s.index('int launch_sqp(const GemmParams& pin, hipStream_t stream)'):s.index('bool gemm_swiglu_one_tile')])
    _in_order(la, ['constexpr int BNO = DUAL ? BN / 2 : BN;', 'const int tiles = ((p.M + BM - 1) / BM) * ((p.N + BNO - 1) / BNO);',
                   'if (PERSIST)', 'const int rounds = (tiles + cus - 1) / cus;', 'grid = (tiles + rounds - 1) / rounds;',
                   'if constexpr (KSPLIT)', 'const int per_cu = launch_util::blocks_per_cu(reinterpret_cast<const void*>(kfn), 64 * WR * WC, smem);',
                   f'if (2 * tiles > cus * per_cu || p.K * (F16 ? 2 : 1) / 128 < {GC.SPLITK_MIN_KTILES}) return 1;', 'grid = 2 * tiles;',
                   'if (tiles * 2 * 4 > kKsplitFlagBytes) return 1;', 'hipLaunchKernelGGL(kfn, dim3(grid)'], 'launch_sqp')
    assert f'constexpr int kKsplitFlagBytes = {GC.SPLITK_FLAG_BYTES};' in s
    # LDS per workgroup of the split-K forms bounds the workgroups per CU the mirror assumes: 160 KiB / smem
    for i, table, scl in ((64, GC.SQP, 1), (65, GC.SQP, 1), (57, GC.F16P, 0), (58, GC.F16P, 0)):
        bm, bn = GC.sqp_tile(table[i])
        smem = 2 * (bm + bn) * 128 + scl * (bm + bn) * 4
        assert 160 * 1024 // smem == GC.SPLITK_PER_CU[i], i
    assert 'constexpr size_t smem = (size_t) 2 * (BM + BN) * 128 + (SCL ? (BM + BN) * 4 : 0) * (PERSIST ? 2 : 1)' in s
    sw = _squash(_body(s, 'int launch_gemm_swiglu(const GemmParams& p, hipStream_t stream)'))
    _in_order(sw, ['if (p.wtype != W_INT8_SQ || !p.w2 || !p.scale_col2 || !p.swiglu_qscale || p.per_token || p.residual) return 1;',
                   '(p.lda & 15)', '(p.ldw & 15) || (p.K % 128) || p.K <= 0 || p.M < 32) return 1;',
                   'if ((int64_t) p.M * p.lda >= (1ll << 31) || (int64_t) p.N * p.ldw >= (1ll << 31)) return 1;',
                   'if (!(p.ldc & 15) && !(p.N & 15) && !(reinterpret_cast<uintptr_t>(p.c) & 15) && p.K >= 256 && !gemm_swiglu_one_tile)',
                   'return launch_sqp<4, 2, 2, 3, 2, 8, false, 0, 0, true, true, false, true>(p, stream);',
                   'return launch_sqp<4, 2, 2, 3, 0, 6, false, 0, 0, true>(p, stream);'], 'launch_gemm_swiglu')


# ---------------------------------------------------------------------------------------------- gemm_woq.hip, gemm_mfma.hip
def test_the_weight_only_and_register_staged_conditions_are_what_the_mirror_restates():
    w = src('gemm_woq.hip')
    bits = _squash(_body(w, 'int launch_woq_bits(const GemmParams& p, int cfg, hipStream_t stream)'))
    table = {labels[0]: _ints(l[0].replace('BITS,', '', 1)) for labels, l in _case_groups(bits, 'launch_woq_cfg')}
    default = _ints(re.search(r'default: return launch_woq_cfg<BITS, ([\d, ]+)>', bits).group(1))
    assert {**table, 1: default} == GC.WOQ, 'the case labels of launch_woq_bits moved'
    assert 'constexpr int BM = WM * MT * 32, BN = WN * NT * 32;' in w
    sv = _squash(_body(w, 'static bool woq_serves(const GemmParams& p)'))
    _in_order(sv, ['if (!w8 && !w4) return false;', '((p.lda * 2) & 15)',
                   '(p.ldw & 15) || (p.K % 64) || p.K <= 0 || p.M < 32 || !p.scale_col) return false;',
                   'if (p.out_dtype != DT_HALF && p.out_dtype != DT_FLOAT) return false;',
                   'if (p.residual && (p.out_dtype != DT_HALF)) return false;',
                   'if (p.silu_gate && (p.residual || p.out_dtype != DT_HALF || (p.ldc & 7) || (p.N & 7)', 'return true;'], 'woq_serves')
    assert 'if (cfg < 1 || cfg > 6 || !woq_serves(p)) return 1;' in _squash(w)
    lw = _squash(_body(w, 'int launch_gemm_woq(const GemmParams& p, hipStream_t stream)'))
    cands = re.search(r'const Cand cands\[\] = \{(.*?)\};', lw).group(1)
    assert cands == '{1, 256, 192, 1.0}, {6, 256, 128, 1.08}, {2, 128, 128, w8 ? 1.28 : 1.15}'
    assert GC.WOQ_CANDS == ((1, 256, 192, 1.0, 1.0), (6, 256, 128, 1.08, 1.08), (2, 128, 128, 1.28, 1.15))
    for tid, bm, bn, _, _ in GC.WOQ_CANDS:
        assert GC.woq_tile(tid) == (bm, bn)
    _in_order(lw, ['if (!woq_serves(p)) return 1;', 'int cfg = gemm_woq_tune_cfg;', 'if (cfg <= 0)',
                   'const int64_t t = (int64_t) ((p.M + c.bm - 1) / c.bm) * ((p.N + c.bn - 1) / c.bn);',
                   'if (c.id == 6 && t > 2 * cus) continue;', 'const double cost = (double) ((t + cus - 1) / cus) * c.bm * c.bn * c.f;',
                   'if (cost < best)'], 'launch_gemm_woq')
    m = _squash(_body(src('gemm_mfma.hip'), 'int launch_gemm_mfma(const GemmParams& p, hipStream_t stream)'))
    _in_order(m, ['const int a_es = sq ? 1 : 2;', '((p.lda * a_es) & 15)', '(p.ldw & 15)) return 1;', 'if ((p.K * a_es) % 16) return 1;',
                  'if (p.wtype == W_INT8_WOQ && (p.K % 16)) return 1;', 'if (p.wtype == W_INT4_WOQ && (p.K % 32)) return 1;',
                  'if (!sq && p.out_dtype == DT_INT32) return 1;'], 'launch_gemm_mfma')
    assert 'constexpr int BM = 128, BN = 128, BKB = 64;' in src('gemm_mfma.hip')


def test_the_entry_points_and_the_tactic_lists_are_what_the_mirror_restates():
    k = _squash(_body(src('runtime/kernel_api.cpp'), 'int32_t tllm_gemm_kernel('))
    _in_order(k, ['else if ((kernel_id >= 21 && kernel_id <= 27) || (kernel_id >= 31 && kernel_id <= 33))',
                  'else if (kernel_id >= 1 && kernel_id <= 65) rc = launch_gemm_cfg(g, kernel_id, s);',
                  'else if (kernel_id >= 101 && kernel_id <= 106) rc = launch_gemm_woq_cfg(g, kernel_id - 100, s);',
                  'else if (kernel_id == TLLM_GEMM_KERNEL_REGISTER_STAGED)', 'if (residual || silu_gate)', 'rc = launch_gemm_mfma(g, s);',
                  'return rc;'], 'tllm_gemm_kernel')
    api = open(os.path.join(os.path.dirname(CSRC), '..', 'include', 'tllm_runtime_api.h')).read()
    assert f'#define TLLM_GEMM_KERNEL_REGISTER_STAGED {GC.REGISTER_STAGED}' in api
    t = _squash(src('gemm_tactics.hip'))
    for name, want in (('kSqCandidates', GC.SQ_CANDIDATES), ('kFp16Candidates', GC.FP16_CANDIDATES), ('kSqStatic', GC.SQ_STATIC),
                       ('kFp16Static', GC.FP16_STATIC)):
        assert _ints(re.search(rf'const int {name}\[\] = \{{([\d, ]+)\}};', t).group(1)) == want, name
    # the static lists are what gemm_static_cfg can answer; no list names an ablation or an id without a case label
    ids = lambda wt, persist: {i for i, *_ in GC.SHAPES if i not in (6, GC.PHASED_256x128)} | \
        {(62 if persist else 42, 63 if persist else 20) if wt == GC.W_INT8_SQ else (56 if persist else 54, 55 if persist else 50)}
    for wt, static, cands, table in ((GC.W_INT8_SQ, GC.SQ_STATIC, GC.SQ_CANDIDATES, GC.SQP), (GC.W_FP16, GC.FP16_STATIC, GC.FP16_CANDIDATES, GC.F16P)):
        want = set()
        for persist in (0, 1):
            for i in ids(wt, persist):
                want |= set(i) if isinstance(i, tuple) else {i}
        assert set(static) == want
        assert set(cands) | set(static) <= set(GC.GLDS) | set(table)
        assert not (set(cands) | set(static)) & set(GC.ABLATIONS)


# ---------------------------------------------------------------------------------------------- completeness
def uncovered(cases, cus=GC.TABLE_CUS):
    """what the dispatch can reach and no (served) case of `cases` reaches"""
    insts = [GC.instance(c, cus) for c in cases]
    served = [i for i in insts if i[0] != 'refused']
    keys = {GC.key(i) for i in served}
    branches = {i[0] for c, i in zip(cases, insts) if c.kernel == 0}
    posts = {(i[0].split('>')[-1], i[2]) for c, i in zip(cases, insts) if c.kernel == 0 and i[0] != 'refused'}
    refused_ablations = {c.kernel for c, i in zip(cases, insts) if i == ('refused', 'ablation')}
    return ([('kernel', k) for k in sorted(GC.reachable_kernels() - keys, key=str)]
            + [('branch', b) for b in GC.BRANCHES if b not in branches] + [('pass', p) for p in GC.POSTS if p not in posts]
            + [('ablation refused', a) for a in GC.ABLATIONS if a not in refused_ablations])


def test_every_reachable_kernel_and_branch_has_a_case():
    assert uncovered(GC.CASES) == []
    # what the table says it covers is what the mirror makes of it: the refusals are refusals, the named ids are the instances
    for c in GC.CASES:
        i = GC.instance(c)
        assert ('-no-' in c.name or c.name in ('ablation', 'wrong-type', 'no-such-id')) == (i[0] == 'refused'), (GC.case_id(c), i)
        if c.name == 'regstaged-add-not-in-place':  # served out of place, refused with residual == c
            assert i[2] == 'add' and GC.instance(c, inplace=True)[0] == 'refused'
        if c.name.startswith('static-'):
            assert GC.static_cfg(c, GC.TABLE_CUS) == int(c.name[7:]), GC.case_id(c)
        if i[0] == 'persist':
            tm, tiles, grid = GC.persist_walk(c, GC.TABLE_CUS)
            if c.name.startswith('persist-tm'):
                assert tm == int(c.name[10:]) and grid % 8, GC.case_id(c)
            if c.name.startswith('persist-x'):
                assert -(-tiles // grid) == int(c.name[9:]) and grid % 8, GC.case_id(c)
    tms = {(c.kernel, GC.persist_walk(c, 256)[0]) for c in GC.CASES if c.name.startswith('persist-tm')}
    assert tms == {(i, tm) for i in (60, 62, 63, 55, 56) for tm in (1, 2, 5, 6, 7)}


def test_every_one_tile_family_sees_every_variant():
    for wt, fam, n in ((GC.W_INT8_SQ, 'lockstep', 14), (GC.W_FP16, 'lockstep', 14), (GC.W_INT8_SQ, 'phased', 4), (GC.W_FP16, 'phased', 5)):
        cs = [c for c in GC.CASES if c.wt == wt and c.name.startswith(fam + '-') and c.name[len(fam) + 1] in 'AB']
        assert {c.name[len(fam) + 1:] for c in cs} == {f'{x}{v}' for x in 'AB' for v in range(4)}, (wt, fam)
        assert len({c.kernel for c in cs}) == n and all(sum(c.kernel == k for c in cs) == 2 for k in {c.kernel for c in cs})
        assert {(c.per_channel, c.per_token) for c in cs} == {(0, 0), (0, 1), (1, 0), (1, 1)} or wt != GC.W_INT8_SQ
        assert {GC.DT_FLOAT, GC.DT_HALF} | ({GC.DT_INT32} if wt == GC.W_INT8_SQ else set()) == {c.out for c in cs}
        assert {32, 33, 300} == {c.M for c in cs} and {453, 456} == {c.N for c in cs}
        assert any(c.epi == GC.EPI_RES and c.strided and c.inplace for c in cs) and any(c.epi == GC.EPI_RES and not c.strided for c in cs)
        assert any(c.ldc_odd and GC.strides(c)[2] % 2 for c in cs)
        assert (wt == GC.W_INT8_SQ) or any(c.epi == GC.EPI_GATE and c.strided for c in cs)
        kt = {c.K * GC.es_of(wt) // 128 for c in cs}
        assert 1 in kt and any(k >= 9 and k % 2 for k in kt)


def test_removing_a_sole_case_names_the_uncovered_instance():
    insts = [GC.instance(c) for c in GC.CASES]
    tokens = []
    for c, i in zip(GC.CASES, insts):
        t = set()
        if i[0] != 'refused':
            t.add(('kernel', GC.key(i)))
        if c.kernel == 0:
            t.add(('branch', i[0]))
            if i[0] != 'refused':
                t.add(('pass', (i[0].split('>')[-1], i[2])))
        if i == ('refused', 'ablation'):
            t.add(('ablation refused', c.kernel))
        tokens.append(t)
    required = {('kernel', k) for k in GC.reachable_kernels()} | {('branch', b) for b in GC.BRANCHES} | {('pass', p) for p in GC.POSTS} \
        | {('ablation refused', a) for a in GC.ABLATIONS}
    sole = 0
    for n, t in enumerate(tokens):
        only_here = {x for x in t & required if not any(x in u for m, u in enumerate(tokens) if m != n)}
        if not only_here:
            continue
        sole += 1
        missing = set(uncovered(GC.CASES[:n] + GC.CASES[n + 1:]))
        assert only_here <= missing, (GC.case_id(GC.CASES[n]), only_here, missing)
    assert sole >= 10  # the chain's branches, the passes and the ablations' refusals are mostly sole
