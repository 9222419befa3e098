"""LoRA adapters per row, restated in numpy float64 - TEST INFRASTRUCTURE (the kernels: csrc/kernels/lora.hip; the rule as the
kernels state it: csrc/kernels/kernels.h LoraShrinkParams / LoraExpandParams).

A projection site is the fused QKV (segments q | k | v), attention.dense, fc | gate (two segments) or mlp.proj.  For row m with
adapter a = row_adapter[m] >= 0, rank r and scale s_a = alpha / r (alpha / sqrt(r) under rsLoRA):

  shrink   t[m][g r + j] = sum_k A_a[g r + j][k] xh[m][k]            xh: the fp16 row the base projection consumes
  expand   y[m][n] <- f16(y[m][n] + s_a sum_j B_a[n][j] t[m][seg(n) r + j])

A row with adapter -1 is not read by shrink, and expand leaves its y alone.  Here every sum is float64 and the only rounding is
the final one to fp16; the kernels accumulate in fp32 (the tests' bounds say how far that may be)."""
import numpy as np

MODULES = ('q', 'k', 'v', 'o', 'gate', 'up', 'down')
# module key -> (tensor name inside a layer, site, segment of the site)
MODULE_NAMES = {'q': ('attention.q', 'attention.qkv', 0), 'k': ('attention.k', 'attention.qkv', 1),
                'v': ('attention.v', 'attention.qkv', 2), 'o': ('attention.dense', 'attention.dense', 0),
                'gate': ('mlp.fc', 'mlp.fc|gate', 0), 'up': ('mlp.gate', 'mlp.fc|gate', 1), 'down': ('mlp.proj', 'mlp.proj', 0)}


def scale(alpha, r, use_rslora=False):
    return float(alpha) / (np.sqrt(float(r)) if use_rslora else float(r))


def f16(x):
    return np.asarray(x, np.float64).astype(np.float16)


def _rows(M, row_adapter):
    return np.zeros(M, np.int64) if row_adapter is None else np.asarray(row_adapter, np.int64)


def _per_adapter(v):
    return list(v) if isinstance(v, (list, tuple)) else [v]


def shrink(xh, A, row_adapter=None):
    """xh [M, K] (fp16 values); A [R, K] or a list of them, one per adapter; -> t float64 [M, R], NaN on the rows of no adapter
    (nothing may read them)"""
    A = _per_adapter(A)
    xh = np.asarray(xh)
    ra = _rows(xh.shape[0], row_adapter)
    t = np.full((xh.shape[0], A[0].shape[0]), np.nan)
    for m in range(xh.shape[0]):
        if 0 <= ra[m] < len(A):
            t[m] = np.asarray(A[ra[m]], np.float64) @ xh[m].astype(np.float64)
    return t


def segment_of(seg_n):
    """column -> segment, for segments of seg_n[g] columns"""
    return np.repeat(np.arange(len(seg_n)), seg_n)


def delta(t, B, s, seg_n=None, row_adapter=None):
    """s_a sum_j B_a[n][j] t[m][seg(n) r + j] in float64, [M, N]; 0 on the rows of no adapter.  B [N, r] or a list, s a float or a
    list; seg_n: the segments' column counts (None: one segment)"""
    B, ra = _per_adapter(B), _rows(t.shape[0], row_adapter)
    s = _per_adapter(s)
    N, r = B[0].shape
    seg = segment_of(seg_n if seg_n is not None else [N])
    assert seg.shape[0] == N and t.shape[1] == (seg.max() + 1) * r
    d = np.zeros((t.shape[0], N))
    cols = seg[:, None] * r + np.arange(r)[None, :]  # [N, r]: the entries of t a column reads
    for m in range(t.shape[0]):
        if 0 <= ra[m] < len(B):
            d[m] = s[ra[m]] * np.einsum('nj,nj->n', np.asarray(B[ra[m]], np.float64), t[m][cols])
    return d


def expand(y16, t, B, s, seg_n=None, row_adapter=None):
    """-> fp16 [M, N]; rows of no adapter keep their bits"""
    y16 = np.asarray(y16, np.float16)
    ra = _rows(y16.shape[0], row_adapter)
    on = (ra >= 0) & (ra < len(_per_adapter(B)))
    out = y16.copy()
    d = delta(t, B, s, seg_n, row_adapter)
    out[on] = f16(y16[on].astype(np.float64) + d[on])
    return out


def pad_rank(A, B, r_max, nseg=1):
    """zero-pad an adapter of a site from its rank r to r_max: A [nseg r, K] -> [nseg r_max, K] (per segment), B [N, r] -> [N, r_max]"""
    r = B.shape[1]
    assert A.shape[0] == nseg * r and r <= r_max
    Ap = np.zeros((nseg * r_max, A.shape[1]), A.dtype)
    for g in range(nseg):
        Ap[g * r_max:g * r_max + r] = A[g * r:(g + 1) * r]
    Bp = np.zeros((B.shape[0], r_max), B.dtype)
    Bp[:, :r] = B
    return Ap, Bp


def pack_site(modules, seg_n, K, r):
    """modules: per segment (A_g [r, K], B_g [seg_n[g], r]) or None (zeros) -> (A [nseg r, K], B [sum seg_n, r]) of the site"""
    A = np.zeros((len(seg_n) * r, K), np.float16)
    B = np.zeros((int(np.sum(seg_n)), r), np.float16)
    off = 0
    for g, mod in enumerate(modules):
        if mod is not None:
            A[g * r:(g + 1) * r] = mod[0]
            B[off:off + seg_n[g]] = mod[1]
        off += seg_n[g]
    return A, B


class wrap_oracle_linear:
    """The oracle's _Linear call convention with an adapter behind it: (x16, in_q) -> f16(base(x16, in_q) + s (x16 A^T) B^T), so
    that a test can put adapters into qmodel['oracle']['layers'][i][name] without touching oracle/.  A [nseg r, K], B [N, r], seg_n
    the segments' columns (None: one).  per_sequence: a list with one (A, B, s) or None per sequence of the batch instead - the
    rows of a call are the sequences' rows in order, M / len(per_sequence) each (the prompt's [B * S] and a step's [B])."""
    kind = 'lora'

    def __init__(self, base, A=None, B=None, s=1.0, seg_n=None, per_sequence=None):
        self.base, self.seg_n = base, seg_n
        self.per_sequence = per_sequence if per_sequence is not None else [(A, B, s)]

    def __call__(self, x16, in_q=None):
        y = np.asarray(self.base(x16, in_q), np.float32)
        x = np.asarray(x16)
        M, nb = x.shape[0], len(self.per_sequence)
        ra = np.arange(M) // (M // nb) if nb > 1 else np.zeros(M, np.int64)
        live = [i for i, a in enumerate(self.per_sequence) if a is not None]
        if not live:
            return y
        slot = {i: j for j, i in enumerate(live)}
        rows = np.array([slot.get(int(b), -1) for b in ra])
        As, Bs, ss = zip(*[self.per_sequence[i] for i in live])
        t = shrink(x.astype(np.float16), list(As), rows)
        return expand(y.astype(np.float16), t, list(Bs), list(ss), self.seg_n, rows).astype(np.float32)


def random_adapter(cfg, seed, r, modules=MODULES, b_std=0.05, num_kv_heads=None):
    """engine-named tensors of one adapter: layers.{i}.{module}.lora_a [r, K] ~ N(0, 1 / K), .lora_b [N, r] ~ N(0, b_std^2), fp16"""
    rng = np.random.default_rng(seed)
    D, I, H = cfg['hidden_size'], cfg['inter_size'], cfg['num_heads']
    kvd = (num_kv_heads or H) * (D // H)
    shape = {'q': (D, D), 'k': (kvd, D), 'v': (kvd, D), 'o': (D, D), 'gate': (I, D), 'up': (I, D), 'down': (D, I)}  # (N, K)
    out = {}
    for i in range(cfg['num_layers']):
        for m in modules:
            N, K = shape[m]
            out[f'layers.{i}.{MODULE_NAMES[m][0]}.lora_a'] = (rng.standard_normal((r, K)) / np.sqrt(K)).astype(np.float16)
            out[f'layers.{i}.{MODULE_NAMES[m][0]}.lora_b'] = (rng.standard_normal((N, r)) * b_std).astype(np.float16)
    return out


def site_adapters(cfg, tensors, layer, r, num_kv_heads=None):
    """the (A, B, seg_n) of the four sites of one layer from engine-named adapter tensors, keyed by the oracle's LINEARS names
    ('mlp.fc|gate' holds the two-segment site; split_gate_up gives the oracle's two separate linears)"""
    D, I, H = cfg['hidden_size'], cfg['inter_size'], cfg['num_heads']
    kvd = (num_kv_heads or H) * (D // H)
    segs = {'attention.qkv': ([D, kvd, kvd], D), 'attention.dense': ([D], D), 'mlp.fc|gate': ([I, I], D), 'mlp.proj': ([D], I)}
    out = {}
    for site, (seg_n, K) in segs.items():
        mods = [None] * len(seg_n)
        for m, (name, st, g) in MODULE_NAMES.items():
            a = tensors.get(f'layers.{layer}.{name}.lora_a')
            if st == site and a is not None:
                mods[g] = (a, tensors[f'layers.{layer}.{name}.lora_b'])
        if any(m is not None for m in mods):
            out[site] = pack_site(mods, seg_n, K, r) + (seg_n, )
    return out


def adapt_oracle(model, cfg, per_sequence, r, num_kv_heads=None):
    """a copy of an oracle model (quant_oracle's qmodel['oracle'] or _fp16_model) whose linears carry adapters: per_sequence = one
    (tensors, scale) or None per sequence (one entry: every row)"""
    out = dict(model, layers=[])
    for li, lw in enumerate(model['layers']):
        sites = [None if p is None else site_adapters(cfg, p[0], li, r, num_kv_heads) for p in per_sequence]
        scales = [None if p is None else p[1] for p in per_sequence]

        def wrap(base, pick):
            ps, seg = [], None
            for d, s in zip(sites, scales):
                e = None if d is None else pick(d)  # (A, B, seg_n) or None
                ps.append(None if e is None else (e[0], e[1], s))
                seg = e[2] if e is not None else seg
            return base if seg is None else wrap_oracle_linear(base, seg_n=seg, per_sequence=ps)

        def site(name):
            return lambda d: d.get(name)

        def half(g):  # fc | gate -> the oracle's separate mlp.fc / mlp.gate
            def pick(d):
                if 'mlp.fc|gate' not in d:
                    return None
                A, B, seg_n = d['mlp.fc|gate']
                return A[g * r:(g + 1) * r], B[g * seg_n[0]:g * seg_n[0] + seg_n[g]], [seg_n[g]]
            return pick

        nl = dict(lw)
        nl['attention.qkv'] = wrap(lw['attention.qkv'], site('attention.qkv'))
        nl['attention.dense'] = wrap(lw['attention.dense'], site('attention.dense'))
        nl['mlp.fc'] = wrap(lw['mlp.fc'], half(0))
        nl['mlp.gate'] = wrap(lw['mlp.gate'], half(1))
        nl['mlp.proj'] = wrap(lw['mlp.proj'], site('mlp.proj'))
        out['layers'].append(nl)
    return out
