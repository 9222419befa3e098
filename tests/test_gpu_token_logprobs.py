"""GPU tests of the token-scoring kernels (csrc/kernels/token_logprob.hip) through tllm_token_logprobs, every row held to the
numpy float64 restatement of the rule (tensorrt_llm/runtime/scoring_ref.py): log-probability and log-sum-exp within TOL, the
arg-max exact wherever float64's top value is unique (the lowest id on the ties row), the logits untouched, a second call
bit-identical, and every vocabulary slot counted exactly once (head / vector body / tail of rows at every 4-byte alignment,
part seams, padding ids holding 1e30).

TOL.  Device and restatement read the same fp32 logits; they differ in how lse = M + log S, S = sum exp(x - M), is rounded.
Relative error of S on the device (ids more than 16 below the maximum weigh under 1.2e-7 of it and do not count):
  * x - m rounded to fp32: 2^-24 * 16 = 9.5e-7 on the exponent; expf 1 - 2 ulp = 1.2e-7 - 2.4e-7: 1.2e-6 per term, and so for
    their sum (all terms are positive);
  * the online form rescales a partial sum by exp(m_old - m_new) whenever its maximum rises: the roundings of those differences
    add up to at most 2^-24 * 16 = 9.5e-7 along a path, each expf adds up to 2.4e-7; a path has the thread's own rises (about
    ln 32 = 4 on an i.i.d. row), 6 shuffle levels, 3 wave joins and the merge, ~14 factors: 9.5e-7 + 3.4e-6 = 4.3e-6 at worst;
  * fp32 summation: 2 levels in a group of four, a chain of 32 groups per thread at vocab 32000, 6 + 3 + 1 join levels, 44
    additions deep against the log2(V) = 15 of a pure tree: 44 * 2^-24 = 2.6e-6 at worst, ~ sqrt(44) * 2^-24 = 4e-7 typically.
Then logf adds 1 - 2 ulp of log S <= 10.4 (1.9e-6), and M + log S and x_t - lse each round to half an ulp of their magnitude,
up to 7.6e-6 for the rows shifted by +-60 with std 16 (|lse| and |log_prob| reach 128 - 200), 1.2e-7 - 9.5e-7 for the others.
Every term at its worst at once: 1.2e-6 + 4.3e-6 + 2.6e-6 + 1.9e-6 + 2 * 7.6e-6 = 2.5e-5; the terms are independent roundings,
their root-sum-square is 1.2e-5, and with the typical instead of the worst size of the summation and rescale terms the sum is
about 1e-5 - the figure a numpy fp32 emulation of the online reduction supports (worst 4.2e-6 over these rows).  Derived
bound: 1e-5.  The bar is 4 x that, TOL = 4e-5, below the 1e-4 of probability mass from which a dropped id would pass.
Largest error measured on an MI355X over every row of this file: 5.03e-6 (MEASURED below; profiles/token_logprobs.txt), half the
derived bound and an eighth of the bar."""
import numpy as np
import pytest

from tensorrt_llm.runtime import scoring_ref as R
from tensorrt_llm.runtime.native import token_logprobs

pytestmark = pytest.mark.gpu

DERIVED = 1e-5
TOL = 4 * DERIVED
assert TOL <= 1e-4
MEASURED = 5.03e-6  # largest |device - float64| of log_probs / lse seen on an MI355X (a log_probs row of the V = 32000 case)

SHAPES = [(32000, 1), (32003, 1), (257, 1), (1, 1), (32003, 4), (1000, 4)]
IDS = [f'v{v}-x{n}' for v, n in SHAPES]
NINF = np.float32(-np.inf)
_worst = [0.0]


def run_kernel(x, targets, nparts):
    """x [rows, V] fp32 host, targets [rows] -> (log_probs, lse, top1, records) from tllm_token_logprobs, twice; the rows laid
    out as the all-gather of vocabulary shards leaves them, [nparts, rows, ceil(V / nparts)], the padding ids holding 1e30"""
    import torch
    rows, V = x.shape
    vp = -(-V // nparts)
    full = np.full((rows, nparts * vp), 1e30, np.float32)
    full[:, :V] = x
    dev = torch.from_numpy(np.ascontiguousarray(full.reshape(rows, nparts, vp).transpose(1, 0, 2))).cuda()
    tg = torch.from_numpy(np.ascontiguousarray(targets, dtype=np.int32)).cuda()
    before = dev.clone()
    rec = torch.full((nparts, rows, 8), 7.0, dtype=torch.float32, device='cuda')
    lp, lse, top = token_logprobs(dev, tg, vocab=V, partials=rec)
    rec2 = torch.full((nparts, rows, 8), 9.0, dtype=torch.float32, device='cuda')
    lp2, lse2, top2 = token_logprobs(dev, tg, vocab=V, partials=rec2)
    torch.cuda.synchronize()
    assert torch.equal(before.view(torch.int32), dev.view(torch.int32)), 'the kernels must not modify the logits'
    for a, b in ((lp, lp2), (lse, lse2), (top, top2), (rec, rec2)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), 'a second call must give identical bits'
    return lp.cpu().numpy(), lse.cpu().numpy(), top.cpu().numpy(), rec.cpu().numpy()


def check_close(got, ref, what):
    """infinities exactly, the rest within TOL of float64; returns the largest error"""
    got = got.astype(np.float64)
    fin = np.isfinite(ref)
    assert not np.isnan(got).any(), f'{what}: NaN'
    assert np.array_equal(got[~fin], ref[~fin]), f'{what}: special values differ: {got[~fin]} vs {ref[~fin]}'
    err = float(np.abs(got[fin] - ref[fin]).max()) if fin.any() else 0.0
    if err > _worst[0]:
        _worst[0] = err
        print(f'[token_logprobs] largest error so far {err:.3e} ({what})')
    bad = np.flatnonzero(fin)[np.abs(got[fin] - ref[fin]) > TOL]
    assert err <= TOL, f'{what}: |device - float64| = {err:.3e} > {TOL:.1e} at rows {bad[:8]}: {got[bad[:8]]} vs {ref[bad[:8]]}'
    return err


def draw_rows(r, V):
    """std 0.5 ... 16, the same shifted by +60 and -60, exact ties, 90 % -inf, only -inf"""
    base = [(r.standard_normal(V) * s).astype(np.float32) for s in (0.5, 1.0, 2.0, 4.0, 8.0, 16.0)]
    rows = base + [b + np.float32(60) for b in base] + [b - np.float32(60) for b in base]
    rows.append(r.integers(-3, 4, V).astype(np.float32))
    sparse = (r.standard_normal(V) * 3).astype(np.float32)
    sparse[r.random(V) < 0.9] = NINF
    rows.append(sparse)
    rows.append(np.full(V, NINF, np.float32))
    return np.stack(rows)


@pytest.mark.parametrize('V,nparts', SHAPES, ids=IDS)
def test_rows_match_the_float64_restatement(V, nparts):
    r = np.random.default_rng(V * 11 + nparts)
    base = draw_rows(r, V)
    n = base.shape[0]
    ties_row = n - 3
    # target sets: random, id 0, id V - 1, a -inf entry where the row has one (random elsewhere), none
    t_inf = r.integers(0, V, n)
    for i in range(n):
        dead = np.flatnonzero(np.isneginf(base[i]))
        if dead.size:
            t_inf[i] = dead[r.integers(0, dead.size)]
    sets = [r.integers(0, V, n), np.zeros(n, np.int64), np.full(n, V - 1), t_inf, np.full(n, -1)]
    x = np.concatenate([base] * len(sets))
    targets = np.concatenate(sets)
    lp, lse, top, rec = run_kernel(x, targets, nparts)
    lp0, lse0, top0 = R.token_logprobs(x, targets)
    tag = f'V {V} x {nparts}'
    check_close(lp, lp0, f'log_probs, {tag}')
    check_close(lse, lse0, f'lse, {tag}')
    assert (lp[targets < 0] == 0).all()
    # the arg-max: exact wherever float64's top value is unique, the lowest id otherwise (the ties row: several ids share 3.0)
    x64 = x.astype(np.float64)
    assert np.array_equal(top, top0), f'{tag}: top1 differs at rows {np.flatnonzero(top != top0)[:8]}'
    if V > 100:
        assert (x64[ties_row] == x64[ties_row].max()).sum() > 1 and top[ties_row] == np.flatnonzero(x64[ties_row] == 3.0)[0]
    assert top[n - 1] == 0 and lse[n - 1] == NINF and lp[n - 1] == NINF  # the row of only -inf with a real target
    # the records of the parts against the restatement's, and their merge
    rec0 = R.partials(np.ascontiguousarray(_parts(x, nparts)), targets, V)
    assert np.array_equal(rec[..., 0].astype(np.float64), rec0[..., 0]), 'part maxima'
    assert np.array_equal(rec[..., 2].astype(np.float64), rec0[..., 2]), 'target logits'
    assert np.array_equal(rec[..., 3].astype(np.float64), rec0[..., 3]), 'part top values'
    assert np.array_equal(rec[..., 4].view(np.int32), rec0[..., 4].astype(np.int32)), 'part top ids'
    assert (rec[..., 5:] == 0).all()
    live = rec0[..., 1] > 0
    assert np.array_equal(rec[..., 1][~live], rec0[..., 1][~live])
    assert np.abs(rec[..., 1][live] / rec0[..., 1][live] - 1).max() <= TOL
    if nparts == 1:  # the merge is the identity on the record
        f = np.isfinite(lse0)  # lse = m + logf(s) of exactly these two words: logf's 2 ulp and one rounding of the sum apart
        assert np.abs(lse[f] - (rec[0, f, 0].astype(np.float64) + np.log(rec[0, f, 1].astype(np.float64)))).max() <= DERIVED
        assert np.array_equal(top, np.where(rec[0, :, 4].view(np.int32) == R.NO_ID, 0, rec[0, :, 4].view(np.int32)))


def _parts(x, nparts):
    rows, V = x.shape
    vp = -(-V // nparts)
    full = np.full((rows, nparts * vp), 1e30, np.float64)
    full[:, :V] = x
    return full.reshape(rows, nparts, vp).transpose(1, 0, 2)


@pytest.mark.parametrize('V,nparts', SHAPES, ids=IDS)
def test_every_slot_is_counted_exactly_once(V, nparts):
    """x = -30 everywhere except x[j] = 0: with target j the log-probability is 0 to 1e-6 (a double count gives -0.69, a miss
    about -19) and the arg-max is j; with another target it is -30."""
    vp = -(-V // nparts)
    js = sorted({j for j in list(range(6)) + [7, 8, 63, 64, 255, 256, 1023, 1024, 4095, 4096, vp - 1, vp, vp + 1, V - 2, V - 1]
                 if 0 <= j < V})
    x = np.full((2 * len(js), V), -30, np.float32)
    targets = np.zeros(2 * len(js), np.int64)
    for k, j in enumerate(js):
        x[k, j] = x[len(js) + k, j] = 0
        targets[k] = j
        targets[len(js) + k] = (j + 1 + (V // 2)) % V  # another id (== j only when V == 1)
    lp, lse, top, _ = run_kernel(x, targets, nparts)
    lp0, lse0, top0 = R.token_logprobs(x, targets)
    for k, j in enumerate(js):
        assert abs(lp[k]) < 1e-6 and top[k] == j, f'V {V} x {nparts}: slot {j}: log_prob {lp[k]!r}, top1 {top[k]}'
        assert top[len(js) + k] == j
    check_close(lp, lp0, f'one-hot rows, V {V} x {nparts}')
    check_close(lse, lse0, f'one-hot rows lse, V {V} x {nparts}')
    if V > 1:
        assert np.abs(lp[len(js):] + 30).max() <= TOL
