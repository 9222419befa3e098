"""Host restatement, in numpy float64, of the token-scoring rule the device implements (csrc/kernels/kernels.h,
TokenLogprobParams; csrc/kernels/token_logprob.hip; tllm_session_score), the counterpart of sampling_ref.py.

Row r with target t over the ids v < vocab:  lse = log sum_v exp(x[v]),  log_prob = x[t] - lse,  top1 = arg-max (ties -> lowest id).
Special values: t outside [0, vocab) (-1 = no target) -> log_prob 0; x[t] = -inf -> log_prob -inf (the row of only -inf has
lse -inf and top1 0); NaN / +inf logits are undefined.  The vocabulary may come in parts [nparts, rows, vocab_part] with id =
part * vocab_part + i and ids >= vocab padding that is never read: `partials` gives one record per (part, row), `merge` folds them
in part order."""
import numpy as np

NO_ID = 0x7FFFFFFF  # top_id of a part without a valid id


def _lse(x: np.ndarray):
    """x float64 [rows, n] -> (m, s, lse): m = row max (-inf for n == 0 or a row of only -inf), s = sum exp(x - m) (0 then)."""
    rows, n = x.shape
    m = x.max(axis=1) if n else np.full(rows, -np.inf)
    live = np.isfinite(m)
    s = np.zeros(rows)
    if live.any():
        with np.errstate(invalid='ignore'):
            s[live] = np.exp(x[live] - m[live, None]).sum(axis=1)
    with np.errstate(divide='ignore'):
        lse = np.where(live, m + np.log(np.where(live, s, 1.0)), -np.inf)
    return m, s, lse


def _finish(xt, lse, targets, vocab):
    has = (targets >= 0) & (targets < vocab)
    with np.errstate(invalid='ignore'):
        lp = np.where(np.isneginf(xt), -np.inf, xt - lse)
    return np.where(has, lp, 0.0)


def token_logprobs(x, targets, vocab=None):
    """x [rows, >= vocab] (columns >= vocab are padding), targets int [rows] -> (log_probs f64, lse f64, top1 int32)."""
    x = np.asarray(x, np.float64)
    targets = np.asarray(targets, np.int64)
    vocab = x.shape[1] if vocab is None else int(vocab)
    x = x[:, :vocab]
    _, _, lse = _lse(x)
    has = (targets >= 0) & (targets < vocab)
    xt = np.where(has, x[np.arange(x.shape[0]), np.where(has, targets, 0)], -np.inf)
    top1 = x.argmax(axis=1).astype(np.int32)  # first occurrence = lowest id; a row of only -inf gives 0
    return _finish(xt, lse, targets, vocab), lse, top1


def partials(x, targets, vocab):
    """x [nparts, rows, vocab_part] -> records float64 [nparts, rows, 5]: m, s, xt, top_val, top_id of every (part, row)."""
    x = np.asarray(x, np.float64)
    targets = np.asarray(targets, np.int64)
    nparts, rows, vp = x.shape
    rec = np.zeros((nparts, rows, 5))
    for p in range(nparts):
        first = p * vp
        n = int(min(max(vocab - first, 0), vp))
        part = x[p, :, :n]
        m, s, _ = _lse(part)
        inside = (targets >= first) & (targets < first + n)
        xt = np.where(inside, part[np.arange(rows), np.where(inside, targets - first, 0)] if n else -np.inf, -np.inf)
        rec[p, :, 0], rec[p, :, 1], rec[p, :, 2] = m, s, xt
        rec[p, :, 3] = part.max(axis=1) if n else -np.inf
        rec[p, :, 4] = first + part.argmax(axis=1) if n else NO_ID
    return rec


def merge(rec, targets, vocab):
    """records [nparts, rows, >= 5] in part order -> (log_probs, lse, top1); one part: the identity on what it holds."""
    rec = np.asarray(rec, np.float64)
    targets = np.asarray(targets, np.int64)
    m, s, xt, tv, ti = (rec[..., k] for k in range(5))
    M = m.max(axis=0)
    live = np.isfinite(M)
    with np.errstate(invalid='ignore'):
        S = np.where(np.isfinite(m), s * np.exp(m - M[None]), 0.0).sum(axis=0)
    with np.errstate(divide='ignore'):
        lse = np.where(live, M + np.log(np.where(live, S, 1.0)), -np.inf)
    best = tv.max(axis=0)
    top1 = np.where(tv == best[None], ti, float(NO_ID)).min(axis=0)
    top1 = np.where(top1 == NO_ID, 0, top1).astype(np.int32)
    return _finish(xt.max(axis=0), lse, targets, vocab), lse, top1


def sequence_scores(position_logits, ids, lens, vocab=None):
    """position_logits [B, S, V]: row (b, t) = the logits after ids[b][:t + 1].  -> (log_probs f64 [B, S], top1 int32 [B, S]):
    log_probs[b][t] = log softmax(position_logits[b][t - 1])[ids[b][t]] for 1 <= t < lens[b], 0 elsewhere; top1 the arg-max of
    that distribution, -1 elsewhere (tllm_session_score's convention)."""
    z = np.asarray(position_logits, np.float64)
    ids = np.asarray(ids, np.int64)
    B, S = ids.shape
    lp, top = np.zeros((B, S)), np.full((B, S), -1, np.int32)
    for b in range(B):
        n = int(lens[b])
        if n > 1:
            lp[b, 1:n], _, top[b, 1:n] = token_logprobs(z[b, :n - 1], ids[b, 1:n], vocab)
    return lp, top


def perplexity(log_probs, lens):
    """exp(-sum log_probs / sum (len - 1)) over all sequences given; nan when no token is scored."""
    log_probs = np.asarray(log_probs, np.float64)
    n = float(np.sum(np.maximum(np.asarray(lens, np.int64) - 1, 0)))
    return float(np.exp(-log_probs.sum() / n)) if n > 0 else float('nan')
