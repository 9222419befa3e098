"""Host restatement, in numpy, of the sampling rule the device sampler implements (csrc/kernels/kernels.h, SamplingParams;
csrc/kernels/sampling.hip): counter-based uniform variates, temperature, repetition / presence penalty, minimum length,
top-k / top-p candidates and the prefix-sum draw.

The rule follows the reference's dynamic decoder at beam_width 1 (layers/baseSamplingLayer.cpp:171-248,
layers/topKSamplingLayer.cu:42-60, kernels/samplingTopKKernels.cu:271-300, samplingTopPKernels.cu:884-970,
samplingPenaltyKernels.cu) except for the random sequence: u is Philox4x32-10 of (seed, row, token number), not cuRAND's.

Penalty arithmetic is fp32 in the device's order; the prefix sums are fp64 (the device sums exp in fp32 scaled to 2^40 integers,
so the two agree to about 1e-6 of the total mass - what `interval` lets a test check without depending on either rounding)."""
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_M32 = 0xFFFFFFFF
TOP_K_MAX = 1024  # the reference's TOP_K_MAX (samplingTopKKernels.h)


def philox4x32_10(counter: Sequence[int], key: Sequence[int]):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11): 4 counter words, 2 key words -> 4 output words."""
    c0, c1, c2, c3 = (int(x) & _M32 for x in counter)
    k0, k1 = (int(x) & _M32 for x in key)
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + PHILOX_W0) & _M32, (k1 + PHILOX_W1) & _M32
    return c0, c1, c2, c3


def uniform(seed: int, b: int, g: int) -> np.float32:
    """u in (0, 1] of row b's generated token number g (1-based): a function of (seed, b, g) and nothing else."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w0 = philox4x32_10((b, g, 0, 0), (seed & _M32, seed >> 32))[0]
    return np.float32(((w0 >> 8) + 1) * 2.0 ** -24)


@dataclass
class Config:
    top_k: int = 1
    top_p: float = 0.0
    temperature: float = 1.0
    repetition_penalty: float = 1.0
    presence_penalty: float = 0.0
    min_length: int = 1
    random_seed: int = 0

    def effective(self, vocab: int):
        """(k', p') after clipping and the reference's two substitutions (topKSamplingLayer.cu:42-60)."""
        k, p = int(self.top_k), min(float(np.float32(self.top_p)), 1.0)
        if k == 0 and p == 0.0:
            k = 1
        elif k > 0 and p == 0.0:
            p = 1.0
        k = vocab if k == 0 else min(k, TOP_K_MAX)
        return min(k, vocab), p


def history_ids(history_row, input_length: int, max_input_len: int, g: int) -> np.ndarray:
    """The ids that count for the penalty: real prompt tokens [0, input_length) and the g - 1 generated tokens behind the padded
    prompt; padding slots [input_length, max_input_len) do not."""
    h = np.asarray(history_row)
    return np.concatenate([h[:min(input_length, max_input_len)], h[max_input_len:max_input_len + g - 1]]).astype(np.int64)


def transform(logits, cfg: Config, g: int, end_id: int = -1, history: Optional[np.ndarray] = None) -> np.ndarray:
    """Steps 1-3: y (fp32) from the raw logits of one row.  `history`: the ids from history_ids()."""
    y = np.asarray(logits, np.float32).copy()
    V = y.shape[0]
    with np.errstate(all='ignore'):
        if np.float32(cfg.temperature) != np.float32(1.0):
            y = y * (np.float32(1.0) / (np.float32(cfg.temperature) + np.float32(1e-6)))
        rep, pres = np.float32(cfg.repetition_penalty), np.float32(cfg.presence_penalty)
        if rep != 1 and pres != 0:
            raise ValueError('repetition_penalty and presence_penalty are mutually exclusive')
        if (rep != 1 or pres != 0) and history is not None and len(history):
            ids = np.unique(np.asarray(history, np.int64))  # once per distinct id
            ids = ids[(ids >= 0) & (ids < V)]
            if rep != 1:
                y[ids] = np.where(y[ids] < 0, y[ids] * rep, y[ids] / rep).astype(np.float32)
            else:
                y[ids] = (y[ids] - pres).astype(np.float32)
    if g < cfg.min_length and 0 <= end_id < V:
        y[end_id] = -np.finfo(np.float32).max
    y[np.isnan(y)] = -np.inf
    y[y == 0] = 0.0  # -0 -> +0
    return y


def order(y: np.ndarray) -> np.ndarray:
    """ids by (y descending, id ascending)."""
    return np.lexsort((np.arange(y.shape[0]), -y.astype(np.float64)))


@dataclass
class Draw:
    token: int            # the id the rule selects in fp64
    cand: np.ndarray      # the first k' ids of the order
    prefix: np.ndarray    # fp64 inclusive prefix sums of their weights
    total: float          # S
    target: float         # u * p' * S
    u: float

    def interval(self, token: int):
        """(position among the candidates or -1, prefix before it, prefix including it)."""
        pos = np.nonzero(self.cand == token)[0]
        if len(pos) == 0:
            return -1, None, None
        i = int(pos[0])
        return i, (float(self.prefix[i - 1]) if i else 0.0), float(self.prefix[i])

    def excess(self, token: int) -> float:
        """How far outside [prefix[i-1], prefix[i]] the target lies for this token, as a share of S (0 = inside; inf = not a
        candidate)."""
        i, lo, hi = self.interval(token)
        if i < 0:
            return float('inf')
        return max(lo - self.target, self.target - hi, 0.0) / self.total if self.total > 0 else 0.0

    def unique(self) -> bool:
        """True when the configuration leaves one possible token (k' = 1, or every candidate but one at weight 0)."""
        w = np.diff(np.concatenate([[0.0], self.prefix]))
        return len(self.cand) == 1 or int((w > 0).sum()) <= 1


def draw(logits, cfg: Config, b: int, g: int, end_id: int = -1, history: Optional[np.ndarray] = None,
         u: Optional[float] = None) -> Draw:
    """Steps 1-5 for one row.  `u` overrides the generator (tests of the rule itself)."""
    y = transform(logits, cfg, g, end_id, history)
    V = y.shape[0]
    k, p = cfg.effective(V)
    cand = order(y)[:k]
    yc = y[cand].astype(np.float64)
    ymax = yc[0]
    with np.errstate(all='ignore'):
        w = np.where(yc == ymax, 1.0, np.where(np.isneginf(yc), 0.0, np.exp(yc - ymax)))
    if np.isneginf(ymax):
        w = np.zeros_like(yc)
    prefix = np.cumsum(w)
    total = float(prefix[-1])
    uu = float(uniform(cfg.random_seed, b, g) if u is None else u)
    target = uu * p * total
    reached = np.nonzero(prefix >= target)[0]
    i = int(reached[0]) if len(reached) else k - 1
    return Draw(int(cand[i]), cand, prefix, total, target, uu)


def sample(logits, cfg: Config, b: int, g: int, end_id: int = -1, history: Optional[np.ndarray] = None,
           u: Optional[float] = None) -> int:
    return draw(logits, cfg, b, g, end_id, history, u).token


def probabilities(logits, cfg: Config, g: int = 1, end_id: int = -1, history: Optional[np.ndarray] = None) -> np.ndarray:
    """[vocab] probability of every id under the rule with u uniform on (0, 1]: the candidates' weights cut at p' of their mass."""
    d = draw(logits, cfg, 0, g, end_id, history, u=1.0)
    out = np.zeros(np.asarray(logits).shape[0])
    if d.total <= 0:
        out[d.cand[0]] = 1.0
        return out
    lim = d.target  # p' * S
    lo = np.concatenate([[0.0], d.prefix[:-1]])
    out[d.cand] = np.clip(np.minimum(d.prefix, lim) - lo, 0.0, None) / lim
    return out
