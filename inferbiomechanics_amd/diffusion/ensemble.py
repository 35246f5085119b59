"""[BUILD-DEFINED] Host arithmetic of the order statistics of a posterior ensemble (csrc/ensemble.hip, hip.ensemble_order):
where in the sorted K members a quantile lies, and what an interval made of such quantiles can cover.  Plain float64, no
device work.

The plotting position is Weibull's (Hyndman & Fan type 6), pos = q (K + 1) - 1 on the 0-based sorted members, deliberately
not numpy's default (type 7): for a truth exchangeable with the members, P(y < s_(i)) = (i + 1) / (K + 1), so the type-6
quantile at level q has probability q below it wherever the position is not clipped, and an interval's nominal coverage means
what it says.  Where it IS clipped -- q < 1 / (K + 1) or q > K / (K + 1): the ensemble is too small for the level -- the
quantile is the smallest / largest member and the interval covers less than its level: ``calibrated_coverage`` says how much."""
import math
from typing import Tuple

import numpy as np


def _position(q: float, K: int) -> float:
    q, K = float(q), int(K)
    if K < 1:
        raise ValueError(f"an ensemble has at least one member, got K = {K}")
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"a quantile level lies in [0, 1], got {q}")
    return min(max(q * (K + 1) - 1.0, 0.0), float(K - 1))


def quantile_position(q: float, K: int) -> Tuple[int, float]:
    """(i, f): the level-q quantile of K sorted members s is s[i] + f (s[min(i + 1, K - 1)] - s[i]); f is a float32 value in
    [0, 1], 0 at the last member"""
    pos = _position(q, K)
    i = min(int(math.floor(pos)), K - 1)
    f = 0.0 if i == K - 1 else float(np.float32(pos - i))
    return i, f


def interval_levels(L: float) -> Tuple[float, float, float]:
    """the levels of the central interval of nominal coverage L and of the median"""
    try:
        L = float(L)
    except (TypeError, ValueError):
        raise ValueError(f"an interval level is a number in (0, 1), got {L!r}") from None
    if not 0.0 < L < 1.0:
        raise ValueError(f"an interval level lies strictly between 0 and 1, got {L}")
    return (1.0 - L) / 2.0, 0.5, (1.0 + L) / 2.0


def calibrated_coverage(L: float, K: int) -> float:
    """the coverage that the level-L interval of a perfectly calibrated K-member ensemble attains: (pos_hi - pos_lo) / (K + 1)
    with the clipped positions -- L itself where neither end is clipped, less where the ensemble is too small for the level
    (K = 8, L = 0.8: 7 / 9).  Exact when both positions are whole numbers."""
    lo, _, hi = interval_levels(L)
    return (_position(hi, K) - _position(lo, K)) / (K + 1)
