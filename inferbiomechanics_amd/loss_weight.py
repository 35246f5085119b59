"""Weighting the diffusion loss by noise level.  ``include/ib_hip_lossweight.h`` states the kernel's arithmetic,
``csrc/loss_weight.hip`` applies a per-level weight table inside the loss launch of the fused step, and this module makes the
table on the host, in float64, cast to fp32 once.

    snr_t = ab_t / (1 - ab_t)                       ab = alphas_cumprod of the model's schedule
    'uniform'   w_t = 1                              the unweighted eps-MSE, through the weighted launches (for the report)
    'min_snr'   w_t = min(1, gamma / snr_t)          Min-SNR-gamma (Hang et al. 2023) for eps-prediction: min(snr, gamma) / snr
    'table'     w_t = the caller's [n_levels] values, finite and >= 0

A weight multiplies the squared error of what the network predicts (prediction.py).  'uniform' and 'table' mean the same under
every prediction kind; Min-SNR-gamma is min(snr, gamma) divided by the SNR-weight the kind's own squared error already carries
relative to the x0 error: min(snr, gamma) / snr for eps, min(snr, gamma) for x0, min(snr, gamma) / (snr + 1) for v.

The optimised loss is mean(w_t (eps_hat - eps)^2), a plain mean: it is not divided by the sum of the weights.  Beside it the
kernels report the unweighted error, overall and per band of noise level: level t of n_levels falls in band
t * LEVEL_BUCKETS // n_levels (level_band)."""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

from .hip import LOSS_LEVEL_BUCKETS as LEVEL_BUCKETS       # IB_LOSS_LEVEL_BUCKETS, read from the header in one place

KINDS = ("uniform", "min_snr", "table")


def check_gamma(v) -> float:
    try:
        x = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"min-SNR gamma must be a number > 0, got {v!r}") from None
    if not (x > 0.0 and np.isfinite(x)):                # NaN fails the comparison
        raise ValueError(f"min-SNR gamma must be > 0 and finite, got {v}")
    return x


def level_band(t, n_levels: int, buckets: int = LEVEL_BUCKETS):
    """the band of noise level t (an int or an integer array), with the kernel's clamp of t into [0, n_levels)"""
    n_levels = int(n_levels)
    if n_levels < 1:
        raise ValueError(f"n_levels must be >= 1, got {n_levels}")
    tl = np.clip(np.asarray(t, dtype=np.int64), 0, n_levels - 1)
    k = tl * int(buckets) // n_levels
    return int(k) if k.ndim == 0 else k


def band_edges(n_levels: int, buckets: int = LEVEL_BUCKETS) -> List[Tuple[int, int]]:
    """[(t_lo, t_hi)] per band, t_lo <= t < t_hi; t_lo == t_hi: no level falls in the band (n_levels < buckets)"""
    n_levels = int(n_levels)
    lo = [-(-k * n_levels // int(buckets)) for k in range(int(buckets) + 1)]      # ceil(k n / NB): the first level of band k
    return [(lo[k], lo[k + 1]) for k in range(int(buckets))]


class LossWeight:
    """LossWeight('min_snr', gamma=5.0) / LossWeight('uniform') / LossWeight('table', table=values)"""

    def __init__(self, kind: str, gamma: float = 5.0, table=None):
        if kind not in KINDS:
            raise ValueError(f"loss weight kind must be one of {KINDS}, got {kind!r}")
        self.kind = kind
        self.gamma = check_gamma(gamma)
        self.table: Optional[np.ndarray] = None
        if kind == "table":
            if table is None:
                raise ValueError("LossWeight('table') needs the table")
            tb = np.asarray(table.detach().cpu().numpy() if hasattr(table, "detach") else table, dtype=np.float64)
            if tb.ndim != 1 or tb.size < 1:
                raise ValueError(f"the weight table must be a non-empty vector, got shape {tb.shape}")
            if not np.all(np.isfinite(tb)) or np.any(tb < 0):
                raise ValueError("the weight table must be finite and >= 0")
            self.table = tb.copy()
        elif table is not None:
            raise ValueError(f"a table goes with kind 'table', not '{kind}'")

    def check_levels(self, n_levels: int):
        """a table must have one weight per noise level of the model (HipTrainer's constructor calls this)"""
        if self.table is not None and self.table.size != int(n_levels):
            raise ValueError(f"the weight table has {self.table.size} entries, the model {int(n_levels)} noise levels")

    def weights64(self, alpha_bar, prediction: str = "eps") -> np.ndarray:
        if prediction not in ("eps", "x0", "v"):
            raise ValueError(f"prediction must be one of ('eps', 'x0', 'v'), got {prediction!r}")
        ab = np.asarray(alpha_bar.detach().cpu().numpy() if hasattr(alpha_bar, "detach") else alpha_bar, dtype=np.float64)
        if ab.ndim != 1 or ab.size < 1:
            raise ValueError(f"alpha_bar must be a non-empty vector, got shape {ab.shape}")
        if self.kind == "uniform":
            return np.ones(ab.size, dtype=np.float64)
        if self.kind == "table":
            self.check_levels(ab.size)
            return self.table.copy()
        if not np.all((ab > 0) & (ab < 1)):
            raise ValueError("alpha_bar must lie in (0, 1) for an SNR")
        snr = ab / (1.0 - ab)
        if prediction == "x0":
            return np.minimum(snr, self.gamma)
        if prediction == "v":
            return np.minimum(snr, self.gamma) / (snr + 1.0)
        return np.minimum(1.0, self.gamma / snr)

    def weights(self, alpha_bar, prediction: str = "eps") -> np.ndarray:
        """fp32 [n_levels]: what goes to the device"""
        return self.weights64(alpha_bar, prediction).astype(np.float32)

    # ---- checkpoint payload
    def fields(self) -> dict:
        return {"kind": self.kind, "gamma": self.gamma, "table": None if self.table is None else self.table.tolist()}

    @classmethod
    def from_fields(cls, f) -> Optional["LossWeight"]:
        if f is None:
            return None
        return cls(f["kind"], gamma=f.get("gamma", 5.0), table=f.get("table"))

    def __eq__(self, other):
        if not isinstance(other, LossWeight):
            return NotImplemented
        return self.kind == other.kind and (self.kind != "min_snr" or self.gamma == other.gamma) and \
            (self.table is None) == (other.table is None) and (self.table is None or np.array_equal(self.table, other.table))

    __hash__ = None

    def __repr__(self):
        if self.kind == "min_snr":
            return f"min_snr(gamma={self.gamma:g})"
        return self.kind if self.table is None else f"table[{self.table.size}]"
