"""A temporal-difference (velocity) term on the predicted clean window.  ``include/ib_hip_velocity.h`` states the kernel's
arithmetic, ``csrc/velocity.hip`` computes the term inside the loss launch of the fused step, and this module makes its two
per-level tables on the host, in float64, cast to fp32 once, and restates the whole launch in float64.

The term is the "geometric loss" of motion diffusion (MDM, Tevet et al. 2023): the squared error of the frame difference of
the predicted x0,

    L_vel = mean over windows, frames f < T-1, scored columns of  m_t ((x0hat[f+1] - x0hat[f]) - (x0[f+1] - x0[f]))^2

For every prediction kind the error of the implied x0 is a per-window constant times the error q = o - target of the
network's output: x0hat - x0 = c_t q with c_t^2 = 1 / snr_t (eps), 1 (x0), 1 - ab_t = 1 / (snr_t + 1) (v).  So

    vtab_t = lambda m_t c_t^2      the weight of (q[f+1] - q[f])^2 in the optimised loss
    xtab_t = c_t^2                 puts the reported velocity error in x0 units

with m_t = min(snr_t, gamma), the truncated-SNR weighting loss_weight.py uses for x0 (gamma = inf: the plain snr), or the
caller's table[t].  With the default rule vtab / lambda is Min-SNR in the form of the kind: min(1, gamma / snr) for eps,
min(snr, gamma) for x0, min(snr, gamma) / (snr + 1) for v.  The optimised loss of a step with the term is

    mean(w_t q^2) + mean over f < T-1 of (vtab_t (q[f+1] - q[f])^2)

both plain means: neither is divided by the sum of its weights."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

from .hip import LOSS_LEVEL_BUCKETS as LEVEL_BUCKETS
from .prediction import _alpha_bar64, check_kind


def check_weight(v) -> float:
    try:
        x = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"the velocity-loss weight must be a number > 0, got {v!r}") from None
    if not (x > 0.0 and np.isfinite(x)):                # NaN fails the comparison
        raise ValueError(f"the velocity-loss weight must be > 0 and finite, got {v}")
    return x


def check_gamma(v) -> float:
    """gamma > 0; inf is allowed: m_t = snr_t"""
    try:
        x = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"the velocity-loss gamma must be a number > 0, got {v!r}") from None
    if not x > 0.0:                                     # NaN fails the comparison
        raise ValueError(f"the velocity-loss gamma must be > 0, got {v}")
    return x


def x0_units64(alpha_bar, kind: str) -> np.ndarray:
    """float64 [n_levels]: c_t^2, the factor from the squared error of the network's output to that of the implied x0"""
    ab = _alpha_bar64(alpha_bar)
    check_kind(kind)
    if kind == "x0":
        return np.ones(ab.size, dtype=np.float64)
    return (1.0 - ab) / ab if kind == "eps" else 1.0 - ab


class VelocityLoss:
    """VelocityLoss(weight, gamma=5.0) / VelocityLoss(weight, table=values): weight = lambda > 0"""

    def __init__(self, weight: float, gamma: float = 5.0, table=None):
        self.weight = check_weight(weight)
        self.gamma = check_gamma(gamma)
        self.table: Optional[np.ndarray] = None
        if table is not None:
            tb = np.asarray(table.detach().cpu().numpy() if hasattr(table, "detach") else table, dtype=np.float64)
            if tb.ndim != 1 or tb.size < 1:
                raise ValueError(f"the velocity-loss table must be a non-empty vector, got shape {tb.shape}")
            if not np.all(np.isfinite(tb)) or np.any(tb < 0):
                raise ValueError("the velocity-loss table must be finite and >= 0")
            self.table = tb.copy()

    def check_levels(self, n_levels: int):
        """a table must have one entry per noise level of the model (HipTrainer's constructor calls this)"""
        if self.table is not None and self.table.size != int(n_levels):
            raise ValueError(f"the velocity-loss table has {self.table.size} entries, the model {int(n_levels)} noise levels")

    def level_weights64(self, alpha_bar) -> np.ndarray:
        """float64 [n_levels]: m_t, the weight of the squared x0-velocity error at each level"""
        ab = _alpha_bar64(alpha_bar)
        if self.table is not None:
            self.check_levels(ab.size)
            return self.table.copy()
        return np.minimum(ab / (1.0 - ab), self.gamma)

    def tables64(self, alpha_bar, kind: str) -> Tuple[np.ndarray, np.ndarray]:
        """(vtab, xtab) in float64"""
        ab = _alpha_bar64(alpha_bar)
        check_kind(kind)
        if self.table is not None:
            self.check_levels(ab.size)
            return self.weight * self.table * x0_units64(ab, kind), x0_units64(ab, kind)
        # the three closed forms, each written so that no factor of m_t c_t^2 is rounded twice
        snr = ab / (1.0 - ab)
        if kind == "eps":
            m = np.minimum(1.0, self.gamma / snr)
        elif kind == "x0":
            m = np.minimum(snr, self.gamma)
        else:
            m = np.minimum(snr, self.gamma) / (snr + 1.0)
        return self.weight * m, x0_units64(ab, kind)

    def tables(self, alpha_bar, kind: str) -> Tuple[np.ndarray, np.ndarray]:
        """(vtab, xtab) in fp32: what goes to the device"""
        v, x = self.tables64(alpha_bar, kind)
        return v.astype(np.float32), x.astype(np.float32)

    # ---- checkpoint payload
    def fields(self) -> dict:
        return {"weight": self.weight, "gamma": self.gamma, "table": None if self.table is None else self.table.tolist()}

    @classmethod
    def from_fields(cls, f) -> Optional["VelocityLoss"]:
        if f is None:
            return None
        return cls(f["weight"], gamma=f.get("gamma", 5.0), table=f.get("table"))

    def __eq__(self, other):
        if not isinstance(other, VelocityLoss):
            return NotImplemented
        return self.weight == other.weight and (self.table is not None or self.gamma == other.gamma) and \
            (self.table is None) == (other.table is None) and (self.table is None or np.array_equal(self.table, other.table))

    __hash__ = None

    def __repr__(self):
        rule = f"gamma={self.gamma:g}" if self.table is None else f"table[{self.table.size}]"
        return f"velocity(weight={self.weight:g}, {rule})"


def velocity_terms64(pred, x0, eps, t, alpha_bar, kind: str, wtab, utab, vtab, xtab, cond_cols: int = 0,
                     buckets: int = LEVEL_BUCKETS, target=None) -> dict:
    """ib_vel_loss_partial + ib_vel_loss_finalize restated in float64 torch, on any device, differentiable in `pred`.
    pred / x0 / eps: [B, T, D]; t: integer [B] (clamped into the tables as the kernel clamps it); alpha_bar and the four
    tables: [n_levels] (pass the fp32 tables the device holds to restate a launch exactly).  target, [B, T, D]: what the
    output is held against where the caller has formed it already -- the kernel's own fp32 target of kind 'v', say -- in
    place of the float64 target of `kind`.  Returns
      "loss" = "mse" + "vel", "mse" = mean(w q^2), "vel" = mean over f < T-1 of (v dn^2)     torch scalars with a graph
      "eps_mse" = mean(u q^2), "bands" [NB] its sums per band, "counts" [NB] the windows per band
      "x0_vel" = mean over f < T-1 of (x dn^2), "x0_bands" [NB] its sums per band
      "dpred" [B, T, D] the analytic gradient of "loss" (dm + dv, zero on the conditioning columns), "dm", "dp", "dn" its
      parts and "gscale", "vscale", "v" ([B, 1, 1]) the factors: dv = (dp - dn) * vscale * v."""
    import torch
    check_kind(kind)
    f64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64) if not isinstance(a, torch.Tensor) else a).to(torch.float64)
    pred = pred if isinstance(pred, torch.Tensor) and pred.dtype == torch.float64 else f64(pred)
    dev = pred.device
    x0, eps = f64(x0).to(dev), f64(eps).to(dev)
    B, T, D = pred.shape
    C = int(cond_cols)
    if T < 2:
        raise ValueError(f"a frame difference needs windows of at least 2 frames, got {T}")
    if not 0 <= C < D:
        raise ValueError(f"cond_cols must lie in [0, {D}), got {C}")
    ab = f64(alpha_bar).to(dev)
    n_levels = ab.numel()
    tl = torch.as_tensor(t).to(dev).to(torch.int64).clamp(0, n_levels - 1)
    lvl = lambda tab: f64(tab).to(dev)[tl].view(B, 1, 1)
    w, u, v, x = lvl(wtab), lvl(utab), lvl(vtab), lvl(xtab)
    a, s = ab[tl].sqrt().view(B, 1, 1), (1.0 - ab[tl]).sqrt().view(B, 1, 1)
    if target is not None:
        target = f64(target).to(dev)
    else:
        target = eps if kind == "eps" else (x0 if kind == "x0" else a * eps - s * x0)
    scored = torch.zeros(D, dtype=torch.float64, device=dev)
    scored[C:] = 1.0
    q = (pred - target) * scored
    dn = torch.zeros_like(q)
    dn[:, :-1] = q[:, 1:] - q[:, :-1]                  # 0 at f = T-1
    dp = torch.zeros_like(q)
    dp[:, 1:] = dn[:, :-1]                             # 0 at f = 0
    n, n_v = B * T * (D - C), B * (T - 1) * (D - C)
    mse, vel = (w * q * q).sum() / n, (v * dn * dn).sum() / n_v
    band = tl * int(buckets) // n_levels
    per_w_eps, per_w_x0 = (u * q * q).sum(dim=(1, 2)), (x * dn * dn).sum(dim=(1, 2))
    bands = torch.zeros(buckets, dtype=torch.float64, device=dev).index_add(0, band, per_w_eps.detach())
    x0_bands = torch.zeros(buckets, dtype=torch.float64, device=dev).index_add(0, band, per_w_x0.detach())
    counts = torch.bincount(band, minlength=buckets)
    gscale, vscale = 2.0 / n, 2.0 / n_v
    qd, dnd, dpd = q.detach(), dn.detach(), dp.detach()
    dm = qd * gscale * w
    return {"loss": mse + vel, "mse": mse, "vel": vel, "eps_mse": per_w_eps.detach().sum() / n, "bands": bands,
            "counts": counts, "x0_vel": per_w_x0.detach().sum() / n_v, "x0_bands": x0_bands,
            "dpred": dm + (dpd - dnd) * vscale * v, "dm": dm, "dp": dpd, "dn": dnd, "gscale": gscale, "vscale": vscale, "v": v}
