"""What a denoiser predicts.  ``include/ib_hip_predict.h`` states the kernels' arithmetic (``csrc/predict.hip``); this module
holds the names, the per-level table that keeps a run's reported error in noise units, and float64 restatements of the
target and of the two conversions.  With alpha_t = sqrt(ab_t), sigma_t = sqrt(1 - ab_t) and the state
x_t = alpha_t x0 + sigma_t eps:

    kind    the network's output o approximates     noise prediction from o and x_t
    'eps'   eps                                      o
    'x0'    x0                                       (x_t - alpha_t o) / sigma_t
    'v'     alpha_t eps - sigma_t x0                 alpha_t o + sigma_t x_t           (Salimans & Ho 2022)

An error q = o - target of the network is an error sqrt(u_t) q of the implied noise prediction, u_t = 1, ab_t / (1 - ab_t),
ab_t: the loss launch multiplies the sums it reports by u_t, so the "unweighted" numbers of a run stay the eps-MSE under
every kind and can be compared between runs."""
from __future__ import annotations

import numpy as np

KINDS = ("eps", "x0", "v")


def check_kind(kind) -> str:
    if kind not in KINDS:
        raise ValueError(f"prediction must be one of {KINDS}, got {kind!r}")
    return kind


def _alpha_bar64(alpha_bar) -> np.ndarray:
    ab = np.asarray(alpha_bar.detach().cpu().numpy() if hasattr(alpha_bar, "detach") else alpha_bar, dtype=np.float64)
    if ab.ndim != 1 or ab.size < 1:
        raise ValueError(f"alpha_bar must be a non-empty vector, got shape {ab.shape}")
    if not np.all((ab > 0) & (ab < 1)):
        raise ValueError("alpha_bar must lie in (0, 1)")
    return ab


def eps_units64(alpha_bar, kind: str) -> np.ndarray:
    """float64 [n_levels]: u_t, the factor from the squared error of the network's output to that of the implied noise
    prediction"""
    ab = _alpha_bar64(alpha_bar)
    check_kind(kind)
    if kind == "eps":
        return np.ones(ab.size, dtype=np.float64)
    return ab / (1.0 - ab) if kind == "x0" else ab.copy()


def eps_units(alpha_bar, kind: str) -> np.ndarray:
    """fp32 [n_levels]: what goes to the device"""
    return eps_units64(alpha_bar, kind).astype(np.float32)


def _levels(ab_t, like):
    """(alpha, sigma) of the per-window ab_t, shaped to broadcast over [B, ...] arrays"""
    ab_t = np.asarray(ab_t, dtype=np.float64)
    shape = ab_t.shape + (1,) * (np.ndim(like) - ab_t.ndim)
    return np.sqrt(ab_t).reshape(shape), np.sqrt(1.0 - ab_t).reshape(shape)


def target64(x0, eps, ab_t, kind: str) -> np.ndarray:
    """what the network's output is held against, in float64; ab_t: alpha_bar at each window's level, [B] or a scalar"""
    check_kind(kind)
    x0, eps = np.asarray(x0, dtype=np.float64), np.asarray(eps, dtype=np.float64)
    if kind == "eps":
        return eps.copy()
    if kind == "x0":
        return x0.copy()
    a, s = _levels(ab_t, x0)
    return a * eps - s * x0


def pred_to_eps64(x_t, out, ab_t, kind: str) -> np.ndarray:
    """the noise prediction that the output `out` at the state x_t implies, in float64"""
    check_kind(kind)
    x_t, out = np.asarray(x_t, dtype=np.float64), np.asarray(out, dtype=np.float64)
    if kind == "eps":
        return out.copy()
    a, s = _levels(ab_t, x_t)
    return (x_t - a * out) / s if kind == "x0" else a * out + s * x_t
