"""Clipping the gradient to a maximum global L2 norm (torch.nn.utils.clip_grad_norm_) inside the fused optimizer step.
``include/ib_hip_gradnorm.h`` states the rule, ``csrc/optim.hip`` takes the norm (ib_grad_sumsq) and applies the coefficient
inside the optimizer kernel (ib_optim_step_gradnorm), and this module restates the coefficient on the host.

    total  = sum of float64(g_i)^2                 the device's sum, in its fixed order
    norm_d = sqrt(total) * |float64(grad_scale)|
    coef_d = float64(max_norm) / (norm_d + 1e-6)
    coef   = fp32(coef_d) if coef_d < 1 else 1     torch's rule; NaN gives 1
    gs     = fp32(grad_scale * coef)               one fp32 multiply

The update uses g * gs where it uses g * grad_scale without clipping."""
from __future__ import annotations

from typing import Tuple

import numpy as np


def check_max_grad_norm(v) -> float:
    """the fp32 value the kernel receives: 0 is off, inf measures without clipping; refuses a negative or NaN value"""
    try:
        x = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"max_grad_norm must be a number >= 0, got {v!r}") from None
    if not x >= 0.0:                                    # NaN fails the comparison
        raise ValueError(f"max_grad_norm must be >= 0 and not NaN, got {v}")
    with np.errstate(over="ignore"):
        return float(np.float32(x))


def clip_coef(total: float, grad_scale: float, max_norm: float) -> Tuple[float, float, float]:
    """(norm, coef, gs) of the kernel for the float64 sum of squares `total`, as fp32 values"""
    with np.errstate(all="ignore"):
        gscale = np.float32(grad_scale)
        norm_d = np.sqrt(np.float64(total)) * np.abs(np.float64(gscale))
        coef_d = np.float64(np.float32(max_norm)) / (norm_d + np.float64(1e-6))
        coef = np.float32(coef_d) if coef_d < 1.0 else np.float32(1.0)
        return float(np.float32(norm_d)), float(coef), float(gscale * coef)
