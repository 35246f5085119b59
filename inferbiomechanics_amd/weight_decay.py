"""Decoupled weight decay of the fused optimizer (Loshchilov & Hutter; with Adam: torch.optim.AdamW).
``include/ib_hip_decay.h`` states the rule, ``csrc/optim.hip`` applies it inside the optimizer kernel, and this module
restates the factor on the host and builds the table of decayed ranges.

    f   = fp32(1 - fp32(lr_s) * fp32(wd))      the product and the difference in float64, rounded to fp32 once
    p'  = fp32(p * f)                          one fp32 multiply of its own
    p_new, s1, s2 = the optimizer's update of (p', g)

lr_s is the fp32 rate of the step: the base rate, or ``LrSchedule.lr_at(base, step)`` under a schedule.  The product of two
fp32 values is exact in float64, so ``decay_factor`` is bitwise the kernel's f.

Which elements: by default the parameters with ``ndim >= 2`` (weight matrices, embedding tables); biases and normalisation
gains / offsets are left alone.  A ``decay_filter(name, shape) -> bool`` overrides the rule."""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np


def _f32(x: float) -> float:
    return float(np.float32(x))


def decay_factor(lr: float, wd: float) -> float:
    """f of the kernel for the fp32 rate `lr` and the fp32 decay `wd`: an fp32 value.  Exactly 1.0 for wd = 0."""
    return _f32(1.0 - _f32(lr) * _f32(wd))


def default_decay_filter(name: str, shape: Sequence[int]) -> bool:
    """weight matrices and embedding tables are decayed, biases and LayerNorm / BatchNorm gains and offsets are not"""
    return len(tuple(shape)) >= 2


def check_weight_decay(wd) -> float:
    """the fp32 value the kernel receives; refuses a negative, NaN or infinite decay"""
    try:
        v = float(wd)
    except (TypeError, ValueError):
        raise ValueError(f"weight_decay must be a number >= 0, got {wd!r}") from None
    if not 0.0 <= v < float("inf"):                     # NaN fails the comparison
        raise ValueError(f"weight_decay must be finite and >= 0, got {wd}")
    return _f32(v)


def decayed_names(shapes: Dict[str, Tuple[int, ...]], decay_filter: Optional[Callable] = None) -> List[str]:
    """the names the rule selects, in the order of `shapes`"""
    rule = default_decay_filter if decay_filter is None else decay_filter
    return [k for k, shp in shapes.items() if bool(rule(k, tuple(shp)))]


def decay_ranges(layout: Dict[str, Tuple[int, int]], names: Sequence[str], align: int = 64) -> List[Tuple[int, int]]:
    """(start, len) of the decayed ranges in flat-buffer coordinates, sorted and disjoint.  A parameter's range runs to the end
    of its alignment padding (the padding belongs to it), so two decayed neighbours touch and are merged into one range."""
    out: List[List[int]] = []
    for off, n in sorted(layout[k] for k in names):
        end = -(-(off + n) // align) * align
        if out and out[-1][0] + out[-1][1] == off:
            out[-1][1] = end - out[-1][0]
        else:
            out.append([off, end - off])
    return [(a, b) for a, b in out]
