"""Learning-rate schedules of the fused optimizer: a linear warmup, then a constant rate or a linear / cosine decay to
``min_ratio`` times the base rate.  ``include/ib_hip_sched.h`` states the rule, ``csrc/optim.hip`` (lr_scheduled) evaluates it
inside the optimizer kernel from the device step counter, and ``LrSchedule.lr_at`` restates it on the host in float64: the
same operations in the same order, each rounded on its own, the result rounded to fp32 once.  The two agree bitwise except
where the last place of the device's double cos() flips that final rounding (cosine decay only, one fp32 ulp at the most).

    s <= w             f = s / w
    s >  w, constant   f = 1
    otherwise          u = min(1, (s - w) / (T - w));  f = m + (1 - m) * (1 - u)                    linear
                                                       f = m + (1 - m) * (0.5 * (1 + cos(pi * u)))  cosine
    lr_s = fp32(fp32(lr) * f)

s is the 1-based step number (the one the bias corrections use).  Step 1 runs at lr / w, step w at lr, step T and every
later step at m * lr."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np

KINDS = {"constant": 0, "linear": 1, "cosine": 2}          # IB_SCHED_* of include/ib_hip_sched.h
_I32_MAX = (1 << 31) - 1


def _f32(x: float) -> float:
    return float(np.float32(x))


@dataclass(frozen=True)
class LrSchedule:
    """kind: 'constant' | 'linear' | 'cosine'; warmup >= 0 steps; total: the step at which the decay reaches min_ratio (a
    decay needs total > warmup; a constant schedule ignores it); min_ratio in [0, 1], held as the fp32 value the kernel
    receives."""
    kind: str = "constant"
    warmup: int = 0
    total: int = 0
    min_ratio: float = 0.0

    def __post_init__(self):
        if self.kind not in KINDS:
            raise ValueError(f"lr schedule kind must be one of {sorted(KINDS)}, got {self.kind!r}")
        for name in ("warmup", "total"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"lr schedule {name} must be an integer, got {v!r}")
            if not 0 <= int(v) <= _I32_MAX:
                raise ValueError(f"lr schedule {name} must lie in [0, 2^31), got {v}")
            object.__setattr__(self, name, int(v))
        if self.kind != "constant" and self.total <= self.warmup:
            raise ValueError(f"a {self.kind} lr schedule needs total steps > warmup steps, got total = {self.total} and "
                             f"warmup = {self.warmup}")
        try:
            m = float(self.min_ratio)
        except (TypeError, ValueError):
            raise ValueError(f"lr schedule min_ratio must be a number in [0, 1], got {self.min_ratio!r}") from None
        if not 0.0 <= m <= 1.0:                                 # NaN fails both comparisons
            raise ValueError(f"lr schedule min_ratio must lie in [0, 1], got {self.min_ratio}")
        object.__setattr__(self, "min_ratio", _f32(m))

    @property
    def kind_code(self) -> int:
        return KINDS[self.kind]

    def is_constant(self) -> bool:
        """no warmup and no decay: every step runs at the base rate, through the entry points without a schedule"""
        return self.kind == "constant" and self.warmup == 0

    def factor(self, s: int) -> float:
        """f of step s (1-based), float64"""
        s, w, T, m = int(s), self.warmup, self.total, self.min_ratio
        if s <= w:
            return s / w
        if self.kind == "constant":
            return 1.0
        u = min(1.0, (s - w) / (T - w))
        shape = 0.5 * (1.0 + math.cos(math.pi * u)) if self.kind == "cosine" else 1.0 - u
        return m + (1.0 - m) * shape

    def lr_at(self, base_lr: float, s: int) -> float:
        """the rate of step s (1-based), an fp32 value: what the kernel puts in lr's place"""
        return _f32(_f32(base_lr) * self.factor(s))

    def fields(self) -> Dict:
        """the four fields as plain values (a checkpoint's "lr_schedule")"""
        return {"kind": self.kind, "warmup": self.warmup, "total": self.total, "min_ratio": self.min_ratio}

    @classmethod
    def from_fields(cls, d: Optional[Dict]) -> Optional["LrSchedule"]:
        return None if d is None else cls(str(d["kind"]), int(d["warmup"]), int(d["total"]), float(d["min_ratio"]))

    def __str__(self) -> str:
        return f"{self.kind}(warmup={self.warmup}, total={self.total}, min_ratio={self.min_ratio:g})"


def active(schedule: Optional[LrSchedule]) -> Optional[LrSchedule]:
    """the schedule if it changes any step's rate, else None (None and a constant schedule without warmup are the same run)"""
    return None if schedule is None or schedule.is_constant() else schedule
