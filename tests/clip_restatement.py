"""Restatement of the kernels of csrc/clip.hip (include/ib_hip_clip.h) on the host, in float32 numpy with one rounding per
operation as the header spells them.  A fused multiply-add of float32 values is formed exactly: the product of two float32
is exact in float64, the sum's rounding error is recovered (TwoSum) and folded in as a sticky bit (round to odd), so the one
rounding to float32 that follows is the fma's.  The order statistic of 'dynamic' is numpy.partition on |u|.  Shared by the
CPU and the GPU tests of the x0 clip; no test of its own."""
import numpy as np
import torch


def f32(v):
    return np.asarray(v, dtype=np.float32)


def fma32(a, b, c):
    """fmaf(a, b, c) of float32 arrays, correctly rounded"""
    a, b, c = (f32(v).astype(np.float64) for v in np.broadcast_arrays(a, b, c))
    p = a * b                                                          # exact: 24 + 24 bits
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                                    # exact: p + c == s + err
    odd = (s.view(np.int64) & 1) == 1
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where((err != 0) & ~odd, np.nextafter(s, toward), s)        # round to odd: the sticky bit of the inexact sum
    return s.astype(np.float32)


def widen(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().to(torch.float32).numpy()


def bounded(lo, hi) -> np.ndarray:
    lo, hi = f32(lo), f32(hi)
    return np.isfinite(lo) & np.isfinite(hi) & (hi > lo)


def active(mask, lo, hi, T: int, D: int, ld: int) -> np.ndarray:
    """bool [T, ld]: the free elements of bounded columns (mask [T, ld] non-zero: observed; None: none)"""
    act = np.zeros((T, ld), dtype=bool)
    act[:, :D] = bounded(lo, hi)[None, :]
    if mask is not None:
        act &= np.asarray(mask.detach().cpu().numpy() if isinstance(mask, torch.Tensor) else mask)[:, :ld] == 0
    return act


def predicted_x0(row, x, e):
    ia, sa = f32(row[0]), f32(row[1])
    return fma32(-sa, e, ia * x)                                       # ia * x: float32 times float32, rounded once


def eps_for(row, x, x0c):
    a, is_ = f32(row[2]), f32(row[3])
    return fma32(-a, x0c, x) * is_


def _pad_cols(v, ld, fill):
    out = np.full(ld, fill, dtype=np.float32)
    out[:len(v)] = f32(v)
    return out


def _store(eps: torch.Tensor, new: np.ndarray, changed: np.ndarray) -> torch.Tensor:
    out = eps.detach().cpu().clone()
    ch = torch.from_numpy(changed)
    out[ch] = torch.from_numpy(new).to(eps.dtype)[ch]                  # float32 -> bfloat16: round to nearest even
    return out


def clip_range(x: torch.Tensor, eps: torch.Tensor, mask, lo, hi, row, D: int):
    """-> (eps after ib_x0_clip_range, bool [B, T, ld] of the elements it wrote).  x, eps [B, T, ld]; row = (ia, sa, a, is)"""
    B, T, ld = x.shape
    xv, ev = widen(x), widen(eps)
    act = active(mask, lo, hi, T, D, ld)[None]
    l, h = _pad_cols(lo, ld, 0.0), _pad_cols(hi, ld, 0.0)
    with np.errstate(invalid="ignore"):
        x0 = predicted_x0(row, xv, ev)
        x0c = np.minimum(np.maximum(x0, l), h)
        changed = act & (x0c != x0)
        new = eps_for(row, xv, np.where(changed, x0c, x0))
    return _store(eps, new, changed), changed


def clip_dynamic(x: torch.Tensor, eps: torch.Tensor, mask, lo, hi, m, h, ih, k: int, row, D: int):
    """-> (eps after ib_x0_clip_dynamic, bool [B, T, ld] of the elements it wrote, float32 [B] sw per window)"""
    B, T, ld = x.shape
    xv, ev = widen(x), widen(eps)
    act = active(mask, lo, hi, T, D, ld)
    mm, hh, ii = _pad_cols(m, ld, 0.0), _pad_cols(h, ld, 1.0), _pad_cols(ih, ld, 1.0)
    n = int(act.sum())
    changed = np.zeros((B, T, ld), dtype=bool)
    new = ev.copy()
    sws = np.ones(B, dtype=np.float32)
    if n == 0:
        return eps.detach().cpu().clone(), changed, sws
    kk = min(int(k), n)
    with np.errstate(invalid="ignore", over="ignore"):
        x0 = predicted_x0(row, xv, ev)
        u = (x0 - mm) * ii                                             # two float32 roundings
        for b in range(B):
            au = np.abs(u[b][act])
            q = np.partition(au, kk - 1)[kk - 1]
            sw = np.maximum(q, np.float32(1.0))
            sws[b] = sw
            uc = np.minimum(np.maximum(u[b], -sw), sw) / sw
            x0c = np.where(uc == u[b], x0[b], fma32(hh, uc, mm))
            changed[b] = act & (x0c != x0[b])
            new[b] = eps_for(row, xv[b], np.where(changed[b], x0c, x0[b]))
    return _store(eps, new, changed), changed, sws


def column_range(table: torch.Tensor, T: int, D: int) -> torch.Tensor:
    """fp32 [D, 2]: (amin, amax) per column of the widened values, the pad behind T * D left out"""
    v = table.detach().cpu().to(torch.float32)[:, :T * D].reshape(-1, D)
    return torch.stack([v.amin(dim=0), v.amax(dim=0)], dim=1)
