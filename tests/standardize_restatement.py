"""Restatement of the kernels of csrc/standardize.hip (include/ib_hip_standardize.h) on the host, in numpy: the affine in
float32 with one rounding per operation the header states (the fused multiply-add formed exactly, as in
tests/clip_restatement.py), bfloat16 by round to nearest even on the bit pattern; the moments as a float64 two-pass mean and
population standard deviation over the values as stored; the finalisation's rule for scale and inv.  Shared by the CPU and
the GPU tests of the standardisation; no test of its own."""
import numpy as np
import torch

from tests.clip_restatement import f32, fma32, widen

STANDARDIZE, DESTANDARDIZE = 0, 1


def bf16_round(v) -> np.ndarray:
    """float32 -> the float32 value bfloat16 keeps: round to nearest, ties to even (finite inputs)"""
    u = f32(v).copy().view(np.uint32)
    u += ((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF)
    u &= np.uint32(0xFFFF0000)
    return u.view(np.float32)


def to_dtype(y, dtype: torch.dtype) -> np.ndarray:
    """the float32 value of y as stored in `dtype`"""
    return bf16_round(y) if dtype == torch.bfloat16 else f32(y)


def affine(x, a, b, mode: int) -> np.ndarray:
    """float32: mode 0  d = x - a, y = d * b (two roundings);  mode 1  y = fma(x, b, a), or x * b when a is None.
    a, b broadcast along the last axis of x."""
    x, b = f32(x), f32(b)
    if mode == STANDARDIZE:
        return (x - f32(a)) * b
    return x * b if a is None else fma32(x, b, f32(a))


def affine_into(dst: torch.Tensor, x: torch.Tensor, a, b, mode: int, cols=None) -> np.ndarray:
    """the float32 image of dst [..., ld] after ib_column_affine over x [..., ld'] and the column window cols = (c0, w)
    (default: all len(b) columns): the window's elements replaced, everything else as it was"""
    c0, w = (0, len(b)) if cols is None else cols
    out = widen(dst).copy()
    av = None if a is None else f32(a)[c0:c0 + w]
    out[..., c0:c0 + w] = to_dtype(affine(widen(x)[..., c0:c0 + w], av, f32(b)[c0:c0 + w], mode), dst.dtype)
    return out


def bits(v) -> np.ndarray:
    return f32(v).view(np.uint32)


def moments_ref(rows):
    """float64 two-pass (mean, population standard deviation) per column of rows [R, D], the values as stored"""
    v = np.asarray(rows, dtype=np.float64)
    mean = v.sum(axis=0) / v.shape[0]
    sd = np.sqrt(((v - mean) ** 2).sum(axis=0) / v.shape[0])
    return mean, sd


def table_rows(table: torch.Tensor, T: int, D: int) -> np.ndarray:
    """float64 [N * T, D]: the rows of a window table [N, pitch], the pad behind T * D left out"""
    return table.detach().cpu().to(torch.float64)[:, :T * D].reshape(-1, D).numpy()


def inv_rule(scale) -> np.ndarray:
    """inv = (float)(1.0 / (double)scale)"""
    return (1.0 / f32(scale).astype(np.float64)).astype(np.float32)


def finalize_rule(s, min_std: float):
    """(scale, inv) from the float32 standard deviation s: scale = s > min_std ? s : 1"""
    s = f32(s)
    scale = np.where(s > np.float32(min_std), s, np.float32(1.0)).astype(np.float32)
    return scale, inv_rule(scale)


def ulp32(v) -> np.ndarray:
    """the spacing of float32 at |v|"""
    return np.spacing(np.abs(f32(v))).astype(np.float64)
