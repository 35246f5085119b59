"""Restatements of the three kernels of csrc/cfg.hip (include/ib_hip_cfg.h), on the host: the drop mask from oracle.ref_cpu's
Philox words, the rest as numpy / torch copies and float32 arithmetic with one rounding per operation.  Shared by the CPU and
the GPU tests of classifier-free guidance; no test of its own."""
import numpy as np
import torch

from oracle import ref_cpu as R

DOMAIN_DROP = 3                              # csrc/philox.h: kDomainDrop


def threshold(p: float) -> int:
    """floor(p * 2^32), p in [0, 1]"""
    return int(float(p) * 4294967296.0)


def drop_mask(B: int, p: float, seed: int, step: int, stream_id: int) -> np.ndarray:
    """uint8 [B]: window b is dropped iff word 0 of Philox4x32-10 at counter (b, step, stream_id, 3), key = seed, is below
    floor(p * 2^32).  A function of (seed, step, stream_id, b) alone."""
    thr = threshold(p)
    if thr == 0:
        return np.zeros(B, dtype=np.uint8)
    w0 = R.draw_words(B, seed, step, stream_id, DOMAIN_DROP)[:, 0].astype(np.uint64)
    return (w0 < np.uint64(thr)).astype(np.uint8)


def seed_with_count(B: int, p: float, step: int, stream_id: int, lo: int, hi: int, first: int = 1) -> int:
    """the first seed >= `first` whose mask drops between lo and hi of the B windows"""
    for seed in range(first, first + 1000):
        if lo <= int(drop_mask(B, p, seed, step, stream_id).sum()) <= hi:
            return seed
    raise AssertionError("no seed found")


def q_sample_cond_drop(cond: torch.Tensor, x0: torch.Tensor, mask: np.ndarray, C: int) -> torch.Tensor:
    """cond: ib_q_sample_cond's x_t [B, T, D] for the same operands.  Free columns: its bits; conditioning columns: x0's bits
    in a kept window, +0 in a dropped one"""
    out = cond.clone()
    keep = torch.from_numpy(mask.astype(bool)).logical_not().to(x0.device)
    out[..., :C] = torch.where(keep[:, None, None], x0[..., :C], torch.zeros_like(x0[..., :C]))
    return out


def cfg_combine(eps: torch.Tensor, s: float) -> torch.Tensor:
    """eps [2B, T, ld] (any dtype torch converts exactly to float32) -> the buffer after ib_cfg_combine: the first half is
    round_to_dtype(ec + fl(s * fl(ec - eu))) in float32 numpy, every operation rounded once; the second half as it was"""
    B = eps.shape[0] // 2
    e = eps.detach().cpu().to(torch.float32).numpy()
    ec, eu = e[:B], e[B:]
    d = (ec - eu).astype(np.float32)
    q = (np.float32(s) * d).astype(np.float32)
    g = (ec + q).astype(np.float32)
    out = eps.detach().cpu().clone()
    out[:B] = torch.from_numpy(g).to(eps.dtype)          # float32 -> bfloat16: round to nearest even, as the kernel's store
    return out


def cfg_mirror(x: torch.Tensor, t: torch.Tensor, C: int, D: int):
    """(x [2B, T, ld], t [2B]) after ib_cfg_mirror: columns C .. D-1 and the timesteps of the first half copied to the second"""
    B = x.shape[0] // 2
    x, t = x.detach().cpu().clone(), t.detach().cpu().clone()
    x[B:, :, C:D] = x[:B, :, C:D]
    t[B:] = t[:B]
    return x, t
