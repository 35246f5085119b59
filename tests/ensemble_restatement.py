"""The order statistics of an ensemble (csrc/ensemble.hip, include/ib_hip_ensemble.h) restated in numpy: `restate` does
numpy.sort on float32 and then the header's formulas in float32, in the stated order, one rounding per operation -- what the
kernel must equal as numbers; `reference` is a float64 brute force of the same quantities (the CRPS by its O(K^2) double sum),
against which the restatement's own rounding error is bounded (`crps_bound`)."""
import numpy as np

U = 2.0 ** -24                               # unit roundoff of float32


def members_of(x, c0: int, w: int) -> np.ndarray:
    """x [B, K, rows, ld] (a torch tensor of any float dtype, any device) -> float32 [K, B * rows * w]: the members of every
    element of the column window, elements in the order of the kernel's outputs.  bf16 widens exactly."""
    x = x.detach().float().cpu().numpy()
    B, K, rows, _ = x.shape
    return np.ascontiguousarray(x[:, :, :, c0:c0 + w].transpose(1, 0, 2, 3).reshape(K, B * rows * w))


def restate(m: np.ndarray, pos, y=None) -> dict:
    """m float32 [K, n], pos = ((i, f) for lo, median, hi) from diffusion.ensemble.quantile_position, y float32 [n] or None"""
    assert m.dtype == np.float32 and m.ndim == 2
    K = m.shape[0]
    s = np.sort(m, axis=0)

    def Q(i, f):
        a, b = s[i], s[min(i + 1, K - 1)]
        d = b - a
        t = np.float32(f) * d
        return a + t

    out = {k: Q(*p) for k, p in zip(("lo", "median", "hi"), pos)}
    assert all(v.dtype == np.float32 for v in out.values())
    if y is None:
        return out
    y = np.asarray(y)
    assert y.dtype == np.float32 and y.shape == (m.shape[1],)
    A = np.zeros_like(y)
    G = np.zeros_like(y)
    for i in range(K):
        A = A + np.abs(s[i] - y)
        G = G + np.float32(2 * i - K + 1) * s[i]
    crps = A / np.float32(K)
    if K > 1:
        crps = crps - G / np.float32(K * (K - 1))
    assert crps.dtype == np.float32
    out.update(crps=crps, A=A, G=G, rank=(m < y).sum(axis=0).astype(np.uint8),
               inside=((out["lo"] <= y) & (y <= out["hi"])).astype(np.uint8))
    return out


def reference(m: np.ndarray, pos, y=None) -> dict:
    """the same in float64, by brute force: G and the CRPS' spread term are the double sum over pairs"""
    m = m.astype(np.float64)
    K = m.shape[0]
    s = np.sort(m, axis=0)
    Q = lambda i, f: s[i] + float(np.float32(f)) * (s[min(i + 1, K - 1)] - s[i])
    out = {k: Q(*p) for k, p in zip(("lo", "median", "hi"), pos)}
    if y is None:
        return out
    y = np.asarray(y, dtype=np.float64)
    A = np.abs(m - y).sum(axis=0)
    G = np.zeros_like(y)
    for i in range(K):
        for j in range(i + 1, K):
            G += np.abs(m[j] - m[i])
    crps = A / K - (G / (K * (K - 1)) if K > 1 else 0.0)
    out.update(crps=crps, A=A, G=G, rank=(m < y).sum(axis=0), inside=(out["lo"] <= y) & (y <= out["hi"]))
    return out


def crps_bound(m: np.ndarray, y) -> np.ndarray:
    """first-order bound of |restated CRPS - float64 CRPS| per element: (K + 2) u (A / K + sum_i |2i - K + 1| |s_i| / (K (K - 1)))
    -- each sum of K terms carries at most K - 1 additions and one rounding per term (the difference, or the product), the
    division one more"""
    m = m.astype(np.float64)
    K = m.shape[0]
    s = np.sort(m, axis=0)
    A = np.abs(m - np.asarray(y, dtype=np.float64)).sum(axis=0)
    wgt = np.abs(2.0 * np.arange(K) - K + 1)[:, None]
    spread = (wgt * np.abs(s)).sum(axis=0) / (K * (K - 1)) if K > 1 else 0.0
    return (K + 2) * U * (A / K + spread)
