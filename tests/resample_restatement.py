"""Restatements, on the host in float64, of what RePaint resampling of the masked loop computes (diffusion/schedule.py's
resample_walk / resample_coefficients, csrc/resample.hip, DDIMSampler._loop):

  jump_normals      the normals of one jump of one trial, from oracle.ref_cpu.draw_words in domain 4 with float64 Box-Muller
  renoise           one jump over trial tensors: free elements cx x + cz z', observed ones ox x0 + oz z
  gaussian_problem  the 2-D Gaussian inpainting problem of docs/EXPERIMENTS.md and its analytic optimal denoiser
  gaussian_walk     the whole masked loop, plain or resampled, over that problem

Imported by tests/test_resample_plumbing_cpu.py (the statistics) and the two GPU test files (the references)."""
import numpy as np
import torch

from oracle import ref_cpu as R

DOMAIN_JUMP = 4


def jump_normals(frames, D, seed, visit, tid):
    """float64 [frames, D]: element (f, d) of trial `tid` at jump `visit` from block (f D + d) / 4 of counter
    (block, visit, tid, 4), words paired (x, y) -> elements 0, 1 and (z, w) -> elements 2, 3 of the block"""
    n = frames * D
    nb = (n + 3) // 4
    w = (R.draw_words(nb, seed, visit, tid, DOMAIN_JUMP) >> np.uint32(8)).astype(np.float64)
    out = np.empty((nb, 4), dtype=np.float64)
    for a in (0, 2):
        r = np.sqrt(-2.0 * np.log((w[:, a] + 1.0) * 2.0 ** -24))
        th = 2.0 * np.pi * (w[:, a + 1] * 2.0 ** -24)
        out[:, a], out[:, a + 1] = r * np.cos(th), r * np.sin(th)
    return torch.from_numpy(out.reshape(-1)[:n].reshape(frames, D).copy())


def trial_jump_normals(frames, D, ld, seed, visit, ids):
    """float64 [len(ids), frames, ld]: jump_normals per trial id, pad columns 0"""
    Z = torch.zeros(len(ids), frames, ld, dtype=torch.float64)
    for n, i in enumerate(ids):
        Z[n, :, :D] = jump_normals(frames, D, seed, visit, int(i))
    return Z


def renoise(X, X0, Z, obs_cols, coef_row, obs_row, normals):
    """one jump over trial tensors [N, F, ld] in float64: free columns coef_row (x, z'), observed columns (obs_cols [ld]
    bool, or None: every column free) obs_row (x0, z)"""
    want = float(coef_row[0]) * X.double() + float(coef_row[1]) * normals
    if obs_cols is not None:
        pin = float(obs_row[0]) * X0.double() + float(obs_row[1]) * Z.double()
        want = torch.where(obs_cols[None, None, :], pin, want)
    return want


def gaussian_problem(corr=0.9, a=1.5):
    """x ~ N(0, [[1, corr], [corr, 1]]), the first coordinate observed at a -> (mean, std) of the second given the first"""
    return corr * a, (1.0 - corr * corr) ** 0.5


def optimal_eps(x, ab, corr):
    """E[eps | x_t = x] for x_t = sqrt(ab) x0 + sqrt(1 - ab) eps, x0 ~ N(0, C), C = [[1, corr], [corr, 1]]: sqrt(1 - ab)
    (ab C + (1 - ab) I)^-1 x, x [..., 2] float64"""
    p, q = ab + (1.0 - ab), ab * corr                                  # the covariance of x_t is [[p, q], [q, p]], p = 1
    det = p * p - q * q
    s = (1.0 - ab) ** 0.5 / det
    return np.stack([s * (p * x[..., 0] - q * x[..., 1]), s * (p * x[..., 1] - q * x[..., 0])], axis=-1)


def gaussian_walk(S, resample, K, corr=0.9, a=1.5, seed=0, spacing="time", num_train_steps=1000):
    """the free coordinate of K runs of the masked loop, eta = 0, over gaussian_problem in float64 on the project's own
    schedule tables: resample None is the replacement method as ConditionalDDIMSampler runs it, (jump, times) walks
    schedule.resample_walk.  Normals from a numpy generator -> (samples [K], denoiser evaluations)"""
    from inferbiomechanics_amd.diffusion import schedule as sch
    ab = sch.alphas_cumprod(num_train_steps).numpy()
    ts = sch.sample_timesteps(num_train_steps, S, spacing).tolist()
    c2 = sch.ddim_coefficients(num_train_steps, S, spacing).numpy()
    oc = sch.observation_coefficients(num_train_steps, S, spacing).numpy()
    walk = sch.resample_walk(S, *resample) if resample is not None else [("step", p) for p in range(S)]
    rc = sch.resample_coefficients(num_train_steps, S, resample[0], spacing).numpy() if resample is not None else None
    g = np.random.default_rng(seed)
    z = g.standard_normal((K, 2))                                      # the start draw; its first column stays the observed noise
    x = z.copy()
    x[:, 0] = oc[0, 0] * a + oc[0, 1] * z[:, 0]
    evals = 0
    for op in walk:
        if op[0] == "step":
            p = op[1]
            eps = optimal_eps(x, float(ab[ts[p]]), corr)
            x[:, 1] = c2[p, 0] * x[:, 1] + c2[p, 1] * eps[:, 1]
            x[:, 0] = oc[p + 1, 0] * a + oc[p + 1, 1] * z[:, 0]
            evals += 1
        else:
            p, q = op[1], op[1] - resample[0]
            x[:, 1] = rc[p, 0] * x[:, 1] + rc[p, 1] * g.standard_normal(K)
            x[:, 0] = oc[q, 0] * a + oc[q, 1] * z[:, 0]
    return x[:, 1], evals
