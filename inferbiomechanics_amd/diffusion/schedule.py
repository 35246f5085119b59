"""[BUILD-DEFINED] DDPM / DDIM schedule tables (no reference counterpart).

Everything is computed in float64 on the host exactly as the oracle does (literature definitions:
linear beta schedule 1e-4..0.02 over 1000 steps, alpha_bar = cumprod(1-beta); DDIM with eta in [0, 1]; sinusoidal
embedding [sin(t w_i), cos(t w_i)], w_i = exp(-ln(1e4) i / half)), cast ONCE to fp32 and uploaded; the
kernels only index the tables, so schedule values and timestep indices are bit-exact.
"""
import math
from typing import Dict, Optional

import torch


def linear_beta_schedule(num_steps: int = 1000, beta_start: float = 1e-4, beta_end: float = 0.02) -> torch.Tensor:
    return torch.linspace(beta_start, beta_end, num_steps, dtype=torch.float64)


def alphas_cumprod(num_steps: int = 1000) -> torch.Tensor:
    return torch.cumprod(1.0 - linear_beta_schedule(num_steps), dim=0)


def ddim_timesteps(num_train_steps: int = 1000, num_sample_steps: int = 100) -> torch.Tensor:
    if num_train_steps % num_sample_steps:
        raise ValueError("num_sample_steps must divide num_train_steps")
    stride = num_train_steps // num_sample_steps
    return torch.arange(num_sample_steps - 1, -1, -1, dtype=torch.int64) * stride


def log_snr(num_train_steps: int = 1000) -> torch.Tensor:
    """[N] float64: lambda_t = 1/2 log(alpha_bar_t / (1 - alpha_bar_t)), the half log-SNR; strictly decreasing in t"""
    ab = alphas_cumprod(num_train_steps)
    return 0.5 * torch.log(ab / (1.0 - ab))


SPACINGS = ("time", "logsnr")
SOLVERS = ("ddim", "dpmpp2m", "dpmpp2m_sde")
OBSERVATIONS = ("noised", "clean")


def check_sampler_settings(eta: float, solver: str, spacing: str, observations: str = "noised"):
    """the refusals of a sampling loop's settings, for the sampler constructors and DiffusionTables.set_sampler alike"""
    if not 0.0 <= float(eta) <= 1.0:
        raise ValueError(f"eta must be in [0, 1], got {eta}")
    if solver not in SOLVERS:
        raise ValueError(f"solver must be one of {SOLVERS}, got {solver!r}")
    if spacing not in SPACINGS:
        raise ValueError(f"spacing must be one of {SPACINGS}, got {spacing!r}")
    if solver == "dpmpp2m" and float(eta) > 0.0:
        raise ValueError("solver 'dpmpp2m' is deterministic: it needs eta = 0")
    if observations not in OBSERVATIONS:
        raise ValueError(f"observations must be one of {OBSERVATIONS}, got {observations!r}")


def sample_timesteps(num_train_steps: int = 1000, num_sample_steps: int = 100, spacing: str = "time") -> torch.Tensor:
    """[S] int64, strictly decreasing: the sampling grid.  'time' is ddim_timesteps (uniform in t, needs S | N).  'logsnr' is
    uniform in lambda: S targets from lambda_{N-1} to lambda_0, each rounded to the timestep whose lambda is nearest; the
    linear beta schedule packs much of the lambda range into the last few timesteps, so neighbouring targets can round to
    one timestep there -- strict decrease is then forced from the clean end, t[S-1] = nearest, t[i] = max(nearest[i],
    t[i+1] + 1).  Needs no S | N; an S so large that the forcing would pass N - 1 is an error."""
    if spacing == "time":
        return ddim_timesteps(num_train_steps, num_sample_steps)
    if spacing != "logsnr":
        raise ValueError(f"spacing must be one of {SPACINGS}, got {spacing!r}")
    N, S = int(num_train_steps), int(num_sample_steps)
    if S < 1:
        raise ValueError("num_sample_steps must be at least 1")
    lam = log_snr(N)
    targets = torch.linspace(float(lam[N - 1]), float(lam[0]), S, dtype=torch.float64)
    up = lam.flip(0)                                                       # ascending: up[j] = lambda_{N-1-j}
    hi = torch.searchsorted(up, targets).clamp(1, N - 1)                   # up[hi - 1] < target <= up[hi]
    hi = torch.where(targets - up[hi - 1] < up[hi] - targets, hi - 1, hi)  # the nearer neighbour; a tie takes the smaller t
    nearest = (N - 1 - hi).tolist()
    ts = list(nearest)
    for i in range(S - 2, -1, -1):
        ts[i] = max(nearest[i], ts[i + 1] + 1)
    if ts[0] > N - 1:
        raise ValueError(f"no strictly decreasing log-SNR grid of {S} steps fits {N} training steps")
    return torch.tensor(ts, dtype=torch.int64)


def ddim_coefficients(num_train_steps: int = 1000, num_sample_steps: int = 100, spacing: str = "time") -> torch.Tensor:
    """[S, 2] float64 (c_x, c_eps): x_prev = c_x x_t + c_eps eps (eta = 0; last step goes to alpha_bar = 1)."""
    ab = alphas_cumprod(num_train_steps)
    ts = sample_timesteps(num_train_steps, num_sample_steps, spacing).tolist()
    rows = []
    for i, t in enumerate(ts):
        ab_t = ab[t]
        ab_p = ab[ts[i + 1]] if i + 1 < len(ts) else torch.tensor(1.0, dtype=torch.float64)
        cx = torch.sqrt(ab_p) / torch.sqrt(ab_t)
        ce = torch.sqrt(1 - ab_p) - torch.sqrt(ab_p) * torch.sqrt(1 - ab_t) / torch.sqrt(ab_t)
        rows.append(torch.stack([cx, ce]))
    return torch.stack(rows)


def observation_coefficients(num_train_steps: int = 1000, num_sample_steps: int = 100, spacing: str = "time") -> torch.Tensor:
    """[S + 1, 2] float64 (c_x0, c_z) of the masked (inpainting) loop: an observed element is x0 forward-noised with the
    fixed draw z to the loop's noise level, c_x0 x0 + c_z z.  Row 0 = (sqrt ab[t_0], sqrt(1 - ab[t_0])) is the start state;
    row s + 1 = (sqrt ab_prev(s), sqrt(1 - ab_prev(s))) is the level after step s, so the last row is exactly (1, 0)."""
    ab = alphas_cumprod(num_train_steps)
    ts = sample_timesteps(num_train_steps, num_sample_steps, spacing).tolist()
    levels = [ab[ts[0]]] + [ab[ts[i + 1]] if i + 1 < len(ts) else torch.tensor(1.0, dtype=torch.float64)
                            for i in range(len(ts))]
    return torch.stack([torch.stack([torch.sqrt(a), torch.sqrt(1 - a)]) for a in levels])


def clean_observation_coefficients(num_train_steps: int = 1000, num_sample_steps: int = 100,
                                   spacing: str = "time") -> torch.Tensor:
    """[S + 1, 2] float64, every row (1, 0): the observation table of a denoiser trained on clean conditioning columns
    (`train --cond-cols`).  An observed element is then c_x0 x0 + c_z z = the observation itself in the start state and after
    every step, through the update kernels the noised table goes through.  Same shape as observation_coefficients (the
    grid only fixes the row count)."""
    S = int(sample_timesteps(num_train_steps, num_sample_steps, spacing).numel())
    out = torch.zeros((S + 1, 2), dtype=torch.float64)
    out[:, 0] = 1.0
    return out


def _levels(num_train_steps: int, num_sample_steps: int, spacing: str = "time"):
    """(alpha_bar[t_s], alpha_bar of the next level) per sampling step, float64; the last step goes to alpha_bar = 1"""
    ab = alphas_cumprod(num_train_steps)
    ts = sample_timesteps(num_train_steps, num_sample_steps, spacing).tolist()
    one = torch.tensor(1.0, dtype=torch.float64)
    return [(ab[t], ab[ts[i + 1]] if i + 1 < len(ts) else one) for i, t in enumerate(ts)]


def ddim_sigmas(num_train_steps: int = 1000, num_sample_steps: int = 100, eta: float = 0.0,
                spacing: str = "time") -> torch.Tensor:
    """[S] float64: sigma_s = eta sqrt((1 - p) / (1 - a)) sqrt(1 - a / p) (Song et al., DDIM eq. 16); eta = 1 with S = N is
    the DDPM posterior's standard deviation.  Exactly 0 at eta = 0 and in the last row (p = 1)."""
    if not 0.0 <= float(eta) <= 1.0:
        raise ValueError(f"eta must be in [0, 1], got {eta}")
    return torch.stack([float(eta) * torch.sqrt((1 - p) / (1 - a)) * torch.sqrt(1 - a / p)
                        for a, p in _levels(num_train_steps, num_sample_steps, spacing)])


def ddim_coefficients_eta(num_train_steps: int = 1000, num_sample_steps: int = 100, eta: float = 0.0,
                          spacing: str = "time") -> torch.Tensor:
    """[S, 3] float64 (c_x, c_eps, sigma): x_prev = c_x x_t + c_eps eps + sigma z', z' ~ N(0, I).  c_x does not depend on
    eta; c_eps = sqrt(1 - p - sigma^2) - sqrt(p) sqrt(1 - a) / sqrt(a).  At eta = 0 the first two columns are
    ddim_coefficients bit for bit."""
    sig = ddim_sigmas(num_train_steps, num_sample_steps, eta, spacing)
    rows = []
    for (a, p), sg in zip(_levels(num_train_steps, num_sample_steps, spacing), sig):
        cx = torch.sqrt(p) / torch.sqrt(a)
        ce = torch.sqrt(1 - p - sg * sg) - torch.sqrt(p) * torch.sqrt(1 - a) / torch.sqrt(a)
        rows.append(torch.stack([cx, ce, sg]))
    return torch.stack(rows)


def observation_noise_coefficients(num_train_steps: int = 1000, num_sample_steps: int = 100, eta: float = 0.0,
                                   spacing: str = "time") -> torch.Tensor:
    """[S, 2] float64 (r, q): an observed element of the masked loop follows the DDIM posterior given the observation,
    q_sigma(x_prev | x_t, x0).  With e the element's current noise (x_t = sqrt(a) x0 + sqrt(1 - a) e), the noise of the next
    level is e' = r e + q z' with r = sqrt(1 - p - sigma^2) / sqrt(1 - p), q = sigma / sqrt(1 - p), r^2 + q^2 = 1.  Exactly
    (1, 0) at eta = 0 (e stays the start draw); (0, 0) in the last row, where the level is the observation itself."""
    sig = ddim_sigmas(num_train_steps, num_sample_steps, eta, spacing)
    rows = []
    for (a, p), sg in zip(_levels(num_train_steps, num_sample_steps, spacing), sig):
        if float(p) == 1.0:
            rows.append(torch.zeros(2, dtype=torch.float64))
        else:
            rows.append(torch.stack([torch.sqrt(1 - p - sg * sg) / torch.sqrt(1 - p), sg / torch.sqrt(1 - p)]))
    return torch.stack(rows)


def dpmpp_coefficients(num_train_steps: int = 1000, num_sample_steps: int = 100, spacing: str = "time") -> torch.Tensor:
    """[S, 5] float64 (A, E, C, hx, he) of DPM-Solver++(2M) (Lu et al. 2022, Algorithm 2; data prediction, multistep):
    x' = A x + E eps + C h_prev, and the history the next step reads is h = hx x + he eps = (x - sigma_s eps) / alpha_s, the
    data prediction at this step's level (alpha = sqrt(alpha_bar), sigma = sqrt(1 - alpha_bar)).  Step i from level s to
    level t: h_i = lambda_t - lambda_s, g = alpha_t (1 - exp(-h_i)), c = h_i / (2 h_{i-1}); the solver's
    x' = (sigma_t / sigma_s) x + g ((1 + c) x0_s - c x0_prev) gives A = sigma_t / sigma_s + g (1 + c) / alpha_s,
    E = -g (1 + c) sigma_s / alpha_s, C = -g c.  The first row has no history and the last goes to alpha_bar = 1 (h
    infinite): both are first order, which in this parametrisation is the DDIM update -- their (A, E) are the
    ddim_coefficients rows of the same grid and C = 0."""
    ab = alphas_cumprod(num_train_steps)
    ts = sample_timesteps(num_train_steps, num_sample_steps, spacing).tolist()
    first = ddim_coefficients(num_train_steps, num_sample_steps, spacing)
    lam = log_snr(num_train_steps)
    S = len(ts)
    zero = torch.tensor(0.0, dtype=torch.float64)
    rows = []
    for i, s in enumerate(ts):
        al_s, sg_s = torch.sqrt(ab[s]), torch.sqrt(1 - ab[s])
        hx, he = 1.0 / al_s, -sg_s / al_s
        if i == 0 or i == S - 1:
            A, E, C = first[i, 0], first[i, 1], zero
        else:
            t = ts[i + 1]
            al_t, sg_t = torch.sqrt(ab[t]), torch.sqrt(1 - ab[t])
            h = lam[t] - lam[s]
            c = h / (2.0 * (lam[s] - lam[ts[i - 1]]))
            g = -al_t * torch.expm1(-h)
            A = sg_t / sg_s + g * (1 + c) / al_s
            E = -g * (1 + c) * sg_s / al_s
            C = -g * c
        rows.append(torch.stack([A, E, C, hx, he]))
    return torch.stack(rows)


def _sde_steps(num_train_steps: int, num_sample_steps: int, spacing: str):
    """per sampling step but the last: (alpha_s, sigma_s, alpha_t, sigma_t, h, c) of the step from level s = t_i to
    t = t_{i+1} in float64 -- h = lambda_t - lambda_s, c = h / (2 (lambda_s - lambda_{t_{i-1}})), 0 in the first row.  The last
    step (to alpha_bar = 1, h infinite) comes as (alpha_s, sigma_s) alone"""
    ab = alphas_cumprod(num_train_steps)
    ts = sample_timesteps(num_train_steps, num_sample_steps, spacing).tolist()
    lam = log_snr(num_train_steps)
    out = []
    for i, s in enumerate(ts):
        al_s, sg_s = torch.sqrt(ab[s]), torch.sqrt(1 - ab[s])
        if i == len(ts) - 1:
            out.append((al_s, sg_s))
            continue
        t = ts[i + 1]
        h = lam[t] - lam[s]
        c = h / (2.0 * (lam[s] - lam[ts[i - 1]])) if i > 0 else torch.tensor(0.0, dtype=torch.float64)
        out.append((al_s, sg_s, torch.sqrt(ab[t]), torch.sqrt(1 - ab[t]), h, c))
    return out


def sde_dpmpp_coefficients(num_train_steps: int = 1000, num_sample_steps: int = 100, eta: float = 0.0,
                           spacing: str = "time") -> torch.Tensor:
    """[S, 6] float64 (A, E, C, hx, he, G) of SDE-DPM-Solver++(2M) (Lu et al. 2022; k-diffusion's dpmpp_2m_sde), the
    stochastic form of dpmpp_coefficients: x' = A x + E eps + C h_prev + G z', z' ~ N(0, I), with the same history
    h = hx x + he eps.  Step i from level s to level t, h_i = lambda_t - lambda_s, c = h_i / (2 h_{i-1}) (0 in the first
    row), g = -alpha_t expm1(-(1 + eta) h_i):
      A = (sigma_t / sigma_s) exp(-eta h_i) + g (1 + c) / alpha_s,  E = -g (1 + c) sigma_s / alpha_s,  C = -g c,
      G = sigma_t sqrt(-expm1(-2 eta h_i)).
    The last row goes to alpha_bar = 1: (1 / alpha_s, -sigma_s / alpha_s, 0, hx, he, 0), the last row of ddim_coefficients.
    At eta = 0 the rows are dpmpp_coefficients' bit for bit (they are returned, not recomputed) and G = 0; at eta = 1 the
    first row's (A, E, G) is the DDPM row of ddim_coefficients_eta.  It belongs on the 'logsnr' grid: uniform in t its steps
    in lambda are very uneven and 20 of them are poor (docs/EXPERIMENTS.md)."""
    if not 0.0 <= float(eta) <= 1.0:
        raise ValueError(f"eta must be in [0, 1], got {eta}")
    eta = float(eta)
    if eta == 0.0:
        five = dpmpp_coefficients(num_train_steps, num_sample_steps, spacing)
        return torch.cat([five, torch.zeros((five.shape[0], 1), dtype=torch.float64)], dim=1)
    zero = torch.tensor(0.0, dtype=torch.float64)
    rows = []
    for st in _sde_steps(num_train_steps, num_sample_steps, spacing):
        al_s, sg_s = st[0], st[1]
        hx, he = 1.0 / al_s, -sg_s / al_s
        if len(st) == 2:
            rows.append(torch.stack([hx, he, zero, hx, he, zero]))
            continue
        _, _, al_t, sg_t, h, c = st
        g = -al_t * torch.expm1(-(1.0 + eta) * h)
        A = (sg_t / sg_s) * torch.exp(-eta * h) + g * (1 + c) / al_s
        E = -g * (1 + c) * sg_s / al_s
        C = -g * c
        G = sg_t * torch.sqrt(-torch.expm1(-2.0 * eta * h))
        rows.append(torch.stack([A, E, C, hx, he, G]))
    return torch.stack(rows)


def sde_observation_noise_coefficients(num_train_steps: int = 1000, num_sample_steps: int = 100, eta: float = 0.0,
                                       spacing: str = "time") -> torch.Tensor:
    """[S, 2] float64 (r, q) of the masked 'dpmpp2m_sde' loop: an observed element keeps x = sqrt(ab) x0 + sqrt(1 - ab) e and
    its stored noise becomes e' = r e + q z' with r = exp(-eta h), q = sqrt(-expm1(-2 eta h)), r^2 + q^2 = 1 (the true x0 as
    the data prediction makes the solver's second-order term vanish, which leaves the first-order SDE step).  (0, 0) in the
    last row, where the level is the observation itself.  At eta = 1 it is observation_noise_coefficients(eta = 1); at
    eta < 1 the two differ, so a loop reads only its own solver's table."""
    if not 0.0 <= float(eta) <= 1.0:
        raise ValueError(f"eta must be in [0, 1], got {eta}")
    eta = float(eta)
    rows = []
    for st in _sde_steps(num_train_steps, num_sample_steps, spacing):
        if len(st) == 2:
            rows.append(torch.zeros(2, dtype=torch.float64))
        else:
            h = st[4]
            rows.append(torch.stack([torch.exp(-eta * h), torch.sqrt(-torch.expm1(-2.0 * eta * h))]))
    return torch.stack(rows)


def check_resample(resample, num_sample_steps: int):
    """the refusals of a `resample = (jump, times)` setting for a loop of S steps -> (jump, times), or None where the loop is
    the plain one: resample None, or times == 1 (every jump point is left backwards times - 1 = 0 times)"""
    if resample is None:
        return None
    try:
        jump, times = resample
        ok = int(jump) == jump and int(times) == times
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"resample must be None or (jump, times), two integers, got {resample!r}")
    jump, times, S = int(jump), int(times), int(num_sample_steps)
    if not 1 <= jump <= S - 1:
        raise ValueError(f"resample: jump = {jump} must be in 1 .. S - 1 = {S - 1} (a jump goes back `jump` of the loop's "
                         f"{S} steps and must land on a position >= 1)")
    if times < 1:
        raise ValueError(f"resample: times = {times} must be at least 1 (1: the plain loop)")
    return None if times == 1 else (jump, times)


def resample_walk(num_sample_steps: int, jump: int, times: int):
    """The operations of one resampled sampling call (RePaint, Lugmayr et al. 2022, Algorithm 1 and its get_schedule_jump,
    restated on POSITIONS): the loop's position p in 0 .. S is the noise level of the state, p < S at alpha_bar[t_p] and S at
    alpha_bar = 1; ('step', p) is update row p and moves p -> p + 1, ('jump', p, visit) diffuses the state back from p to
    p - jump, visit = 0, 1, 2, ... the ordinal of the jump within the call.  Jump points are p = S - m jump, m = 0, 1, ...
    while p - jump > 0; on arriving at one the walk leaves it backwards, times - 1 times in total (the counters are not
    refilled when a later jump passes them again).  Evaluations: S + (ceil(S / jump) - 1) (times - 1) jump.  times == 1 is
    the plain loop."""
    S = int(num_sample_steps)
    if check_resample((jump, times), S) is None:
        return [("step", p) for p in range(S)]
    jump, times = int(jump), int(times)
    left = {}
    p = S
    while p - jump > 0:
        left[p] = times - 1
        p -= jump
    ops, p, visit = [], 0, 0
    while p < S:
        ops.append(("step", p))
        p += 1
        if left.get(p, 0) > 0:
            left[p] -= 1
            ops.append(("jump", p, visit))
            visit += 1
            p -= jump
    return ops


def resample_evaluations(num_sample_steps: int, jump: int, times: int) -> int:
    """denoiser evaluations of resample_walk(S, jump, times)"""
    S, jump, times = int(num_sample_steps), int(jump), int(times)
    return S + (-(-S // jump) - 1) * (times - 1) * jump


def resample_coefficients(num_train_steps: int = 1000, num_sample_steps: int = 100, jump: int = 1,
                          spacing: str = "time") -> torch.Tensor:
    """[S + 1, 2] float64 (c_x, c_z) of a resampling jump, indexed by the position p the state is at: the forward diffusion
    from level L[p] back to L[p - jump], x <- sqrt(rho) x + sqrt(1 - rho) z' with rho = L[p - jump] / L[p], L[p] =
    alpha_bar[t_p] for p < S and L[S] = 1.  Rows p < jump are (0, 0) and never read."""
    ab = alphas_cumprod(num_train_steps)
    ts = sample_timesteps(num_train_steps, num_sample_steps, spacing).tolist()
    S, jump = len(ts), int(jump)
    if not 1 <= jump <= S - 1:
        raise ValueError(f"jump = {jump} must be in 1 .. S - 1 = {S - 1}")
    L = [ab[t] for t in ts] + [torch.tensor(1.0, dtype=torch.float64)]
    out = torch.zeros((S + 1, 2), dtype=torch.float64)
    for p in range(jump, S + 1):
        rho = L[p - jump] / L[p]
        out[p, 0], out[p, 1] = torch.sqrt(rho), torch.sqrt(1 - rho)
    return out


CLIP_MODES = ("range", "dynamic")


def x0_coefficients(num_train_steps: int = 1000, num_sample_steps: int = 100, spacing: str = "time") -> torch.Tensor:
    """[S, 4] float64 (ia, sa, a, is) of the x0 clip (csrc/clip.hip), row s at the level of sampling timestep t_s:
    ia = 1 / sqrt(ab), sa = sqrt(1 - ab) / sqrt(ab), a = sqrt(ab), is = 1 / sqrt(1 - ab).  The data prediction of a step is
    x0 = ia x - sa eps, and the noise prediction that reconstructs a clipped x0c is (x - a x0c) is."""
    ab = alphas_cumprod(num_train_steps)
    ts = sample_timesteps(num_train_steps, num_sample_steps, spacing)
    a = torch.sqrt(ab[ts])
    s = torch.sqrt(1.0 - ab[ts])
    return torch.stack([1.0 / a, s / a, a, 1.0 / s], dim=1)


def clip_tables(lo, hi):
    """the per-column tables of the x0 clip from bounds lo[D] <= hi[D] -> (m, h, ih, bounded), float64 [D] and bool [D]:
    the centre (lo + hi) / 2, the half width (hi - lo) / 2 and its reciprocal.  A column is bounded iff both bounds are finite
    and hi > lo; any other column is never counted and never changed (+-inf is the way to say 'no bound'), and its m, h, ih
    are never read.  A NaN bound, lo > hi or lengths that differ are a ValueError."""
    lo = torch.as_tensor(lo, dtype=torch.float64).reshape(-1)
    hi = torch.as_tensor(hi, dtype=torch.float64).reshape(-1)
    if lo.numel() != hi.numel() or lo.numel() == 0:
        raise ValueError(f"clip bounds: lo and hi must have one value per column each, got {lo.numel()} and {hi.numel()}")
    if bool(torch.isnan(lo).any()) or bool(torch.isnan(hi).any()):
        raise ValueError("clip bounds: NaN is no bound (use -inf / +inf for 'no bound')")
    if bool((lo > hi).any()):
        c = int(torch.nonzero(lo > hi)[0])
        raise ValueError(f"clip bounds: lo > hi in column {c} ({float(lo[c])} > {float(hi[c])})")
    bounded = torch.isfinite(lo) & torch.isfinite(hi) & (hi > lo)
    safe_lo, safe_hi = torch.where(bounded, lo, torch.zeros_like(lo)), torch.where(bounded, hi, torch.ones_like(hi))
    m, h = (safe_lo + safe_hi) / 2.0, (safe_hi - safe_lo) / 2.0
    return m, h, 1.0 / h, bounded


def clip_rank(p: float, n: int) -> int:
    """the nearest-rank position of the quantile p in (0, 1] among n values: k = min(n, max(1, ceil(p n))), 1-based"""
    p, n = float(p), int(n)
    if not 0.0 < p <= 1.0:
        raise ValueError(f"the clip quantile must be in (0, 1], got {p}")
    if n < 1:
        raise ValueError(f"clip_rank: n = {n} values have no order statistic")
    return min(n, max(1, math.ceil(p * n)))


STITCH_KMAX = 8                 # IB_STITCH_KMAX (include/ib_hip_stitch.h): the most windows that may cover one trial frame
STITCH_BLENDS = ("uniform", "ramp")


def stitch_layout(F: int, T: int, hop: int, blend: str = "ramp"):
    """The layout of a trial of F frames denoised as overlapping windows of T frames (sampler.StitchedDDIMSampler, the tables
    of ib_stitch_ddim_step) -> (start, cover, wn, KMAX):
      start int32 [W]       window starts 0, hop, 2 hop, ... while start + T <= F, plus a last window at F - T when the grid
                            does not land there: every frame is covered, the starts strictly increase
      cover int32 [F, 2]    per trial frame the first covering window and how many cover it (they are consecutive)
      wn    fp32  [F, KMAX] the blend weights of the covering windows in window order, normalised per frame in float64 to sum
                            to 1 and cast once; slots beyond the count are 0
    blend 'uniform': equal weights.  'ramp': the raw weight of in-window frame t is min(t + 1, T - t, R) / R with
    R = max(T - hop, 1), a trapezoid, so a window fades in and out over its overlap."""
    F, T, hop = int(F), int(T), int(hop)
    if T < 1 or F < T:
        raise ValueError(f"F = {F} must be at least the window T = {T}: a trial shorter than a window cannot be stitched")
    if hop < 1 or hop > T:
        raise ValueError(f"hop = {hop} must be in 1 .. T = {T} (a larger hop leaves frames uncovered)")
    if blend not in STITCH_BLENDS:
        raise ValueError(f"blend must be one of {STITCH_BLENDS}, got {blend!r}")
    starts = list(range(0, F - T + 1, hop))
    if starts[-1] != F - T:
        starts.append(F - T)
    R = max(T - hop, 1)
    start = torch.tensor(starts, dtype=torch.int32)
    cover = torch.zeros((F, 2), dtype=torch.int32)
    w64 = torch.zeros((F, STITCH_KMAX), dtype=torch.float64)
    for f in range(F):
        ws = [w for w, s0 in enumerate(starts) if s0 <= f < s0 + T]
        if len(ws) > STITCH_KMAX:
            raise ValueError(f"hop = {hop} is too small for T = {T}: frame {f} is covered by {len(ws)} windows, more than "
                             f"{STITCH_KMAX}")
        cover[f, 0], cover[f, 1] = ws[0], len(ws)
        for k, w in enumerate(ws):
            t = f - starts[w]
            w64[f, k] = 1.0 if blend == "uniform" else min(t + 1, T - t, R) / R
    wn = (w64 / w64.sum(dim=1, keepdim=True)).to(torch.float32)
    return start, cover, wn, STITCH_KMAX


def timestep_embedding_table(num_steps: int, dim: int, max_period: float = 10000.0) -> torch.Tensor:
    """[num_steps, dim] float64: row t = [sin(t w), cos(t w)]."""
    half = dim // 2
    w = torch.exp(-math.log(max_period) * torch.arange(half, dtype=torch.float64) / half)
    a = torch.arange(num_steps, dtype=torch.float64).reshape(-1, 1) * w.reshape(1, -1)
    return torch.cat([torch.sin(a), torch.cos(a)], dim=-1)


class DiffusionTables:
    """fp32 device copies of the float64 tables (cast once)."""

    def __init__(self, device, num_train_steps: int = 1000, num_sample_steps: int = 100, temb_dim: int = 128):
        ab = alphas_cumprod(num_train_steps)
        self.num_train_steps, self.num_sample_steps, self.temb_dim = num_train_steps, num_sample_steps, temb_dim
        self.alphas_cumprod64 = ab
        self.sqrt_ab = torch.sqrt(ab).to(torch.float32).to(device)
        self.sqrt_1mab = torch.sqrt(1.0 - ab).to(torch.float32).to(device)
        self._inv_sqrt_1mab = None
        self.temb = timestep_embedding_table(num_train_steps, temb_dim).to(torch.float32).to(device).contiguous()
        self.observations = "noised"
        self.set_sampler(num_sample_steps)
        self.device = device

    @property
    def inv_sqrt_1mab(self):
        """1 / sqrt(1 - ab) in float64, cast once: what hip.pred_to_eps multiplies by under x0-prediction.  Made when first
        asked for, so an eps model allocates nothing"""
        if self._inv_sqrt_1mab is None:
            self._inv_sqrt_1mab = (1.0 / torch.sqrt(1.0 - self.alphas_cumprod64)).to(torch.float32).to(self.sqrt_ab.device)
        return self._inv_sqrt_1mab

    def set_sampler(self, num_sample_steps: int, eta: float = 0.0, solver: str = "ddim", spacing: str = "time",
                    observations: str = "noised"):
        """the sampler's tables for S steps on the `spacing` grid; eta > 0 adds the stochastic loop's (c_x, c_eps, sigma) and
        (r, q) tables -- with solver 'dpmpp2m_sde' that solver's own (sde_coef [S, 6], sde_obs_noise_coef) instead --, solver
        'dpmpp2m' or 'dpmpp2m_sde' the second-order multistep solver's (A, E, C, hx, he) table.  observations: what
        obs_coef holds -- 'noised', the observation forward-noised to each level (observation_coefficients), or 'clean',
        every row (1, 0) (clean_observation_coefficients: a denoiser trained on clean conditioning columns)"""
        check_sampler_settings(eta, solver, spacing, observations)
        N = self.num_train_steps
        dev = self.sqrt_ab.device
        ddim_t = sample_timesteps(N, num_sample_steps, spacing).to(dev)          # raises before anything is replaced
        self.num_sample_steps, self.eta, self.solver, self.spacing = num_sample_steps, float(eta), solver, spacing
        self.ddim_t = ddim_t
        self.ddim_coef = ddim_coefficients(N, num_sample_steps, spacing).to(torch.float32).to(dev).contiguous()
        self.observations = observations
        obs = clean_observation_coefficients if observations == "clean" else observation_coefficients
        self.obs_coef = obs(N, num_sample_steps, spacing).to(torch.float32).to(dev).contiguous()
        self.ddim_coef_eta = self.obs_noise_coef = self.dpmpp_coef = self.sde_coef = self.sde_obs_noise_coef = None
        self.resample_jump, self.resample_coef = 0, None         # a new grid drops the jump table: set_resample makes it
        up = lambda t: t.to(torch.float32).to(dev).contiguous()
        # an eta > 0 loop gets the stochastic tables of ITS solver and not the other's: the two (r, q) tables differ at
        # eta < 1, and serves() refuses a loop whose own tables are missing
        if self.eta > 0.0 and solver == "dpmpp2m_sde":
            self.sde_coef = up(sde_dpmpp_coefficients(N, num_sample_steps, eta, spacing))
            self.sde_obs_noise_coef = up(sde_observation_noise_coefficients(N, num_sample_steps, eta, spacing))
        elif self.eta > 0.0:
            self.ddim_coef_eta = up(ddim_coefficients_eta(N, num_sample_steps, eta, spacing))
            self.obs_noise_coef = up(observation_noise_coefficients(N, num_sample_steps, eta, spacing))
        if solver in ("dpmpp2m", "dpmpp2m_sde"):                 # 'dpmpp2m_sde' at eta = 0 runs the 'dpmpp2m' launches
            self.dpmpp_coef = up(dpmpp_coefficients(N, num_sample_steps, spacing))

    def set_resample(self, jump: int):
        """the jump table of a resampled loop on the current grid, resample_coef [S + 1, 2] (resample_coefficients), cast once;
        jump = 0 drops it.  No other table is touched, so a captured step that bakes their pointers in stays valid: the jump
        launch is issued between the replays and is handed this table at every call"""
        jump = int(jump)
        if jump == 0:
            self.resample_jump, self.resample_coef = 0, None
            return
        coef = resample_coefficients(self.num_train_steps, self.num_sample_steps, jump, self.spacing)   # raises first
        self.resample_jump = jump
        self.resample_coef = coef.to(torch.float32).to(self.sqrt_ab.device).contiguous()

    clip = None                              # the x0 clip's tables (set_clip), None until a clipped loop asks for them

    def set_clip(self, lo, hi):
        """the tables of the x0 clip on the current grid (csrc/clip.hip), each computed in float64 and cast once: `clip` =
        {'coef': x0_coefficients [S, 4], 'lo', 'hi', 'm', 'h', 'ih': fp32 [D] on the device, 'bounded': bool [D] on the host,
        decided on the CAST bounds, which are what the kernels test, 'key': what clip_serves compares}.  lo = hi = None drops
        them.  No other table is touched: set_sampler and what it makes stay as they are, and a new grid is noticed by
        clip_serves, not here."""
        if lo is None and hi is None:
            self.clip = None
            return
        m, h, ih, _ = clip_tables(lo, hi)                                  # raises before anything is replaced
        lo64 = torch.as_tensor(lo, dtype=torch.float64).reshape(-1)
        hi64 = torch.as_tensor(hi, dtype=torch.float64).reshape(-1)
        coef = x0_coefficients(self.num_train_steps, self.num_sample_steps, self.spacing)
        dev = self.sqrt_ab.device
        up = lambda t: t.to(torch.float32).to(dev).contiguous()
        lo32, hi32 = lo64.to(torch.float32), hi64.to(torch.float32)
        self.clip = {"coef": up(coef), "lo": up(lo64), "hi": up(hi64), "m": up(m), "h": up(h), "ih": up(ih),
                     "bounded": torch.isfinite(lo32) & torch.isfinite(hi32) & (hi32 > lo32),
                     "key": (self.num_sample_steps, self.spacing, tuple(lo64.tolist()), tuple(hi64.tolist()))}

    def clip_serves(self, num_sample_steps: int, spacing: str, lo, hi) -> bool:
        """whether `clip` holds the tables of these bounds (tuples of floats) on this grid"""
        return self.clip is not None and self.clip["key"] == (num_sample_steps, spacing, tuple(lo), tuple(hi))

    def serves(self, num_sample_steps: int, eta: float = 0.0, solver: str = "ddim", spacing: str = "time",
               observations: Optional[str] = None, resample_jump: int = 0) -> bool:
        """whether the current tables are the ones a loop with these settings reads: the grid (S, spacing) must match; the
        eta tables only matter to an eta > 0 loop -- and then they must be those of the loop's own solver, first-order
        ('ddim') or 'dpmpp2m_sde' --, the second-order table only to 'dpmpp2m' and 'dpmpp2m_sde' and the observation table only
        to a masked loop, which names the kind it reads (None: the loop reads no observation table), the jump table only to
        a resampled loop, which names its jump (0: the loop reads no jump table)"""
        noisy = float(eta) > 0.0
        return (self.num_sample_steps == num_sample_steps and self.spacing == spacing
                and (observations is None or self.observations == observations)
                and (not resample_jump or (self.resample_jump == int(resample_jump) and self.resample_coef is not None))
                and (not noisy or self.eta == float(eta))
                and (not (noisy and solver == "ddim") or self.ddim_coef_eta is not None)
                and (not (noisy and solver == "dpmpp2m_sde") or self.sde_coef is not None)
                and (solver not in ("dpmpp2m", "dpmpp2m_sde") or self.dpmpp_coef is not None))

    def host_tables(self) -> Dict[str, torch.Tensor]:
        return {"sqrt_ab": self.sqrt_ab.cpu(), "sqrt_1mab": self.sqrt_1mab.cpu(), "temb": self.temb.cpu(),
                "ddim_t": self.ddim_t.cpu(), "ddim_coef": self.ddim_coef.cpu()}
