"""The stochastic sampler update on the GPU (eta > 0): ib_ddim_step_noise / ib_ddim_cond_step_noise against a float64
restatement fed the oracle's Philox words (oracle/ref_cpu.py::draw_words, Box-Muller in float64), the bitwise relations to
the deterministic entries and across batch position / pitch, the statistics of a whole loop against the exact variance
recursion of Gaussian data, and ib_ensemble_stats against float64.  -m gpu."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
DOMAIN_STEP = 2                  # csrc/philox.h: 0 = eps / start draw, 1 = timesteps, 2 = the noise of a sampling step
GEN_TOL = 2e-5                   # tests/test_noise_gpu.py: hardware log2 / sin / cos against float64, absolute
ARITH = {torch.float32: 2e-6, BF: 8e-3}      # tests/test_cond_sampler_gpu.py: the eta = 0 kernel test's bound, x max |want|


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from inferbiomechanics_amd import hip
    hip.lib()


def ref_normals(T, D, seed, s, wid):
    """float64 [T, D]: element (f, d) from block (f D + d) / 4 of counter (block, s, wid, 2), as philox_normals pairs words"""
    n = T * D
    nb = (n + 3) // 4
    w = (R.draw_words(nb, seed, s, wid, DOMAIN_STEP) >> np.uint32(8)).astype(np.float64)
    out = np.empty((nb, 4), dtype=np.float64)
    for a in (0, 2):
        r = np.sqrt(-2.0 * np.log((w[:, a] + 1.0) * 2.0 ** -24))
        th = 2.0 * np.pi * (w[:, a + 1] * 2.0 ** -24)
        out[:, a], out[:, a + 1] = r * np.cos(th), r * np.sin(th)
    return torch.from_numpy(out.reshape(-1)[:n].reshape(T, D).copy())


def guarded(B, T, ld, D, dt, g, fill=True):
    """a [B, T, ld] view (pad columns 0) in front of 64 sentinel elements no kernel may touch"""
    flat = torch.full((B * T * ld + 64,), 7.0, dtype=dt)
    v = flat[:B * T * ld].view(B, T, ld)
    v.zero_()
    if fill:
        v[:, :, :D] = torch.randn(B, T, D, generator=g).to(dt)
    flat = flat.to(DEV)
    return flat, flat[:B * T * ld].view(B, T, ld)


def tables(S, eta):
    from inferbiomechanics_amd.diffusion.schedule import DiffusionTables
    tabs = DiffusionTables(torch.device(DEV), num_sample_steps=S)
    tabs.set_sampler(S, eta)
    return tabs


SHAPES = [(torch.float32, 3, 10, 177, 177),      # element-wise kernel (T * ld % 8 != 0)
          (torch.float32, 4, 10, 177, 177),      # element-wise, with the rounding of ib_ddim_step's 8-wide kernel
          (torch.float32, 3, 24, 44, 44),        # 8-wide, unpitched, whole blocks
          (torch.float32, 3, 24, 44, 48),        # 8-wide, pitched, whole blocks
          (BF, 3, 10, 177, 192),                 # 8-wide, pitched, D % 4 != 0: blocks looked up per element
          (BF, 2, 10, 300, 320)]                 # the benched row: 8-wide, pitched, two whole blocks per vector


def masks(T, D, ld, g):
    empty = torch.zeros(T, ld, dtype=torch.uint8)
    full = empty.clone()
    full[:, :D] = 1
    label = full.clone()
    label[:, D - 30:D] = 0
    mixed = label.clone()
    mixed[:, 8:D - 30] = (torch.rand(T, D - 38, generator=g) < 0.5).to(torch.uint8) * 3
    return {"empty": empty, "full": full, "label": label, "mixed": mixed}


@pytest.mark.parametrize("dt,B,T,D,ld", SHAPES)
def test_step_noise_against_float64(dt, B, T, D, ld):
    from inferbiomechanics_amd import hip
    S, eta, seed = 10, 0.7, 0x1234_5678_9ABC_DEF0
    g = torch.Generator().manual_seed(17 * B + D + ld)
    tabs = tables(S, eta)
    c3 = tabs.ddim_coef_eta.cpu().double()
    ids = torch.tensor([5, 2 ** 32 - 1, 0, 77][:B], dtype=torch.int64)
    win = ids.to(DEV)
    xf, x = guarded(B, T, ld, D, dt, g)
    _, eps = guarded(B, T, ld, D, dt, g)
    X, E = x.cpu().double(), eps.cpu().double()
    for s in (0, S // 2, S - 1):
        ctr = torch.tensor([s], dtype=torch.int32, device=DEV)
        t_out = torch.full((B,), -7, dtype=torch.int64, device=DEV)
        xs_f = xf.clone()
        xs = xs_f[:B * T * ld].view(B, T, ld)
        hip.ddim_step_noise(xs, eps, tabs.ddim_coef_eta, tabs.ddim_t, win, seed, step_dev=ctr, t_out=t_out, D=D)
        xh = x.clone()
        hip.ddim_step_noise(xh, eps, tabs.ddim_coef_eta, tabs.ddim_t, win, seed, step=s, D=D)
        torch.cuda.synchronize()
        Z = torch.zeros(B, T, ld, dtype=torch.float64)
        for b in range(B):
            Z[b, :, :D] = ref_normals(T, D, seed, s, int(ids[b]))
        sg = float(c3[s, 2])
        assert (sg == 0.0) == (s == S - 1)
        want = c3[s, 0] * X + c3[s, 1] * E + sg * Z
        err = (xs.cpu().double() - want).abs()
        tol = abs(sg) * GEN_TOL + ARITH[dt] * float(want.abs().max())
        print(f"step_noise {dt} B={B} D={D} ld={ld} s={s}: max err {float(err.max()):.3e} (tol {tol:.3e})")
        assert float(err.max()) <= tol, (s, float(err.max()), tol)
        assert not xs[:, :, D:].any(), "pad columns must stay 0"
        assert bool((xs_f[B * T * ld:] == 7.0).all()), "wrote past the state"
        assert torch.equal(xh, xs), "host step index and device step counter disagree"
        assert int(t_out[0]) == (int(tabs.ddim_t[s + 1]) if s + 1 < S else 0) and int(ctr) == s


@pytest.mark.parametrize("dt,B,T,D,ld", SHAPES)
def test_cond_step_noise_against_float64(dt, B, T, D, ld):
    from inferbiomechanics_amd import hip
    S, eta, seed = 10, 1.0, 99
    g = torch.Generator().manual_seed(31 * B + D + ld)
    tabs = tables(S, eta)
    c3, oc, on = (t.cpu().double() for t in (tabs.ddim_coef_eta, tabs.obs_coef, tabs.obs_noise_coef))
    ids = torch.tensor([9, 4, 2 ** 31, 1][:B], dtype=torch.int64)
    win = ids.to(DEV)
    _, x = guarded(B, T, ld, D, dt, g)
    _, eps = guarded(B, T, ld, D, dt, g)
    _, x0 = guarded(B, T, ld, D, dt, g)
    zf, z = guarded(B, T, ld, D, dt, g)
    X, E, X0, Z0 = (t.cpu().double() for t in (x, eps, x0, z))
    for name, m in masks(T, D, ld, g).items():
        mb, md = m.bool(), m.to(DEV)
        for s in (0, S // 2, S - 1):
            ctr = torch.tensor([s], dtype=torch.int32, device=DEV)
            xs, zs_f = x.clone(), zf.clone()
            zs = zs_f[:B * T * ld].view(B, T, ld)
            hip.ddim_cond_step_noise(xs, eps, x0, zs, md, tabs.ddim_coef_eta, tabs.obs_coef, tabs.obs_noise_coef, tabs.ddim_t,
                                     win, seed, step_dev=ctr, D=D)
            torch.cuda.synchronize()
            N = torch.zeros(B, T, ld, dtype=torch.float64)
            for b in range(B):
                N[b, :, :D] = ref_normals(T, D, seed, s, int(ids[b]))
            sg, r, q = float(c3[s, 2]), float(on[s, 0]), float(on[s, 1])
            free = ~mb
            if sg == 0.0:                          # the last row: the deterministic step, z left alone
                assert torch.equal(zs, z)
                e_new = Z0
            else:
                e_want = r * Z0 + q * N
                got_e = zs.cpu().double()
                tol_e = abs(q) * GEN_TOL + ARITH[dt] * float(e_want.abs().max())
                assert float((got_e - e_want)[:, mb].abs().max() if mb.any() else 0.0) <= tol_e, (name, s)
                assert torch.equal(zs[:, free.to(DEV)], z[:, free.to(DEV)]), "free elements must not touch z"
                e_new = got_e                       # the pinned value is formed from the STORED noise
            want = torch.where(mb, oc[s + 1, 0] * X0 + oc[s + 1, 1] * e_new, c3[s, 0] * X + c3[s, 1] * E + sg * N)
            err = (xs.cpu().double() - want).abs()
            tol = abs(sg) * GEN_TOL + ARITH[dt] * float(want.abs().max())
            print(f"cond_step_noise {dt} B={B} D={D} ld={ld} {name} s={s}: max err {float(err.max()):.3e} (tol {tol:.3e})")
            assert float(err.max()) <= tol, (name, s, float(err.max()), tol)
            assert not xs[:, :, D:].any() and not zs[:, :, D:].any(), "pad columns must stay 0"
            assert bool((zs_f[B * T * ld:] == 7.0).all()), "wrote past the noise buffer"
            if s == S - 1:
                obs = mb.to(DEV)
                assert torch.equal(xs[:, obs], x0[:, obs]), "the last step must land on the observation"


@pytest.mark.parametrize("dt,B,T,D,ld", SHAPES)
def test_sigma_zero_rows_equal_the_deterministic_entries(dt, B, T, D, ld):
    """every row of an eta = 0 table and the last row of an eta = 1 table, through the new entries"""
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion import schedule as sch
    S = 10
    g = torch.Generator().manual_seed(5 * B + D + ld)
    tabs = tables(S, 1.0)
    zero3 = sch.ddim_coefficients_eta(1000, S, 0.0).to(torch.float32).to(DEV).contiguous()
    one0 = sch.observation_noise_coefficients(1000, S, 0.0).to(torch.float32).to(DEV).contiguous()
    assert torch.equal(zero3[:, :2], tabs.ddim_coef) and not zero3[:, 2].any()
    win = torch.arange(B, dtype=torch.int64, device=DEV)
    _, x = guarded(B, T, ld, D, dt, g)
    _, eps = guarded(B, T, ld, D, dt, g)
    _, x0 = guarded(B, T, ld, D, dt, g)
    _, z = guarded(B, T, ld, D, dt, g)
    for name, m in masks(T, D, ld, g).items():
        md = m.to(DEV)
        for c3, on, steps in ((zero3, one0, (0, S // 2, S - 1)), (tabs.ddim_coef_eta, tabs.obs_noise_coef, (S - 1,))):
            for s in steps:
                a, b = x.clone(), x.clone()
                hip.ddim_step(a, eps, tabs.ddim_coef, tabs.ddim_t, step=s)
                hip.ddim_step_noise(b, eps, c3, tabs.ddim_t, win, 3, step=s, D=D)
                assert torch.equal(a, b), ("ib_ddim_step", s)
                a, b, zz = x.clone(), x.clone(), z.clone()
                hip.ddim_cond_step(a, eps, x0, z, md, tabs.ddim_coef, tabs.obs_coef, tabs.ddim_t, step=s, D=D)
                hip.ddim_cond_step_noise(b, eps, x0, zz, md, c3, tabs.obs_coef, on, tabs.ddim_t, win, 3, step=s, D=D)
                assert torch.equal(a, b) and torch.equal(zz, z), ("ib_ddim_cond_step", name, s)


@pytest.mark.parametrize("dt,T,D,ld", [(torch.float32, 24, 44, 44), (torch.float32, 24, 44, 48), (BF, 10, 300, 320)])
def test_draw_depends_on_seed_window_and_step_only(dt, T, D, ld):
    from inferbiomechanics_amd import hip
    S, seed = 10, 2024
    tabs = tables(S, 1.0)
    g = torch.Generator().manual_seed(3)
    row = torch.zeros(1, T, ld)
    row[:, :, :D] = torch.randn(1, T, D, generator=g)
    erow = torch.zeros(1, T, ld)
    erow[:, :, :D] = torch.randn(1, T, D, generator=g)
    other = torch.zeros(16, T, ld)
    other[:, :, :D] = torch.randn(16, T, D, generator=g)

    def run(B, pos, wid, s, seed=seed, cond=False):
        x, eps = other[:B].clone(), other[:B].flip(0).clone()
        x[pos], eps[pos] = row[0], erow[0]
        x, eps = x.to(dt).to(DEV), eps.to(dt).to(DEV)
        win = torch.arange(100, 100 + B, dtype=torch.int64)
        win[pos] = wid
        if cond:
            m = torch.zeros(T, ld, dtype=torch.uint8)
            m[:, :D - 30] = 1
            z = x.clone()
            hip.ddim_cond_step_noise(x, eps, eps.clone(), z, m.to(DEV), tabs.ddim_coef_eta, tabs.obs_coef, tabs.obs_noise_coef,
                                     tabs.ddim_t, win.to(DEV), seed, step=s, D=D)
            return torch.cat([x[pos], z[pos]])
        hip.ddim_step_noise(x, eps, tabs.ddim_coef_eta, tabs.ddim_t, win.to(DEV), seed, step=s, D=D)
        return x[pos]

    for cond in (False, True):
        base = run(1, 0, 42, 3, cond=cond)
        assert torch.equal(base, run(16, 7, 42, 3, cond=cond)), "the draw must not depend on the batch position or size"
        assert not torch.equal(base, run(1, 0, 43, 3, cond=cond)), "another window id, the same draw"
        assert not torch.equal(base, run(1, 0, 42, 4, cond=cond)), "another step, the same draw"
        assert not torch.equal(base, run(1, 0, 42, 3, seed=seed + 1, cond=cond)), "another seed, the same draw"


def test_fp32_pitched_and_unpitched_runs_agree():
    from inferbiomechanics_amd import hip
    B, T, D, ld, S = 3, 24, 44, 48, 10
    tabs = tables(S, 0.5)
    g = torch.Generator().manual_seed(8)
    x, eps, x0, z = (torch.randn(B, T, D, generator=g) for _ in range(4))
    win = torch.tensor([3, 1, 4], dtype=torch.int64, device=DEV)
    m = torch.zeros(T, D, dtype=torch.uint8)
    m[:, :D - 30] = 1

    def pitch(t, pld):
        p = torch.zeros(*t.shape[:-1], pld, dtype=t.dtype)
        p[..., :D] = t
        return p.to(DEV)

    outs = []
    for pld in (D, ld):
        a, e, o, n, mk = pitch(x, pld), pitch(eps, pld), pitch(x0, pld), pitch(z, pld), pitch(m, pld)
        u = a.clone()
        hip.ddim_step_noise(u, e, tabs.ddim_coef_eta, tabs.ddim_t, win, 5, step=2, D=D)
        hip.ddim_cond_step_noise(a, e, o, n, mk, tabs.ddim_coef_eta, tabs.obs_coef, tabs.obs_noise_coef, tabs.ddim_t, win, 5,
                                 step=2, D=D)
        outs.append((u[:, :, :D].clone(), a[:, :, :D].clone(), n[:, :, :D].clone()))
    for p, q in zip(*outs):
        assert torch.equal(p, q)


# ---------------------------------------------------------------------------------------------------------------------
# the noise is fresh at every step and has the right scale: a whole loop over Gaussian data
# ---------------------------------------------------------------------------------------------------------------------
def _levels(S):
    ab = R.alphas_cumprod(R.linear_beta_schedule(1000))
    ts = R.ddim_timesteps(1000, S).tolist()
    return [float(ab[t]) for t in ts]


@pytest.mark.parametrize("S,eta", [(100, 0.5), (100, 1.0), (1000, 1.0)])
@pytest.mark.parametrize("s2", [0.25, 4.0])
def test_loop_variance_follows_the_exact_recursion(S, eta, s2):
    """x0 ~ N(0, s2) has the analytic optimal denoiser eps = sqrt(1 - a) x / (a s2 + 1 - a), so every element stays a
    zero-mean Gaussian whose variance obeys v' = (c_x + c_eps sqrt(1 - a) / (a s2 + 1 - a))^2 v + sigma^2 exactly, from v = 1.
    The sample variance over N = 2^22 iid elements has relative standard error sqrt(2 / N); the bound is 5 of them (0.35 %).
    A missing, mis-scaled or step-repeated noise term is percent-level away (the eta = 0 recursion ends at 0.945 / 0.970 of s2,
    these at 0.930 / 0.964, 0.877 / 0.941, 0.985 / 0.994)."""
    from scipy import stats
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion import schedule as sch
    B, T, D = 64, 256, 256
    N = B * T * D
    assert N == 1 << 22
    tabs = tables(S, eta)
    c64 = sch.ddim_coefficients_eta(1000, S, eta)
    lv = _levels(S)
    v = 1.0
    gains = []
    for s in range(S):
        k = (1 - lv[s]) ** 0.5 / (lv[s] * s2 + 1 - lv[s])
        gains.append(k)
        v = (float(c64[s, 0]) + float(c64[s, 1]) * k) ** 2 * v + float(c64[s, 2]) ** 2
    x = torch.randn(B, T, D, generator=torch.Generator(device=DEV).manual_seed(S + int(10 * eta)), device=DEV)
    win = torch.arange(B, dtype=torch.int64, device=DEV)
    ctr = torch.zeros(1, dtype=torch.int32, device=DEV)
    for s in range(S):
        eps = x * gains[s]                       # the test's own denoiser, in torch
        hip.ddim_step_noise(x, eps, tabs.ddim_coef_eta, tabs.ddim_t, win, 77, step_dev=ctr)
        hip.counter_add(ctr, 1)
    got = x.double().cpu().numpy().reshape(-1)
    var = float((got ** 2).mean())
    rel = var / v - 1
    print(f"S={S} eta={eta} s2={s2}: expected variance {v:.6f} ({v / s2:.4f} of s2), sample {var:.6f}, rel {rel:+.3e}, "
          f"bound {5 * (2 / N) ** 0.5:.3e}")
    assert abs(rel) <= 5 * (2 / N) ** 0.5
    assert abs(got.mean()) <= 5 * (v / N) ** 0.5
    assert stats.kstest(got[::16] / v ** 0.5, "norm").pvalue > 1e-3


@pytest.mark.parametrize("dt", [torch.float32, BF])
@pytest.mark.parametrize("eta", [0.5, 1.0])
def test_masked_loop_keeps_unit_noise_and_lands_on_the_observation(dt, eta):
    """Observed elements: e' = r e + q z' with r^2 + q^2 = 1 keeps the stored noise at unit variance, Var e' = r^2 Var e + q^2.
    Sample variance of N iid elements: 5 standard errors, 5 sqrt(2 / N).  bf16 z: every step rounds e' to bf16, relative
    error at most u = 2^-8 (8 significant bits), to nearest so uncorrelated with the value to first order; a step then adds
    at most u^2 Var e' and the deviation d = Var e - 1 obeys d' <= r^2 d + u^2 (1 + d) <= d + u^2 (1 + d): after S steps
    d <= (1 + u^2)^S - 1, 1.5e-3 at S = 100.  The last row is (1, 0): the state ends on the observation."""
    from inferbiomechanics_amd import hip
    S, B, T, D = 100, 16, 256, 256                      # fully observed: N = 2^20 stored noises
    N = B * T * D
    tabs = tables(S, eta)
    g = torch.Generator(device=DEV).manual_seed(4)
    z = torch.randn(B, T, D, generator=g, device=DEV).to(dt)
    x0 = (2 * torch.randn(B, T, D, generator=g, device=DEV)).to(dt)
    x, eps = torch.zeros_like(z), torch.zeros_like(z)
    m = torch.ones(T, D, dtype=torch.uint8, device=DEV)
    win = torch.arange(B, dtype=torch.int64, device=DEV)
    hip.ddim_cond_init(x, x0, z, m, tabs.obs_coef)
    v0 = float((z.double() ** 2).mean())
    ctr = torch.zeros(1, dtype=torch.int32, device=DEV)
    for s in range(S - 1):                              # the last row has sigma = 0 and leaves z alone
        before = z.clone() if s in (0, S // 2) else None
        hip.ddim_cond_step_noise(x, eps, x0, z, m, tabs.ddim_coef_eta, tabs.obs_coef, tabs.obs_noise_coef, tabs.ddim_t, win, 11,
                                 step_dev=ctr)
        hip.counter_add(ctr, 1)
        if before is not None:
            assert not torch.equal(before, z)
    var = float((z.double() ** 2).mean())
    walk = (1 + 2.0 ** -16) ** S - 1 if dt == BF else 0.0
    bound = 5 * (2 / N) ** 0.5 + walk
    print(f"masked loop {dt} eta={eta}: stored noise variance {v0:.6f} -> {var:.6f}, bound |v - 1| <= {bound:.3e}")
    assert abs(var - 1) <= bound
    hip.ddim_cond_step_noise(x, eps, x0, z, m, tabs.ddim_coef_eta, tabs.obs_coef, tabs.obs_noise_coef, tabs.ddim_t, win, 11,
                             step_dev=ctr)
    assert torch.equal(x, x0)


# ---------------------------------------------------------------------------------------------------------------------
# ib_ensemble_stats
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, BF])
@pytest.mark.parametrize("B,K,n", [(3, 4, 300), (2, 1, 77), (1, 16, 1000)])
def test_ensemble_stats_against_float64(dt, B, K, n):
    """mean: the ordered fp32 sum of K terms is within (K - 1) u sum|x| of the exact sum and the division rounds once more:
    |mean - exact| <= u (K sum|x| / K + |mean|) <= (K + 1) u max|x|, u = 2^-24.  std: the K squared deviations carry the
    mean's error and (K + 2) roundings, the division and the square root one each: held to (2 K + 8) u relative to
    max(std, max|x|) (the absolute term covers members that agree to rounding).  K = 1: exactly 0."""
    from inferbiomechanics_amd import hip
    g = torch.Generator().manual_seed(B * K + n)
    x = (3 * torch.randn(B, K, n, generator=g) + 1).to(dt).to(DEV)
    mean, std = hip.ensemble_stats(x)
    torch.cuda.synchronize()
    X = x.cpu().double()
    u = 2.0 ** -24
    amax = float(X.abs().max())
    assert mean.dtype == std.dtype == torch.float32 and mean.shape == std.shape == (B, n)
    assert float((mean.cpu().double() - X.mean(1)).abs().max()) <= (K + 1) * u * amax
    # the ordered fp32 sum itself, bit for bit
    s32 = torch.zeros(B, n)
    for k in range(K):
        s32 = s32 + x[:, k].cpu().float()
    assert torch.equal(mean.cpu(), s32 / K)
    if K == 1:
        assert not std.any()
    else:
        want = X.std(1, unbiased=True)
        assert float((std.cpu().double() - want).abs().max()) <= (2 * K + 8) * u * max(float(want.max()), amax)
    with pytest.raises(hip.HipError):
        hip.ensemble_stats(x[:, :, ::2])
    with pytest.raises(hip.HipError):
        hip.ensemble_stats(x, mean=torch.empty(B, n + 1, device=DEV))
