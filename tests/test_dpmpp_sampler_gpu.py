"""The DPM-Solver++(2M) sampler and the log-SNR grid on the GPU: DDIMSampler / ConditionalDDIMSampler with solver = 'dpmpp2m'
against a float64 loop restated here in the solver's own terms (data predictions, not the coefficient table) over the oracle
denoisers, on both grids; the masked loop's exact relations; the captured step replayed for a second batch; the defaults
bit for bit; and DiffusionLabelPredictor with the new arguments.  -m gpu."""
import math

import pytest
import torch

from oracle import ref_cpu as R
from oracle.fixture_inputs import det_state

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
N = 1000
# tests/test_cond_sampler_gpu.py::test_label_inference_loop_matches_float64 holds the DDIM loop to these, relative to max |want|
BOUND = {torch.float32: 2e-3, BF: 4e-2}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from inferbiomechanics_amd import hip
    hip.lib()


def load_det(module):
    sd = module.state_dict()
    new = det_state({k: tuple(v.shape) for k, v in sd.items()})
    module.load_state_dict({k: v.to(sd[k].dtype) for k, v in new.items()})


def params64(model):
    return {k: v.detach().cpu().double() for k, v in model.state_dict().items()}


def small_models(dt):
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionMLP, DiffusionTransformer
    mlp = DiffusionMLP(44, [64, 64], device=DEV, compute_dtype=dt)
    tr = DiffusionTransformer(44, 24, d_model=128, num_heads=2, dim_feedforward=256, num_layers=2, device=DEV,
                              compute_dtype=dt)
    load_det(mlp)
    load_det(tr)
    return {"mlp": mlp, "transformer": tr}


def eps_fn64(model, kind):
    p = params64(model)
    if kind == "mlp":
        return lambda x, t: R.denoiser_mlp_forward(p, x, t, [64, 64])
    return lambda x, t: R.denoiser_transformer_forward(p, x, t, 2, 2)


def label_mask(T, D, free=30):
    m = torch.ones(T, D, dtype=torch.bool)
    m[:, D - free:] = False
    return m


def grid64(S, spacing):
    """the sampling grid restated: uniform in t, or uniform in lambda = 1/2 log(ab / (1 - ab)) with strict decrease forced
    from the clean end"""
    ab = R.alphas_cumprod(R.linear_beta_schedule(N))
    if spacing == "time":
        return ab, R.ddim_timesteps(N, S).tolist()
    lam = 0.5 * torch.log(ab / (1 - ab))
    near = [int((lam - tg).abs().argmin()) for tg in torch.linspace(float(lam[-1]), float(lam[0]), S, dtype=torch.float64)]
    ts = list(near)
    for i in range(S - 2, -1, -1):
        ts[i] = max(near[i], ts[i + 1] + 1)
    return ab, ts


def loop64(eps_fn, z, S, spacing, solver, x0=None, m=None):
    """float64 restatement of the (masked) loop.  DPM-Solver++(2M), Lu et al. 2022, Algorithm 2: with the data prediction
    d_s = (x - sigma_s eps) / alpha_s, x_t = (sigma_t / sigma_s) x - alpha_t (exp(-h) - 1) D, D = d_s in the first step and
    (1 + 1 / (2 r)) d_s - d_prev / (2 r), r = h_prev / h, afterwards; the last step goes to alpha_bar = 1, first order: x = d_s.
    DDIM is D = d_s in every step.  Observed elements (m) sit on sqrt(ab) x0 + sqrt(1 - ab) z at every level."""
    ab, ts = grid64(S, spacing)
    lam = 0.5 * torch.log(ab / (1 - ab))
    lvl = lambda a: torch.sqrt(a) * x0 + torch.sqrt(1 - a) * z
    x = z if m is None else torch.where(m, lvl(ab[ts[0]]), z)
    d_prev = h_prev = None
    for i, s in enumerate(ts):
        eps = eps_fn(x, torch.full((x.shape[0],), s, dtype=torch.int64))
        al_s, sg_s = torch.sqrt(ab[s]), torch.sqrt(1 - ab[s])
        d = (x - sg_s * eps) / al_s
        if i + 1 < S:
            t = ts[i + 1]
            al_t, sg_t = torch.sqrt(ab[t]), torch.sqrt(1 - ab[t])
            h = lam[t] - lam[s]
            D = d
            if solver == "dpmpp2m" and i > 0:
                r = h_prev / h
                D = (1 + 1 / (2 * r)) * d - d_prev / (2 * r)
            new = (sg_t / sg_s) * x - al_t * torch.expm1(-h) * D
            ab_p = ab[t]
            h_prev = h
        else:
            new, ab_p = d, torch.tensor(1.0, dtype=torch.float64)
        d_prev = d
        x = new if m is None else torch.where(m, lvl(ab_p), new)
    return x


def rel_max(a, e):
    a, e = a.detach().cpu().double(), e.detach().cpu().double()
    assert a.shape == e.shape and bool(torch.isfinite(a).all())
    return float((a - e).abs().max()) / max(float(e.abs().max()), 1e-30)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the loops against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, BF])
@pytest.mark.parametrize("spacing", ["time", "logsnr"])
@pytest.mark.parametrize("kind", ["mlp", "transformer"])
def test_unmasked_loop_matches_float64(kind, spacing, dt):
    """the bounds the DDIM loop is held to in tests/test_cond_sampler_gpu.py: 2e-3 (fp32) and 4e-2 (bf16) of max |want|"""
    from inferbiomechanics_amd.diffusion.sampler import DDIMSampler
    model = small_models(dt)[kind]
    B, T, D, S = 3, 24, 44, 10
    xT = R.det_fill((B, T, D), 11, 1.0, torch.float32).to(dt)
    fn = eps_fn64(model, kind)
    for solver in ("dpmpp2m", "ddim"):
        if solver == "ddim" and spacing == "time":
            continue                                               # today's loop: tests/test_sampler_gpu.py
        got = DDIMSampler(model, S, solver=solver, spacing=spacing).sample(xT.to(DEV))
        with torch.no_grad():
            want = loop64(fn, xT.double(), S, spacing, solver)
        err = rel_max(got, want)
        print(f"unmasked {kind} {dt} {spacing} {solver}: rel max err {err:.3e} (bound {BOUND[dt]:.0e})")
        assert got.dtype == dt and err <= BOUND[dt], (solver, err)


@pytest.mark.parametrize("dt", [torch.float32, BF])
@pytest.mark.parametrize("spacing", ["time", "logsnr"])
@pytest.mark.parametrize("kind", ["mlp", "transformer"])
def test_masked_loop_matches_float64(kind, spacing, dt):
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler
    model = small_models(dt)[kind]
    B, T, D, S = 3, 24, 44, 10
    xT = R.det_fill((B, T, D), 11, 1.0, torch.float32).to(dt)
    obs = R.det_fill((B, T, D), 15, 1.0, torch.float32).to(dt)
    m = label_mask(T, D)
    fn = eps_fn64(model, kind)
    for solver in ("dpmpp2m", "ddim"):
        if solver == "ddim" and spacing == "time":
            continue                                               # today's loop: tests/test_cond_sampler_gpu.py
        got = ConditionalDDIMSampler(model, S, solver=solver, spacing=spacing).sample(xT.to(DEV), obs.to(DEV), m)
        with torch.no_grad():
            want = loop64(fn, xT.double(), S, spacing, solver, obs.double(), m)
        err = rel_max(got[:, :, D - 30:], want[:, :, D - 30:])
        print(f"masked {kind} {dt} {spacing} {solver}: rel max err of the inferred columns {err:.3e} (bound {BOUND[dt]:.0e})")
        assert err <= BOUND[dt], (solver, err)
        assert torch.equal(got.cpu()[:, m], obs[:, m]), "observed elements must equal the observation"


# ---------------------------------------------------------------------------------------------------------------------
# 2. exact relations of the masked loop
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, BF])
@pytest.mark.parametrize("kind", ["mlp", "transformer"])
def test_empty_mask_equals_the_unmasked_sampler(dt, kind):
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler, DDIMSampler
    model = small_models(dt)[kind]
    B, T, D, S = 3, 24, 44, 10
    xT = R.det_fill((B, T, D), 11, 1.0, torch.float32).to(DEV)
    obs = R.det_fill((B, T, D), 12, 1.0, torch.float32).to(DEV)
    for spacing in ("time", "logsnr"):
        want = DDIMSampler(model, S, solver="dpmpp2m", spacing=spacing).sample(xT)
        got = ConditionalDDIMSampler(model, S, solver="dpmpp2m", spacing=spacing).sample(xT, obs, torch.zeros(T, D, dtype=torch.bool))
        assert torch.equal(got, want), spacing
        assert not torch.equal(want, DDIMSampler(model, S, spacing=spacing).sample(xT)), "the solver must change the result"


@pytest.mark.parametrize("dt", [torch.float32, BF])
def test_full_mask_returns_the_observation(dt):
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler
    model = small_models(dt)["transformer"]
    B, T, D, S = 3, 24, 44, 10
    xT = R.det_fill((B, T, D), 13, 1.0, torch.float32)
    obs = R.det_fill((B, T, D), 14, 2.0, torch.float32)
    got = ConditionalDDIMSampler(model, S, solver="dpmpp2m", spacing="logsnr").sample(xT.to(DEV), obs.to(DEV),
                                                                                       torch.ones(T, D, dtype=torch.bool))
    assert got.dtype == dt and torch.equal(got.cpu(), obs.to(dt))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the captured step is replayed for a new batch; steps= truncates; sample_noise
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, BF])
def test_second_batch_replays_the_captured_step(dt):
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler, DDIMSampler
    model = small_models(dt)["transformer"]
    B, T, D, S = 3, 24, 44, 10
    kw = dict(solver="dpmpp2m", spacing="logsnr")
    z1, z2 = (R.det_fill((B, T, D), k, 1.0, torch.float32).to(DEV) for k in (21, 22))
    o1, o2 = (R.det_fill((B, T, D), k, 1.0, torch.float32).to(DEV) for k in (23, 24))
    m1, m2 = label_mask(T, D), label_mask(T, D, free=12)
    smp = ConditionalDDIMSampler(model, S, **kw)
    a = smp.sample(z1, o1, m1)
    graph, hist = smp._graph, smp._bufs["hist"]
    assert graph is not None and hist.dtype == torch.float32
    b = smp.sample(z2, o2, m2)
    assert smp._graph is graph and smp._bufs["hist"] is hist, "a batch of the same shape must replay the captured step"
    assert torch.equal(a, ConditionalDDIMSampler(model, S, **kw).sample(z1, o1, m1))
    assert torch.equal(b, ConditionalDDIMSampler(model, S, **kw).sample(z2, o2, m2))
    assert not torch.equal(a, b)
    assert torch.equal(a, ConditionalDDIMSampler(model, S, use_graph=False, **kw).sample(z1, o1, m1)), "replay and eager loop differ"
    un = DDIMSampler(model, S, **kw)
    u1 = un.sample(z1)
    g2 = un._graph
    u2 = un.sample(z2)
    assert un._graph is g2 and g2 is not None
    assert torch.equal(u1, DDIMSampler(model, S, use_graph=False, **kw).sample(z1))
    assert torch.equal(u2, DDIMSampler(model, S, **kw).sample(z2))
    # steps= truncates the loop: the first k steps of the full one
    part = DDIMSampler(model, S, use_graph=False, **kw).sample(z1, steps=4)
    assert part.shape == u1.shape and bool(torch.isfinite(part).all()) and not torch.equal(part, u1)
    assert torch.equal(part, DDIMSampler(model, S, **kw).sample(z1, steps=4))
    # the device draw
    zs = un.draw_start(B, T, D, seed=7, draw=3)
    assert torch.equal(un.sample_noise(B, T, D, seed=7, draw=3), un.sample(zs))
    # another solver or grid on the same model re-captures instead of replaying stale tables
    other = DDIMSampler(model, S).sample(z1)
    assert torch.equal(un.sample(z1), u1) and torch.equal(DDIMSampler(model, S).sample(z1), other)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the defaults
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, BF])
@pytest.mark.parametrize("kind", ["mlp", "transformer"])
def test_default_arguments_are_the_ddim_loop_bit_for_bit(dt, kind):
    """a sampler built without the new arguments, one built with their defaults spelled out, and the DDIM loop written out
    over the model's plan with ib_ddim_step (what the sampler launched before it had a solver argument)"""
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler, DDIMSampler
    model = small_models(dt)[kind]
    B, T, D, S = 3, 24, 44, 10
    xT = R.det_fill((B, T, D), 11, 1.0, torch.float32).to(DEV)
    obs = R.det_fill((B, T, D), 12, 1.0, torch.float32).to(DEV)
    m = label_mask(T, D)
    DDIMSampler(model, S, solver="dpmpp2m", spacing="logsnr").sample(xT)          # leaves other tables behind on the model
    a = DDIMSampler(model, S).sample(xT)
    b = DDIMSampler(model, S, solver="ddim", spacing="time").sample(xT)
    assert torch.equal(a, b)
    tabs = model.tables(model._flat.device)
    assert tabs.spacing == "time" and tabs.ddim_t.tolist() == R.ddim_timesteps(N, S).tolist()
    assert torch.equal(tabs.ddim_coef.cpu(), R.ddim_coeffs(N, S).to(torch.float32))
    c = ConditionalDDIMSampler(model, S).sample(xT, obs, m)
    d = ConditionalDDIMSampler(model, S, solver="ddim", spacing="time").sample(xT, obs, m)
    assert torch.equal(c, d)
    with hip.record_launches() as rec:
        DDIMSampler(model, S, use_graph=False).sample(xT)
        ConditionalDDIMSampler(model, S, use_graph=False).sample(xT, obs, m)
    names = [n for n, _ in rec.calls]
    assert names.count("ib_ddim_step") == S and names.count("ib_ddim_cond_step") == S
    assert not [n for n in names if n.startswith("ib_dpmpp_")]


# ---------------------------------------------------------------------------------------------------------------------
# 5. the predictor
# ---------------------------------------------------------------------------------------------------------------------
def windows(n):
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import SyntheticWindowDataset
    ds = SyntheticWindowDataset(n, 50, 5)
    items = [ds[i] for i in range(n)]
    return ({k: torch.stack([it[0][k] for it in items]) for k in items[0][0]},
            {k: torch.stack([it[1][k] for it in items]) for k in items[0][1]})


@pytest.mark.parametrize("dt", [torch.float32, BF])
def test_predictor_with_the_new_solver_returns_mean_and_std(dt):
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import LOSS_KEY_ORDER, LOSS_KEY_WIDTHS
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionMLP
    from inferbiomechanics_amd.models.DiffusionLabelPredictor import DiffusionLabelPredictor
    inputs, labels = windows(4)
    model = DiffusionMLP(177, [64, 64], device=DEV, compute_dtype=dt)
    load_det(model)
    pred = DiffusionLabelPredictor(model, 20, seed=3, solver='dpmpp2m', spacing='logsnr', num_samples=3)
    out = pred(inputs, labels, draw=2)
    assert list(out) == LOSS_KEY_ORDER and list(pred.last_std) == LOSS_KEY_ORDER
    for k, w in zip(LOSS_KEY_ORDER, LOSS_KEY_WIDTHS):
        assert out[k].shape == pred.last_std[k].shape == (4, 10, w)
        assert out[k].dtype == pred.last_std[k].dtype == torch.float32
        assert bool(torch.isfinite(out[k]).all()) and bool(torch.isfinite(pred.last_std[k]).all())
        assert bool((pred.last_std[k] >= 0).all())
    assert any(float(pred.last_std[k].max()) > 0 for k in LOSS_KEY_ORDER), "members differ by their start draws"
    assert math.isfinite(sum(float(v.sum()) for v in out.values()))
