"""The x0 clip inside the samplers (`x0_clip = X0Clip(...)`, diffusion/sampler.py).  Off -- None, or bounds that are all
infinite -- every sampler is the sampler without the keyword bit for bit.  On, the captured loop is a loop driven by hand
from the same public pieces (plan.forward, hip.x0_clip_range / hip.x0_clip_dynamic, the row's hip.*_step entry, the
counter), bit for bit, and the final sample of a deterministic fp32 'range' loop lies inside the bounds up to the roundings of
its last step.  Small denoisers (the 2-layer transformer, d_model 128), B = 3, T = 12, D = 44, four sampling steps.  -m gpu."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
from tests.test_cond_trainer_gpu import BF, DEV, make

pytestmark = pytest.mark.gpu

B, T, D, C, S = 3, 12, 44, 14, 4
G = 1.5
SEED = 5
INF = float("inf")
DTYPES = [BF, torch.float32]
LOOPS = [("ddim", 0.0, False), ("ddim", 1.0, False), ("dpmpp2m", 0.0, False), ("ddim", 0.0, True)]   # solver, eta, guided


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from inferbiomechanics_amd import hip
    hip.lib()


def model_for(dtype, window=T):
    m, _ = make("transformer", dtype, D, window)
    m.cond_cols, m.cond_drop = C, 0.1
    m.eval()
    return m


def batch(n, frames, seed):
    z = R.det_fill((n, frames, D), seed, 1.0, torch.float32).to(DEV)
    obs = R.det_fill((n, frames, D), seed + 1, 2.0, torch.float32).to(DEV)
    return z, obs


def prefix_mask():
    m = torch.zeros(T, D, dtype=torch.bool)
    m[:, :C] = True
    return m


def tight(mode, quantile=0.9):
    """bounds far inside what an untrained denoiser predicts, column C + 1 without a bound"""
    from inferbiomechanics_amd.diffusion.sampler import X0Clip
    c = np.arange(D)
    lo, hi = -0.2 - 0.05 * (c % 3), 0.3 + 0.05 * (c % 4)
    lo[C + 1], hi[C + 1] = -INF, INF
    return X0Clip(lo.tolist(), hi.tolist(), mode=mode, quantile=quantile)


def unbounded():
    from inferbiomechanics_amd.diffusion.sampler import X0Clip
    return X0Clip([-INF] * D, [INF] * D, mode="dynamic")


def hand_loop(model, x_T, observed, mask, solver, eta, clip, guided):
    """the masked loop over x_T [B, T, D] with the clip's launch issued by hand -> (the state's D columns, max |x| and
    max |eps| over them as the last update read them)"""
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion.schedule import clip_rank
    m, dt = model, model.compute_dtype
    nb, rows = x_T.shape[0], (2 if guided else 1) * x_T.shape[0]
    m.ensure_packed()
    m.sync_shadow()
    dev = m._flat.device
    tabs = m.tables(dev)
    tabs.set_sampler(S, eta, solver, "time", observations="clean" if guided else "noised")
    tabs.set_clip(clip.lo, clip.hi)
    ct = tabs.clip
    plan = m._get_plan(dev)
    Dp = plan.infer_pitch(D) if (hasattr(plan, "infer_pitch") and dt == BF) else D
    z3 = lambda n=nb, dtype=dt: torch.zeros((n, T, Dp), dtype=dtype, device=dev)
    xin, x0, z, hist = z3(rows), z3(), z3(), z3(dtype=torch.float32)
    eps = z3(rows) if (guided or Dp != D) else None
    t = torch.empty(rows, dtype=torch.int64, device=dev)
    ctr = torch.zeros(1, dtype=torch.int32, device=dev)
    mk = torch.zeros((T, Dp), dtype=torch.uint8, device=dev)
    win = torch.arange(nb, dtype=torch.int64, device=dev)
    x = xin[:nb]
    x[:, :, :D].copy_(x_T.to(dt))
    x0[:, :, :D].copy_(observed.to(dt))
    mk[:, :D].copy_(mask.to(device=dev, dtype=torch.uint8))
    z.copy_(x)
    hip.ddim_cond_init(x, x0, z, mk, tabs.obs_coef, D=D)
    hip.fill_i64(t, int(tabs.ddim_t[0]))
    n = int((mask.cpu() == 0).sum(dim=0)[ct["bounded"]].sum())
    k = clip_rank(clip.quantile, n)

    def mirror():                                                      # ib_cfg_mirror, as torch copies
        if guided:
            xin[nb:, :, C:D].copy_(xin[:nb, :, C:D])
            t[nb:].copy_(t[:nb])

    mirror()
    P = m.param_source()
    if hasattr(plan, "set_inference"):
        plan.set_inference(True)
        plan.prepare_inference(P, T, D, table=tabs.temb)
    last = None
    try:
        for s in range(S):
            if eps is None:
                e = plan.forward(x, t, tabs.temb, P)
            else:
                plan.forward(xin.view(rows * T, Dp)[:, :D], t, tabs.temb, P, out=eps.view(rows * T, Dp)[:, :D], BT=(rows, T))
                if guided:
                    hip.cfg_combine(eps, G)
                e = eps[:nb]
            if clip.mode == "range":
                hip.x0_clip_range(x, e, mk, ct["lo"], ct["hi"], ct["coef"], step_dev=ctr, D=D)
            else:
                hip.x0_clip_dynamic(x, e, mk, ct["lo"], ct["hi"], ct["coef"], ct["m"], ct["h"], ct["ih"], k, step_dev=ctr, D=D)
            if s == S - 1:
                last = (float(x[:, :, :D].float().abs().max()), float(e[:, :, :D].float().abs().max()))
            step = dict(step_dev=ctr, t_out=t[:nb])
            if solver == "dpmpp2m":
                hip.dpmpp_cond_step(x, e, hist, x0, z, mk, tabs.dpmpp_coef, tabs.obs_coef, tabs.ddim_t, D=D, **step)
            elif eta > 0.0:
                hip.ddim_cond_step_noise(x, e, x0, z, mk, tabs.ddim_coef_eta, tabs.obs_coef, tabs.obs_noise_coef, tabs.ddim_t,
                                         win, SEED, D=D, **step)
            else:
                hip.ddim_cond_step(x, e, x0, z, mk, tabs.ddim_coef, tabs.obs_coef, tabs.ddim_t, D=D, **step)
            mirror()
            hip.counter_add(ctr, 1)
    finally:
        if hasattr(plan, "set_inference"):
            plan.set_inference(False)
    torch.cuda.synchronize()
    return x[:, :, :D].clone(), last


@pytest.mark.parametrize("mode", ["range", "dynamic"])
@pytest.mark.parametrize("solver,eta,guided", LOOPS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_clipped_sampler_is_the_hand_driven_loop_bitwise(dtype, solver, eta, guided, mode):
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler
    model = model_for(dtype)
    z, obs = batch(B, T, 31)
    mask, clip = prefix_mask(), tight(mode)
    want, _ = hand_loop(model, z, obs, mask, solver, eta, clip, guided)
    assert torch.isfinite(want).all()
    kw = dict(eta=eta, seed=SEED, solver=solver, observations="clean" if guided else "noised",
              guidance=G if guided else 0.0)
    for use_graph in (False, True):
        smp = ConditionalDDIMSampler(model, S, use_graph=use_graph, x0_clip=clip, **kw)
        got = smp.sample(z, obs, mask)
        assert (smp._graph is not None) == use_graph and "x0_clip" in smp._sig
        assert torch.equal(got, want), f"use_graph = {use_graph}"
    plain = ConditionalDDIMSampler(model, S, **kw).sample(z, obs, mask)
    assert not torch.equal(plain[:, :, C:], want[:, :, C:]), "tight bounds must move the free columns"
    assert torch.equal(plain[:, :, :C], want[:, :, :C]), "the observed columns are the unclipped loop's"


def test_final_sample_lies_inside_the_bounds_up_to_the_last_steps_roundings():
    """fp32, eta = 0, 'range'.  The last row of the update is (cx, ce) = (1 / a, -s / a), so in real arithmetic the last step
    returns exactly the clipped prediction: cx x + ce (x - a x0c) / s = x0c, which lies inside [lo, hi].  What is computed
    differs by roundings, each of relative size at most u = 2^-24: the casts of a, 1 / s, cx and ce (4), r = fma(-a, x0c, x)
    (1), e' = r * is (1), and the update's two products and their sum (at most 3) -- 9 in all, acting on terms no larger
    than M = cx max|x| + |ce| max|e'|, x and e' as the last update reads them (taken from the hand-driven loop, which is the
    sampler bit for bit).  The margin is 12 u M: the 9 first-order terms and room for their products."""
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler
    dtype = torch.float32
    model = model_for(dtype)
    z, obs = batch(B, T, 41)
    mask, clip = prefix_mask(), tight("range")
    want, (xmax, emax) = hand_loop(model, z, obs, mask, "ddim", 0.0, clip, False)
    got = ConditionalDDIMSampler(model, S, x0_clip=clip).sample(z, obs, mask)
    assert torch.equal(got, want)
    cx, ce = (float(v) for v in model.tables(model._flat.device).ddim_coef[S - 1])
    margin = 12.0 * 2.0 ** -24 * (abs(cx) * xmax + abs(ce) * emax)
    lo, hi = torch.tensor(clip.lo, dtype=torch.float64), torch.tensor(clip.hi, dtype=torch.float64)
    free = (~mask)[None].expand(B, T, D) & (torch.isfinite(lo) & torch.isfinite(hi))[None, None, :]
    v = got.cpu().double()
    over = torch.maximum(v - hi, lo - v).clamp(min=0.0)
    print("largest excess", float(over[free].max()), "margin", margin)
    assert 0.0 < margin < 1e-4 and float(over[free].max()) <= margin
    assert torch.equal(got[:, :, :C], obs[:, :, :C]), "observed elements equal the observation"


@pytest.mark.parametrize("dtype", DTYPES)
def test_off_and_infinite_bounds_are_the_unclipped_samplers_bitwise(dtype):
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler, DDIMSampler, StitchedDDIMSampler
    model = model_for(dtype)
    z, obs = batch(B, T, 51)
    zt, obst = batch(2, 20, 61)
    mask, cols = prefix_mask(), prefix_mask()[0].clone()
    runs = {
        "unmasked": lambda **kw: DDIMSampler(model, S, **kw).sample(z),
        "masked": lambda **kw: ConditionalDDIMSampler(model, S, eta=1.0, seed=SEED, **kw).sample(z, obs, mask),
        "stitched": lambda **kw: StitchedDDIMSampler(model, S, hop=4, **kw).sample(zt, obst, cols),
        "guided": lambda **kw: ConditionalDDIMSampler(model, S, observations="clean", guidance=G, **kw).sample(z, obs, mask),
    }
    for name, run in runs.items():
        base = run()
        assert torch.equal(run(x0_clip=None), base), name
        assert torch.equal(run(x0_clip=unbounded()), base), name
    off = ConditionalDDIMSampler(model, S, x0_clip=None)
    off.sample(z, obs, mask)
    assert "x0_clip" not in off._sig


def test_stitched_sampler_clips_every_window_and_replays():
    from inferbiomechanics_amd.diffusion.sampler import StochasticStitchedSampler
    model = model_for(BF)
    zt, obst = batch(2, 20, 71)
    cols = prefix_mask()[0].clone()
    kw = dict(eta=1.0, hop=4, seed=SEED)
    plain = StochasticStitchedSampler(model, S, **kw).sample(zt, obst, cols)
    for mode in ("range", "dynamic"):
        eager = StochasticStitchedSampler(model, S, use_graph=False, x0_clip=tight(mode), **kw).sample(zt, obst, cols)
        smp = StochasticStitchedSampler(model, S, x0_clip=tight(mode), **kw)
        got = smp.sample(zt, obst, cols)
        assert smp._graph is not None and torch.equal(got, eager) and torch.isfinite(got).all()
        assert not torch.equal(got[:, :, C:], plain[:, :, C:]) and torch.equal(got[:, :, :C], plain[:, :, :C])


def test_label_predictor_takes_label_bounds_or_row_bounds():
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import INPUT_KEY_ORDER, LOSS_KEY_ORDER, SyntheticWindowDataset
    from inferbiomechanics_amd.diffusion.sampler import X0Clip
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    from inferbiomechanics_amd.models.DiffusionLabelPredictor import DiffusionLabelPredictor
    ds = SyntheticWindowDataset(4, history_len=50, stride=5, seed=2)
    inputs = {k: torch.stack([ds[i][0][k] for i in range(2)]) for k in INPUT_KEY_ORDER}
    n, F, Dl = DiffusionLabelPredictor.window_matrix(inputs).shape
    torch.manual_seed(0)
    model = DiffusionTransformer(Dl, F, d_model=128, num_heads=4, dim_feedforward=256, num_layers=2, device=DEV,
                                 compute_dtype=BF)
    lo, hi = [-0.1 - 0.01 * c for c in range(30)], [0.1 + 0.01 * c for c in range(30)]
    for mode in ("range", "dynamic"):
        narrow = DiffusionLabelPredictor(model, S, seed=3, x0_clip=X0Clip(lo, hi, mode=mode))(inputs)
        wide = DiffusionLabelPredictor(model, S, seed=3, x0_clip=X0Clip([-INF] * (Dl - 30) + lo, [INF] * (Dl - 30) + hi,
                                                                         mode=mode))(inputs)
        plain = DiffusionLabelPredictor(model, S, seed=3)(inputs)
        assert all(torch.equal(narrow[k], wide[k]) and torch.isfinite(narrow[k]).all() for k in LOSS_KEY_ORDER)
        assert any(not torch.equal(narrow[k], plain[k]) for k in LOSS_KEY_ORDER)
    with pytest.raises(ValueError, match="x0_clip"):
        DiffusionLabelPredictor(model, S, seed=3, x0_clip=X0Clip(lo[:7], hi[:7]))
