"""The samplers over a model whose output is x0 or v (model.prediction, diffusion/sampler.py).  Every loop -- DDIMSampler with
'ddim' and with 'dpmpp2m', ConditionalDDIMSampler plain, guided and with an x0 clip of mode 'range', StitchedDDIMSampler --
equals, bit for bit, a loop driven by hand from the same public pieces: plan.forward, (hip.cfg_combine,) hip.pred_to_eps,
(hip.x0_clip_range,) the row's hip.*_step entry, the counter; captured and with use_graph = False.  prediction = 'eps' is the
sampler without the attribute, bit for bit.  DiffusionLabelPredictor over a v model with standardisation on runs end to end.
Small randomly initialised denoisers (the 2-layer transformer, d_model 128, bf16 and fp32), B = 3, T = 12, D = 44, C = 14, four
sampling steps: the smallest count above three that divides the 1000 training levels.  -m gpu."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
from tests.test_cond_trainer_gpu import BF, DEV, make

pytestmark = pytest.mark.gpu

B, T, D, C, S = 3, 12, 44, 14, 4
G = 1.5
DTYPES = [BF, torch.float32]
# name -> (class, solver, masked, guided, clipped, stitched)
LOOPS = {"ddim": ("DDIMSampler", "ddim", False, False, False, False),
         "dpmpp2m": ("DDIMSampler", "dpmpp2m", False, False, False, False),
         "cond": ("ConditionalDDIMSampler", "ddim", True, False, False, False),
         "cond_guided": ("ConditionalDDIMSampler", "ddim", True, True, False, False),
         "cond_clip": ("ConditionalDDIMSampler", "ddim", True, False, True, False),
         "cond_dpmpp2m": ("ConditionalDDIMSampler", "dpmpp2m", True, False, False, False),
         "stitched": ("StitchedDDIMSampler", "ddim", True, False, False, True)}
N_TRIALS, FRAMES, HOP = 2, 20, 4


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from inferbiomechanics_amd import hip
    hip.lib()


def model_for(dtype, kind=None):
    m, _ = make("transformer", dtype, D, T)
    m.cond_cols, m.cond_drop = C, 0.1
    if kind is not None:
        m.prediction = kind
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


def the_clip():
    """bounds far inside what an untrained denoiser implies, column C + 1 without a bound"""
    from inferbiomechanics_amd.diffusion.sampler import X0Clip
    c = np.arange(D)
    lo, hi = -0.2 - 0.05 * (c % 3), 0.3 + 0.05 * (c % 4)
    lo[C + 1], hi[C + 1] = -float("inf"), float("inf")
    return X0Clip(lo.tolist(), hi.tolist(), mode="range")


def hand_loop(model, kind, x_T, observed, mask, solver, guided, clip, lay=None, N=None):
    """the loop over the window batch x_T [B, T, D], driven from the test: returns the state's D columns.  observed / mask
    None: the unmasked loop."""
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion.sampler import _cut, _join
    m, dt = model, model.compute_dtype
    masked = observed is not None
    nb, rows = x_T.shape[0], (2 if guided else 1) * x_T.shape[0]
    m.ensure_packed()
    m.sync_shadow()
    dev = m._flat.device
    tabs = m.tables(dev)
    tabs.set_sampler(S, 0.0, solver, "time", observations="clean" if guided else "noised")
    if clip is not None:
        tabs.set_clip(clip.lo, clip.hi)
    plan = m._get_plan(dev)
    Dp = plan.infer_pitch(D) if (hasattr(plan, "infer_pitch") and dt == BF) else D
    z3 = lambda n=nb, dtype=dt: torch.zeros((n, T, Dp), dtype=dtype, device=dev)
    xin, x0, z, hist = z3(rows), z3(), z3(), z3(dtype=torch.float32)
    eps = z3(rows) if (guided or Dp != D) else None
    t = torch.empty(rows, dtype=torch.int64, device=dev)
    ctr = torch.zeros(1, dtype=torch.int32, device=dev)
    mk = torch.zeros((T, Dp), dtype=torch.uint8, device=dev)
    x = xin[:nb]
    x[:, :, :D].copy_(x_T.to(dt))
    if masked:
        x0[:, :, :D].copy_(observed.to(dt))
        mk[:, :D].copy_(mask.to(device=dev, dtype=torch.uint8))
        z.copy_(x)
        hip.ddim_cond_init(x, x0, z, mk, tabs.obs_coef, D=D)
        if lay is not None:
            x.copy_(_cut(lay, _join(lay, x, N)))
    hip.fill_i64(t, int(tabs.ddim_t[0]))

    def mirror():                                                      # ib_cfg_mirror, as torch copies
        if guided:
            xin[nb:, :, C:D].copy_(xin[:nb, :, C:D])
            t[nb:].copy_(t[:nb])

    mirror()
    P = m.param_source()
    if hasattr(plan, "set_inference"):
        plan.set_inference(True)
        plan.prepare_inference(P, T, D, table=tabs.temb)
    try:
        for _ in range(S):
            if eps is None:
                e = plan.forward(x, t, tabs.temb, P)
            else:
                plan.forward(xin.view(rows * T, Dp)[:, :D], t, tabs.temb, P, out=eps.view(rows * T, Dp)[:, :D], BT=(rows, T))
                if guided:
                    hip.cfg_combine(eps, G)
                e = eps[:nb]
            if kind != "eps":
                hip.pred_to_eps(x, e, t[:nb], tabs.sqrt_ab, tabs.sqrt_1mab, tabs.inv_sqrt_1mab, kind, D=D)
            if clip is not None:
                ct = tabs.clip
                hip.x0_clip_range(x, e, mk if masked else None, ct["lo"], ct["hi"], ct["coef"], step_dev=ctr, D=D)
            step = dict(step_dev=ctr, t_out=t[:nb])
            if lay is not None:
                v = lambda a: a.view((N, lay["W"]) + tuple(a.shape[1:]))
                hip.stitch_ddim_step(v(x), v(e), v(x0), v(z), mk, tabs.ddim_coef, tabs.obs_coef, tabs.ddim_t, lay["start"],
                                     lay["cover"], lay["wn"], D=D, **step)
            elif solver == "dpmpp2m" and masked:
                hip.dpmpp_cond_step(x, e, hist, x0, z, mk, tabs.dpmpp_coef, tabs.obs_coef, tabs.ddim_t, D=D, **step)
            elif solver == "dpmpp2m":
                hip.dpmpp_step(x, e, hist, tabs.dpmpp_coef, tabs.ddim_t, **step)
            elif masked:
                hip.ddim_cond_step(x, e, x0, z, mk, tabs.ddim_coef, tabs.obs_coef, tabs.ddim_t, D=D, **step)
            else:
                hip.ddim_step(x, e, tabs.ddim_coef, tabs.ddim_t, **step)
            mirror()
            hip.counter_add(ctr, 1)
    finally:
        if hasattr(plan, "set_inference"):
            plan.set_inference(False)
    torch.cuda.synchronize()
    assert not xin[:, :, D:].any(), "the pad columns stay zero"
    return x[:, :, :D].clone()


def run_sampler(model, name, use_graph, z, obs):
    """the sampler's own run of loop `name` -> (the sample, the sampler)"""
    from inferbiomechanics_amd.diffusion import sampler as mod
    cls, solver, masked, guided, clipped, stitched = LOOPS[name]
    kw = dict(use_graph=use_graph, solver=solver)
    if clipped:
        kw["x0_clip"] = the_clip()
    if guided:
        kw.update(observations="clean", guidance=G)
    if stitched:
        smp = mod.StitchedDDIMSampler(model, S, hop=HOP, **kw)
        return smp.sample(z, obs, prefix_mask()[0].clone()), smp
    smp = getattr(mod, cls)(model, S, **kw)
    return (smp.sample(z, obs, prefix_mask()) if masked else smp.sample(z)), smp


@pytest.mark.parametrize("kind", ["x0", "v"])
@pytest.mark.parametrize("name", sorted(LOOPS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_sampler_is_the_hand_driven_loop_bitwise(dtype, name, kind):
    from inferbiomechanics_amd.diffusion.sampler import _cut, _join
    cls, solver, masked, guided, clipped, stitched = LOOPS[name]
    model = model_for(dtype, kind)
    z, obs = batch(N_TRIALS, FRAMES, 41) if stitched else batch(B, T, 31)
    got = {}
    for use_graph in (False, True):
        got[use_graph], smp = run_sampler(model, name, use_graph, z, obs)
        assert (smp._graph is not None) == use_graph
        i = smp._sig.index("prediction")
        assert smp._sig[i + 1] == kind, "the kind is part of the capture signature"
    clip = the_clip() if clipped else None
    if stitched:
        lay = smp.layout
        assert lay["W"] == 3
        mask = prefix_mask()
        want = _join(lay, hand_loop(model, kind, _cut(lay, z), _cut(lay, obs), mask, solver, guided, clip, lay=lay, N=N_TRIALS),
                     N_TRIALS)
    else:
        want = hand_loop(model, kind, z, obs if masked else None, prefix_mask() if masked else None, solver, guided, clip)
    assert torch.isfinite(want).all()
    for use_graph in (False, True):
        assert torch.equal(got[use_graph], want), f"use_graph = {use_graph}"
    # the conversion is no identity: the same weights read as an eps model give another sample
    plain, _ = run_sampler(model_for(dtype), name, True, z, obs)
    free = slice(C, D) if masked else slice(0, D)
    assert not torch.equal(plain[:, :, free], want[:, :, free])


@pytest.mark.parametrize("name", sorted(LOOPS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_eps_is_the_sampler_without_the_attribute_bitwise(dtype, name):
    stitched = LOOPS[name][5]
    z, obs = batch(N_TRIALS, FRAMES, 61) if stitched else batch(B, T, 51)
    without = model_for(dtype)
    del without.prediction                       # a model object from before the attribute
    assert not hasattr(without, "prediction")
    for use_graph in (False, True):
        base, s0 = run_sampler(without, name, use_graph, z, obs)
        got, s1 = run_sampler(model_for(dtype, "eps"), name, use_graph, z, obs)
        assert torch.equal(got, base), f"use_graph = {use_graph}"
        assert "prediction" not in s1._sig and len(s1._sig) == len(s0._sig)


def test_label_predictor_on_a_v_checkpoint_with_standardisation():
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import INPUT_KEY_ORDER, SyntheticWindowDataset
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    from inferbiomechanics_amd.models.DiffusionLabelPredictor import DiffusionLabelPredictor
    ds = SyntheticWindowDataset(4, history_len=50, stride=5, seed=2)
    inputs = {k: torch.stack([ds[i][0][k] for i in range(2)]) for k in INPUT_KEY_ORDER}
    n, F, Dl = DiffusionLabelPredictor.window_matrix(inputs).shape
    torch.manual_seed(0)
    model = DiffusionTransformer(Dl, F, d_model=128, num_heads=4, dim_feedforward=256, num_layers=2, device=DEV,
                                 compute_dtype=BF)
    g = torch.Generator().manual_seed(4)
    model.column_stats = torch.stack([torch.randn(Dl, generator=g) * 0.1, 0.5 + torch.rand(Dl, generator=g)], dim=1)
    eps_out = DiffusionLabelPredictor(model, S, seed=3)(inputs)
    model.prediction = "v"
    with hip.record_launches() as rec:
        eager = DiffusionLabelPredictor(model, S, seed=3, use_graph=False)(inputs)
    assert [nm for nm, _ in rec.calls].count("ib_pred_to_eps") == S
    out = DiffusionLabelPredictor(model, S, seed=3)(inputs)
    assert sorted(out) == sorted(eps_out)
    for k in out:
        assert out[k].shape == eps_out[k].shape and torch.isfinite(out[k]).all()
        assert torch.equal(out[k], eager[k]), "the captured loop is the uncaptured one"
    assert any(not torch.equal(out[k], eps_out[k]) for k in out), "the same weights read as a v model give other labels"
