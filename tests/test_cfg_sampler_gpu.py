"""Guided sampling (classifier-free guidance, `guidance = s`) of the masked samplers against a loop driven by hand from the
same public pieces: plan.forward over a 2B input the test assembles with torch copies, hip.cfg_combine, and the existing
hip.*_step entry of the row.  The forward's shape is the guided sampler's, so its dispatch is, so the two are held bit for bit,
captured and with use_graph = False.  Small denoisers with cond_drop set (the 2-layer transformer, d_model 128, in bf16 and
fp32, and the bf16 MLP), B = 3, T = 12, D = 44, C = 14, four sampling steps.  -m gpu."""
import pytest
import torch

from oracle import ref_cpu as R
from tests.test_cond_trainer_gpu import BF, DEV, make

pytestmark = pytest.mark.gpu

B, T, D, C, S = 3, 12, 44, 14, 4
G = 1.5
SEED = 5
KINDS = [("transformer", BF), ("mlp", BF), ("transformer", torch.float32)]
SETTINGS = [("ddim", 0.0, "time"), ("ddim", 1.0, "time"), ("dpmpp2m", 0.0, "time"), ("dpmpp2m_sde", 1.0, "logsnr")]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from inferbiomechanics_amd import hip
    hip.lib()


def model_for(kind, dtype, window=T):
    m, _ = make(kind, dtype, D, window)
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


def hand_loop(model, x_T, observed, mask, solver, eta, spacing, lay=None, N=None):
    """the guided loop over the window batch x_T [B, T, D], driven from the test: returns the state's D columns"""
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion.sampler import _cut, _join
    from inferbiomechanics_amd.diffusion.schedule import stitch_layout
    m, dt = model, model.compute_dtype
    nb = x_T.shape[0]
    m.ensure_packed()
    m.sync_shadow()
    dev = m._flat.device
    tabs = m.tables(dev)
    tabs.set_sampler(S, eta, solver, spacing, observations="clean")
    plan = m._get_plan(dev)
    Dp = plan.infer_pitch(D) if (hasattr(plan, "infer_pitch") and dt == BF) else D
    z3 = lambda n=nb, dtype=dt: torch.zeros((n, T, Dp), dtype=dtype, device=dev)
    xin, eps, x0, z, hist = z3(2 * nb), z3(2 * nb), z3(), z3(), z3(dtype=torch.float32)
    t = torch.empty(2 * nb, dtype=torch.int64, device=dev)
    ctr = torch.zeros(1, dtype=torch.int32, device=dev)
    mk = torch.zeros((T, Dp), dtype=torch.uint8, device=dev)
    win = torch.arange(nb if lay is None else N, dtype=torch.int64, device=dev)
    x = xin[:nb]
    x[:, :, :D].copy_(x_T.to(dt))
    x0[:, :, :D].copy_(observed.to(dt))
    mk[:, :D].copy_(mask.to(device=dev, dtype=torch.uint8))
    z.copy_(x)
    hip.ddim_cond_init(x, x0, z, mk, tabs.obs_coef, D=D)
    if lay is not None:
        x.copy_(_cut(lay, _join(lay, x, N)))
    hip.fill_i64(t, int(tabs.ddim_t[0]))

    def mirror():                                            # ib_cfg_mirror, as torch copies
        xin[nb:, :, C:D].copy_(xin[:nb, :, C:D])
        t[nb:].copy_(t[:nb])

    mirror()
    P = m.param_source()
    if hasattr(plan, "set_inference"):
        plan.set_inference(True)
        plan.prepare_inference(P, T, D, table=tabs.temb)
    one = tuple(a.to(dev) for a in stitch_layout(T, T, T)[:3])
    try:
        for _ in range(S):
            plan.forward(xin.view(2 * nb * T, Dp)[:, :D], t, tabs.temb, P, out=eps.view(2 * nb * T, Dp)[:, :D], BT=(2 * nb, T))
            hip.cfg_combine(eps, G)
            e, step = eps[:nb], dict(step_dev=ctr, t_out=t[:nb])
            if lay is not None:
                v = lambda a: a.view((N, lay["W"]) + tuple(a.shape[1:]))
                hip.stitch_ddim_step(v(x), v(e), v(x0), v(z), mk, tabs.ddim_coef, tabs.obs_coef, tabs.ddim_t, lay["start"],
                                     lay["cover"], lay["wn"], D=D, **step)
            elif solver == "dpmpp2m_sde":
                v = lambda a: a.view((nb, 1) + tuple(a.shape[1:]))
                hip.sde_dpmpp_step(v(x), v(e), v(hist), v(x0), v(z), mk, tabs.sde_coef, tabs.obs_coef, tabs.sde_obs_noise_coef,
                                   tabs.ddim_t, *one, win, SEED, D=D, **step)
            elif solver == "dpmpp2m":
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
    assert not xin[nb:, :, :C].any() and not xin[:, :, D:].any(), "the null condition and the pad columns stay zero"
    return x[:, :, :D].clone()


@pytest.mark.parametrize("solver,eta,spacing", SETTINGS)
@pytest.mark.parametrize("kind,dtype", KINDS)
def test_guided_sampler_is_the_hand_driven_loop_bitwise(kind, dtype, solver, eta, spacing):
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler
    model = model_for(kind, dtype)
    z, obs = batch(B, T, 31)
    mask = prefix_mask()
    want = hand_loop(model, z, obs, mask, solver, eta, spacing)
    assert torch.isfinite(want).all() and torch.equal(want[:, :, :C], obs.to(dtype)[:, :, :C])
    kw = dict(eta=eta, seed=SEED, solver=solver, spacing=spacing, observations="clean")
    for use_graph in (False, True):
        smp = ConditionalDDIMSampler(model, S, use_graph=use_graph, guidance=G, **kw)
        got = smp.sample(z, obs, mask)
        assert (smp._graph is not None) == use_graph
        assert torch.equal(got, want), f"use_graph = {use_graph}"
        xin = smp._bufs["xin"]
        assert not xin[B:, :, :C].any() and not xin[:, :, D:].any()
        assert torch.equal(xin[B:, :, C:D], xin[:B, :, C:D])
    plain = ConditionalDDIMSampler(model, S, **kw).sample(z, obs, mask)
    assert not torch.equal(plain[:, :, C:], want[:, :, C:]), "guidance must move the free columns"


@pytest.mark.parametrize("dtype", [BF, torch.float32])
def test_guided_stitched_call_is_the_hand_driven_loop_bitwise(dtype):
    from inferbiomechanics_amd.diffusion.sampler import StitchedDDIMSampler, _cut, _join
    N, F, hop = 2, 20, 4
    model = model_for("transformer", dtype)
    z, obs = batch(N, F, 41)
    cols = prefix_mask()[0].clone()
    got = {}
    for use_graph in (False, True):
        smp = StitchedDDIMSampler(model, S, hop=hop, use_graph=use_graph, observations="clean", guidance=G)
        got[use_graph] = smp.sample(z, obs, cols)
        assert (smp._graph is not None) == use_graph
    lay = smp.layout
    assert lay["W"] == 3
    mask = cols[None, :].expand(T, D)
    want = _join(lay, hand_loop(model, _cut(lay, z), _cut(lay, obs), mask, "ddim", 0.0, "time", lay=lay, N=N), N)
    assert want.shape == (N, F, D) and torch.isfinite(want).all()
    for use_graph in (False, True):
        assert torch.equal(got[use_graph], want), f"use_graph = {use_graph}"
    plain = StitchedDDIMSampler(model, S, hop=hop, observations="clean").sample(z, obs, cols)
    assert not torch.equal(plain[:, :, C:], want[:, :, C:])


@pytest.mark.parametrize("kind,dtype", KINDS)
def test_guidance_zero_is_the_unguided_sampler_bitwise(kind, dtype):
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler
    model = model_for(kind, dtype)
    z, obs = batch(B, T, 51)
    a = ConditionalDDIMSampler(model, S, observations="clean")
    b = ConditionalDDIMSampler(model, S, observations="clean", guidance=0.0)
    assert torch.equal(a.sample(z, obs, prefix_mask()), b.sample(z, obs, prefix_mask()))
    assert "xin" not in b._bufs and tuple(b._bufs["t"].shape) == (B,)
    assert [type(e) for e in a._sig] == [type(e) for e in b._sig] and "cfg" not in b._sig


@pytest.mark.parametrize("kind,dtype", [("transformer", BF), ("mlp", BF)])
def test_a_new_batch_replays_the_captured_step(kind, dtype):
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler
    model = model_for(kind, dtype)
    mask = prefix_mask()
    kw = dict(eta=1.0, seed=SEED, observations="clean", guidance=G)
    smp = ConditionalDDIMSampler(model, S, **kw)
    first = smp.sample(*batch(B, T, 61), mask)
    graph, sig = smp._graph, smp._sig
    assert graph is not None
    z2, obs2 = batch(B, T, 71)
    second = smp.sample(z2, obs2, mask)
    assert smp._graph is graph and smp._sig == sig, "a new batch of the same shape must replay the captured step"
    fresh = ConditionalDDIMSampler(model, S, **kw).sample(z2, obs2, mask)
    assert torch.equal(second, fresh) and not torch.equal(second, first)


def test_label_predictor_with_guidance():
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import INPUT_KEY_ORDER, LOSS_KEY_ORDER, LOSS_KEY_WIDTHS, \
        SyntheticWindowDataset
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    from inferbiomechanics_amd.models.DiffusionLabelPredictor import DiffusionLabelPredictor
    ds = SyntheticWindowDataset(4, history_len=50, stride=5, seed=2)
    inputs = {k: torch.stack([ds[i][0][k] for i in range(2)]) for k in INPUT_KEY_ORDER}
    n, F, Dl = DiffusionLabelPredictor.window_matrix(inputs).shape
    torch.manual_seed(0)
    model = DiffusionTransformer(Dl, F, d_model=128, num_heads=4, dim_feedforward=256, num_layers=2, device=DEV,
                                 compute_dtype=BF)
    model.cond_cols = Dl - 30
    with pytest.raises(ValueError, match="cond-drop"):
        DiffusionLabelPredictor(model, S, seed=3, guidance=G)
    model.cond_drop = 0.1
    pred = DiffusionLabelPredictor(model, S, seed=3, guidance=G)
    out = pred(inputs)
    assert pred.sampler.guidance == G and "xin" in pred.sampler._bufs
    trial_inputs = {k: torch.cat([v, v], dim=1) for k, v in inputs.items()}              # [n, 2 F, c]
    trial = pred.predict_trial(trial_inputs, hop=4)
    assert pred._trial[1].guidance == G and "xin" in pred._trial[1]._bufs
    for k, w in zip(LOSS_KEY_ORDER, LOSS_KEY_WIDTHS):
        assert tuple(out[k].shape) == (n, F, w) and torch.isfinite(out[k]).all()
        assert tuple(trial[k].shape) == (n, 2 * F, w) and torch.isfinite(trial[k]).all()
    unguided = DiffusionLabelPredictor(model, S, seed=3)(inputs)
    assert any(not torch.equal(unguided[k], out[k]) for k in LOSS_KEY_ORDER)
