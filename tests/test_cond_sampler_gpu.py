"""The masked (inpainting) DDIM sampler on the GPU: ib_ddim_cond_step / ib_ddim_cond_init against a float64 restatement,
ConditionalDDIMSampler against DDIMSampler (empty mask: bit for bit), against the observation (full mask: exactly) and
against the float64 masked loop over the oracle denoisers (label-inference mask), and the captured step replayed for a
new observation batch.  -m gpu."""
import pytest
import torch

from oracle import ref_cpu as R
from oracle.fixture_inputs import det_state

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16


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


def label_mask(T, D, free=30):
    m = torch.ones(T, D, dtype=torch.bool)
    m[:, D - free:] = False
    return m


def masked_loop64(eps_fn, x0, z, m, S):
    """float64 restatement of the masked loop: observed elements sit on sqrt(ab) x0 + sqrt(1 - ab) z at every level, free
    ones take the DDIM update (R.ddim_step) of the oracle's prediction"""
    ab = R.alphas_cumprod(R.linear_beta_schedule(1000))
    ts = R.ddim_timesteps(1000, S)
    lvl = lambda a: torch.sqrt(a) * x0 + torch.sqrt(1 - a) * z
    x = torch.where(m, lvl(ab[ts[0]]), z)
    for i, t in enumerate(ts.tolist()):
        eps = eps_fn(x, torch.full((x.shape[0],), t, dtype=torch.int64))
        ab_p = ab[ts[i + 1]] if i + 1 < len(ts) else torch.tensor(1.0, dtype=torch.float64)
        x = torch.where(m, lvl(ab_p), R.ddim_step(x, eps, ab[t], ab_p))
    return x


def close(a, e, rt, what):
    a, e = a.detach().cpu().double(), e.detach().cpu().double()
    assert a.shape == e.shape, (what, a.shape, e.shape)
    assert torch.isfinite(a).all(), what
    err, ref = float((a - e).abs().max()), max(float(e.abs().max()), 1e-30)
    assert err <= rt * ref, f"{what}: {err} > {rt} * {ref}"


# ---------------------------------------------------------------------------------------------------------------------
# 1. one launch against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,B,D,ld", [(torch.float32, 3, 177, 177), (torch.float32, 4, 177, 177), (BF, 3, 177, 192),
                                       (BF, 2, 300, 320)])
def test_one_masked_step_and_init_against_float64(dt, B, D, ld):
    """fp32 D = 177: the element-wise kernel (T * ld % 8 != 0), at B = 4 with the rounding of ib_ddim_step's 8-wide kernel;
    bf16 pitched rows: the 8-wide kernel.  The mask mixes all-observed, all-free and mixed 8-element vectors."""
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion.schedule import DiffusionTables
    T, S = 10, 10
    g = torch.Generator().manual_seed(1000 * B + D)

    def pitched():
        t = torch.zeros(B, T, ld)
        t[:, :, :D] = torch.randn(B, T, D, generator=g)
        return t.to(dt).to(DEV)

    x, eps, x0, z = pitched(), pitched(), pitched(), pitched()
    m = torch.zeros(T, ld, dtype=torch.uint8)
    m[:, :16] = 1                                                      # whole observed vectors
    m[:, 32:D - 30] = (torch.rand(T, D - 62, generator=g) < 0.5).to(torch.uint8) * 3      # mixed (any nonzero = observed)
    m[1, 40:48] = 0                                                    # ... and free vectors among them
    mb = m.bool()
    md = m.to(DEV)
    tabs = DiffusionTables(torch.device(DEV), num_sample_steps=S)
    coef, oc = tabs.ddim_coef.cpu().double(), tabs.obs_coef.cpu().double()
    X, E, X0, Z = (t.cpu().double() for t in (x, eps, x0, z))
    tol = 2e-6 if dt == torch.float32 else 8e-3

    xi = x.clone()
    hip.ddim_cond_init(xi, x0, z, md, tabs.obs_coef, D=D)
    torch.cuda.synchronize()
    close(xi.cpu()[:, mb], (oc[0, 0] * X0 + oc[0, 1] * Z)[:, mb], tol, "init observed")
    assert torch.equal(xi[:, ~mb.to(DEV)], x[:, ~mb.to(DEV)]), "init must leave free elements as drawn"

    for s in (0, S // 2, S - 1):
        ctr = torch.tensor([s], dtype=torch.int32, device=DEV)
        t_out = torch.full((B,), -7, dtype=torch.int64, device=DEV)
        xs = x.clone()
        hip.ddim_cond_step(xs, eps, x0, z, md, tabs.ddim_coef, tabs.obs_coef, tabs.ddim_t, step_dev=ctr, t_out=t_out, D=D)
        xr, t_ref = x.clone(), torch.full((B,), -7, dtype=torch.int64, device=DEV)
        hip.ddim_step(xr, eps, tabs.ddim_coef, tabs.ddim_t, step_dev=ctr, t_out=t_ref)
        xh = x.clone()
        hip.ddim_cond_step(xh, eps, x0, z, md, tabs.ddim_coef, tabs.obs_coef, tabs.ddim_t, step=s, D=D)
        torch.cuda.synchronize()
        want = torch.where(mb, oc[s + 1, 0] * X0 + oc[s + 1, 1] * Z, coef[s, 0] * X + coef[s, 1] * E)
        close(xs.cpu(), want, tol, f"step {s}")
        free = ~mb.to(DEV)
        assert torch.equal(xs[:, free], xr[:, free]), f"step {s}: free elements differ from ib_ddim_step"
        assert torch.equal(xh, xs), "host step index and device step counter disagree"
        assert torch.equal(t_out, t_ref) and int(ctr) == s
        assert int(t_out[0]) == (int(tabs.ddim_t[s + 1]) if s + 1 < S else 0)
        assert not xs[:, :, D:].any(), "pad columns must stay 0"
        if s == S - 1:
            obs = mb.to(DEV)
            assert torch.equal(xs[:, obs], x0[:, obs]), "the last step must land on the observation"


# ---------------------------------------------------------------------------------------------------------------------
# 2. empty mask: the unconditional sampler, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def small_models(dt):
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionMLP, DiffusionTransformer
    mlp = DiffusionMLP(44, [64, 64], device=DEV, compute_dtype=dt)
    tr = DiffusionTransformer(44, 24, d_model=128, num_heads=2, dim_feedforward=256, num_layers=2, device=DEV,
                              compute_dtype=dt)
    load_det(mlp)
    load_det(tr)
    return {"mlp": mlp, "transformer": tr}


@pytest.mark.parametrize("dt", [torch.float32, BF])
@pytest.mark.parametrize("kind", ["mlp", "transformer"])
def test_empty_mask_equals_the_unconditional_sampler(dt, kind):
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler, DDIMSampler
    model = small_models(dt)[kind]
    B, T, D, S = 3, 24, 44, 10
    xT = R.det_fill((B, T, D), 11, 1.0, torch.float32).to(DEV)
    obs = R.det_fill((B, T, D), 12, 1.0, torch.float32).to(DEV)
    want = DDIMSampler(model, S).sample(xT)
    got = ConditionalDDIMSampler(model, S).sample(xT, obs, torch.zeros(T, D, dtype=torch.bool))
    assert torch.equal(got, want)


@pytest.fixture(scope="module")
def bench_model():
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    torch.manual_seed(0)                               # bench.py::build_model
    return DiffusionTransformer(300, 200, d_model=512, num_heads=8, dim_feedforward=2048, num_layers=4, device=DEV,
                                compute_dtype=BF)


@pytest.mark.parametrize("B", [1, 16, 256])
def test_empty_mask_equals_the_unconditional_sampler_at_the_benched_shape(bench_model, B):
    """the benched plan (the kernel families of test_sampler_step_gpu.py, read back per launch): at B = 256 the main /
    side-branch split of the fused launches"""
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler, DDIMSampler
    T, D, S = 200, 300, 100
    g = torch.Generator().manual_seed(200 + B)
    xT = torch.randn(B, T, D, generator=g).to(BF).to(DEV)
    obs = torch.randn(B, T, D, generator=g).to(DEV)
    want = DDIMSampler(bench_model, S).sample(xT, steps=3)
    smp = ConditionalDDIMSampler(bench_model, S, use_graph=False)
    with hip.record_launches() as rec:
        got = smp.sample(xT, obs, torch.zeros(T, D, dtype=torch.bool), steps=3)
        torch.cuda.synchronize()
    assert torch.equal(got, want)
    fam = {hip.PATH_NAMES[pth] for (name, _), pth in zip(rec.calls, rec.paths) if pth}
    names = [n for n, _ in rec.calls]
    assert names.count("ib_ddim_cond_step") == 3 and names.count("ib_ddim_cond_init") == 1
    assert "ib_ddim_step" not in names
    if B <= 32:
        assert {"linear_ln_panel", "ffn_infer"} <= fam, fam
        assert ("linear_panel" in fam) == (B * T <= 1600), (B, fam)
    else:
        assert "ffn_chain" in fam and "ib_ffn_chain_fwd_infer" in names, (fam, sorted(set(names)))
        assert {"linear_ln_panel", "ffn_infer"} <= fam, fam
        assert names.count("ib_ffn_chain_fwd_infer") == 4 * 3 and names.count("ib_ffn_infer_fwd") == 4 * 3


# ---------------------------------------------------------------------------------------------------------------------
# 3. full mask: the observation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, BF])
def test_full_mask_returns_the_observation(dt):
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler
    model = small_models(dt)["transformer"]
    B, T, D, S = 3, 24, 44, 10
    xT = R.det_fill((B, T, D), 13, 1.0, torch.float32)
    obs = R.det_fill((B, T, D), 14, 2.0, torch.float32)
    got = ConditionalDDIMSampler(model, S).sample(xT.to(DEV), obs.to(DEV), torch.ones(T, D, dtype=torch.bool))
    assert got.dtype == dt and torch.equal(got.cpu(), obs.to(dt))


# ---------------------------------------------------------------------------------------------------------------------
# 4. / 5. label inference against the float64 masked loop
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,rt", [(torch.float32, 2e-3), (BF, 4e-2)])
@pytest.mark.parametrize("kind", ["mlp", "transformer"])
def test_label_inference_loop_matches_float64(dt, rt, kind):
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler
    model = small_models(dt)[kind]
    B, T, D, S = 3, 24, 44, 10
    xT = R.det_fill((B, T, D), 11, 1.0, torch.float32).to(dt)
    obs = R.det_fill((B, T, D), 15, 1.0, torch.float32).to(dt)
    m = label_mask(T, D)
    got = ConditionalDDIMSampler(model, S).sample(xT.to(DEV), obs.to(DEV), m)
    p = params64(model)
    if kind == "mlp":
        fn = lambda x, t: R.denoiser_mlp_forward(p, x, t, [64, 64])
    else:
        fn = lambda x, t: R.denoiser_transformer_forward(p, x, t, 2, 2)
    with torch.no_grad():
        want = masked_loop64(fn, obs.double(), xT.double(), m, S)
    close(got[:, :, D - 30:], want[:, :, D - 30:], rt, "inferred label columns")
    assert torch.equal(got.cpu()[:, m], obs[:, m]), "observed elements must equal the observation"


def test_long_fp32_label_inference_matches_float64():
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    B, T, D, S = 1, 200, 177, 100
    model = DiffusionTransformer(D, T, d_model=128, num_heads=2, dim_feedforward=256, num_layers=2, device=DEV)
    load_det(model)
    xT = R.det_fill((B, T, D), 16, 1.0, torch.float32)
    obs = R.det_fill((B, T, D), 17, 1.0, torch.float32)
    m = label_mask(T, D)
    got = ConditionalDDIMSampler(model, S).sample(xT.to(DEV), obs.to(DEV), m)
    p = params64(model)
    with torch.no_grad():
        want = masked_loop64(lambda x, t: R.denoiser_transformer_forward(p, x, t, 2, 2), obs.double(), xT.double(), m, S)
    close(got, want, 2e-3, "x_0 after 100 steps")
    assert torch.equal(got.cpu()[:, m], obs[:, m])


# ---------------------------------------------------------------------------------------------------------------------
# 6. the captured step is replayed for a new batch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, BF])
def test_second_batch_replays_the_captured_step(dt):
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler
    model = small_models(dt)["transformer"]
    B, T, D, S = 3, 24, 44, 10
    z1, z2 = (R.det_fill((B, T, D), k, 1.0, torch.float32).to(DEV) for k in (21, 22))
    o1, o2 = (R.det_fill((B, T, D), k, 1.0, torch.float32).to(DEV) for k in (23, 24))
    m1, m2 = label_mask(T, D), label_mask(T, D, free=12)
    smp = ConditionalDDIMSampler(model, S)
    a = smp.sample(z1, o1, m1)
    graph = smp._graph
    assert graph is not None
    b = smp.sample(z2, o2, m2)
    assert smp._graph is graph, "a batch of the same shape must replay the captured step"
    assert torch.equal(a, ConditionalDDIMSampler(model, S).sample(z1, o1, m1))
    assert torch.equal(b, ConditionalDDIMSampler(model, S).sample(z2, o2, m2))
    assert not torch.equal(a, b)
    # the device draw (sample_noise) is the drawn x_T of DDIMSampler.sample_noise
    zs = smp.draw_start(B, T, D, seed=7, draw=3)
    assert torch.equal(smp.sample_noise(B, T, D, o1, m1, seed=7, draw=3), ConditionalDDIMSampler(model, S).sample(zs, o1, m1))
