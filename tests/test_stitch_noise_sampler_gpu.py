"""StochasticStitchedSampler on the GPU: one window against ConditionalDDIMSampler(eta) and eta = 0 against
StitchedDDIMSampler (bit for bit), overlapping windows (captured graph against eager launches, replay with new trial ids), the
fp32 loop against a float64 restatement, and DiffusionLabelPredictor.predict_trial_ensemble.  The bf16 denoiser of
tests/test_stitch_sampler_gpu.py (44 columns in rows padded to the plan's pitch) and the fp32 transformer of
tests/test_eta_sampler_gpu.py.  -m gpu."""
import pytest
import torch

from oracle import ref_cpu as R
from tests.test_eta_sampler_gpu import GEN_TOL, loop64, params64, small_models
from tests.test_stitch_sampler_gpu import C, D, N, T, cols, draws, load_det

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
S = 5
NAME = "ib_stitch_ddim_step_noise"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from inferbiomechanics_amd import hip
    hip.lib()


@pytest.fixture(scope="module")
def model():
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    m = DiffusionTransformer(D, T, d_model=128, num_heads=2, dim_feedforward=256, num_layers=2, device=DEV, compute_dtype=BF)
    load_det(m)
    return m


@pytest.mark.parametrize("eta", [0.5, 1.0])
def test_one_window_is_the_conditional_sampler(model, eta):
    from inferbiomechanics_amd.diffusion import ConditionalDDIMSampler, DDIMSampler, StochasticStitchedSampler
    z, obs = draws(T, 1)
    ids = [7, 2 ** 32 - 1]
    ref = ConditionalDDIMSampler(model, S, eta=eta, seed=31).sample(z, obs, cols()[None, :].expand(T, D).contiguous(),
                                                                    window_ids=ids)
    st = StochasticStitchedSampler(model, S, eta=eta, seed=31)
    got = st.sample(z, obs, cols(), trial_ids=ids)
    Dp = st._bufs["x"].shape[-1]
    assert st._bufs["x"].shape == (N, T, Dp) and Dp > D and Dp % 8 == 0 and "eps" in st._bufs, "the pitched state"
    assert got.shape == (N, T, D) and torch.equal(got, ref)
    assert not torch.equal(got, st.sample(z, obs, cols()))             # ids 0, 1: another trajectory
    # without observations: DDIMSampler(eta)
    assert torch.equal(StochasticStitchedSampler(model, S, eta=eta, seed=31).sample(z, trial_ids=ids),
                       DDIMSampler(model, S, eta=eta, seed=31).sample(z, window_ids=ids))


def test_eta_zero_is_the_deterministic_stitched_sampler(model):
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion import StitchedDDIMSampler, StochasticStitchedSampler
    z, obs = draws(2 * T, 2)
    want = StitchedDDIMSampler(model, S, hop=T // 2).sample(z, obs, cols())
    with hip.record_launches() as rec:
        got = StochasticStitchedSampler(model, S, eta=0.0, hop=T // 2, seed=9).sample(z, obs, cols(), trial_ids=[4, 5])
        torch.cuda.synchronize()
    assert torch.equal(got, want) and NAME not in [n for n, _ in rec.calls]
    assert torch.equal(StochasticStitchedSampler(model, S, eta=0.0, hop=T // 2).sample(z),
                       StitchedDDIMSampler(model, S, hop=T // 2).sample(z))


@pytest.mark.parametrize("eta", [0.5, 1.0])
def test_overlapping_windows(model, eta):
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion import StochasticStitchedSampler
    F = 2 * T
    z, obs = draws(F, 3)
    graph = StochasticStitchedSampler(model, S, eta=eta, hop=T // 2, seed=5)
    eager = StochasticStitchedSampler(model, S, eta=eta, hop=T // 2, seed=5, use_graph=False)
    with hip.record_launches() as rec:
        want = eager.sample(z, obs, cols())
        torch.cuda.synchronize()
    names = [n for n, _ in rec.calls]
    assert names.count(NAME) == S and not [n for n in names if n.endswith(("ddim_step", "ddim_cond_step", "dpmpp_step",
                                                                           "dpmpp_cond_step", "cond_step_noise"))]
    got = graph.sample(z, obs, cols())
    assert graph.layout["W"] == 3 and graph._graph is not None and eager._graph is None
    assert got.shape == (N, F, D) and bool(torch.isfinite(got).all())
    assert torch.equal(got[..., :C], obs[..., :C].to(BF)), "observed columns must equal the observation"
    assert torch.equal(got, want), "captured graph and eager launches disagree"
    g0 = graph._graph
    other = graph.sample(z, obs, cols(), trial_ids=[8, 9])
    assert graph._graph is g0, "new trial ids of the same shape replay the captured step"
    assert not torch.equal(other, got) and torch.equal(other[..., :C], got[..., :C])
    assert torch.equal(other, eager.sample(z, obs, cols(), trial_ids=[8, 9]))
    again = graph.sample(z, obs, cols(), trial_ids=[0, 1])
    assert graph._graph is g0 and torch.equal(again, got), "the same ids give the same result"
    assert not torch.equal(StochasticStitchedSampler(model, S, eta=eta, hop=T // 2, seed=6).sample(z, obs, cols()), got)
    # without observations: the unconditional loop of the same class
    a = StochasticStitchedSampler(model, S, eta=eta, hop=T // 2, seed=5).sample(z)
    b = StochasticStitchedSampler(model, S, eta=eta, hop=T // 2, seed=5, use_graph=False).sample(z)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


@pytest.mark.parametrize("eta", [0.5, 1.0])
def test_fp32_loop_matches_float64(eta):
    """The stitched loop restated in float64: loop64 of tests/test_eta_sampler_gpu.py over the TRIAL ([N, F, D], normals
    indexed by trial frame), its denoiser the oracle transformer on the W = 3 windows with the blend of their predictions.
    That test's tolerance, 2e-3 of the largest value + 2e-5 sum_s sigma_s: the blend is a convex combination and does not
    amplify."""
    from inferbiomechanics_amd.diffusion import StochasticStitchedSampler
    from inferbiomechanics_amd.diffusion.schedule import stitch_layout
    mdl = small_models()["transformer"]
    Nn, Tt, Dd, Ff, steps, seed = 2, 24, 44, 48, 10, 12345
    ids = [11, 2 ** 32 - 2]
    start, cover, wn, _ = stitch_layout(Ff, Tt, Tt // 2, "ramp")
    W = start.numel()
    assert W == 3
    gather = start.long()[:, None] + torch.arange(Tt)[None, :]
    p = params64(mdl)

    def eps_fn(x, t):                                                  # x [N, F, D] -> the blended prediction [N, F, D]
        xw = x[:, gather].reshape(Nn * W, Tt, Dd)
        ew = R.denoiser_transformer_forward(p, xw, t[:1].expand(Nn * W), 2, 2).view(Nn, W, Tt, Dd)
        out = torch.zeros_like(x)
        for f in range(Ff):
            w0, cnt = cover[f].tolist()
            for k in range(cnt):
                out[:, f] += float(wn[f, k]) * ew[:, w0 + k, f - int(start[w0 + k])]
        return out

    xT = R.det_fill((Nn, Ff, Dd), 11, 1.0, torch.float32)
    obs = R.det_fill((Nn, Ff, Dd), 15, 1.0, torch.float32)
    mc = torch.ones(Dd, dtype=torch.bool)
    mc[Dd - 30:] = False
    m = mc[None, :].expand(Ff, Dd)
    for cond in (False, True):
        smp = StochasticStitchedSampler(mdl, steps, eta=eta, seed=seed)
        got = smp.sample(xT.to(DEV), *((obs.to(DEV), mc) if cond else ()), trial_ids=ids)
        assert smp.layout["W"] == W
        with torch.no_grad():
            want, sig_sum = loop64(eps_fn, xT.double(), steps, eta, seed, ids, obs.double() if cond else None, m if cond else None)
        err = float((got.cpu().double() - want).abs().max())
        tol = 2e-3 * float(want.abs().max()) + GEN_TOL * sig_sum
        print(f"stitched eta={eta} cond={cond}: max err {err:.3e} (tol {tol:.3e}, sum sigma {sig_sum:.3f})")
        assert torch.isfinite(got).all() and err <= tol, (cond, err, tol)
        if cond:
            assert torch.equal(got.cpu()[..., mc], obs[..., mc]), "observed elements must equal the observation"


def test_predict_trial_ensemble():
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import LOSS_KEY_ORDER, LOSS_KEY_WIDTHS, SyntheticWindowDataset
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    from inferbiomechanics_amd.models.DiffusionLabelPredictor import DiffusionLabelPredictor
    m = DiffusionTransformer(177, 10, d_model=128, num_heads=2, dim_feedforward=256, num_layers=2, device=DEV, compute_dtype=BF)
    load_det(m)
    ds = SyntheticWindowDataset(4, 50, 5)                              # windows of 10 frames
    items = [ds[i] for i in range(4)]
    inputs = {k: torch.stack([torch.cat([items[2 * n][0][k], items[2 * n + 1][0][k]]) for n in range(2)]).to(DEV)
              for k in items[0][0]}                                    # [2, 20, c]
    K, draw = 3, 2
    pred = DiffusionLabelPredictor(m, S, seed=3, eta=1.0, num_samples=K)
    out = pred.predict_trial_ensemble(inputs, hop=4, draw=draw)
    std = pred.last_std
    assert list(out) == LOSS_KEY_ORDER and list(std) == LOSS_KEY_ORDER
    for k, w in zip(LOSS_KEY_ORDER, LOSS_KEY_WIDTHS):
        assert out[k].shape == std[k].shape == (2, 20, w) and out[k].dtype == std[k].dtype == torch.float32
        assert bool(torch.isfinite(out[k]).all()) and bool(torch.isfinite(std[k]).all()) and bool((std[k] >= 0).all())
        assert bool((std[k] > 0).any()), k
    again = pred.predict_trial_ensemble(inputs, hop=4, draw=draw)      # the captured step replayed: the same ensemble
    for k in LOSS_KEY_ORDER:
        assert torch.equal(again[k], out[k])
    # the mean of K = 3 members = the mean of three K = 1 calls with the members' trial ids, summed in member order
    single = DiffusionLabelPredictor(m, S, seed=3, eta=1.0)
    for b in range(2):
        one = {k: v[b:b + 1] for k, v in inputs.items()}
        members = [single.predict_trial_ensemble(one, hop=4, draw=(draw + b) * K + j) for j in range(K)]
        assert not any(bool(v.any()) for v in single.last_std.values()), "one member has no spread"
        for k in LOSS_KEY_ORDER:
            # a K = 1 call returns its member's values exactly (fp32 of the bf16 state), so the three members reduced by the
            # same kernel, in member order, with its division, must give the ensemble's mean and spread bit for bit
            stack = torch.stack([mem[k] for mem in members], dim=1).contiguous()
            assert stack.shape == (1, K, 20, out[k].shape[-1]) and stack.dtype == torch.float32
            want_mean, want_std = hip.ensemble_stats(stack)
            assert torch.equal(out[k][b:b + 1], want_mean), (b, k, "mean")
            assert torch.equal(std[k][b:b + 1], want_std), (b, k, "std")
            swapped = hip.ensemble_stats(stack[:, [2, 1, 0]].contiguous())[0]
            print(f"trial {b} {k}: {int((swapped != want_mean).sum())} elements of the mean depend on the member order")
            assert not torch.equal(members[0][k], members[1][k])
    with pytest.raises(ValueError, match="eta"):
        pred.predict_trial(inputs)
