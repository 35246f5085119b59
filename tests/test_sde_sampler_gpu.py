"""solver 'dpmpp2m_sde' through the sampler classes on the GPU: eta = 0 against 'dpmpp2m' (bit for bit), the captured graph
against eager launches, one window against ConditionalDDIMSampler with window ids = trial ids, the trial ids, the masked loop's
last step in both observation modes, two samplers sharing one model's tables, and predict_trial_ensemble.  The small denoiser
of tests/test_stitch_sampler_gpu.py (44 columns; in bf16 the rows are padded to the plan's pitch), in fp32 and bf16.  -m gpu."""
import pytest
import torch

from tests.test_stitch_sampler_gpu import C, D, N, T, cols, draws, load_det

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
S = 5
NAME = "ib_sde_dpmpp_step"
SDE = dict(solver="dpmpp2m_sde", spacing="logsnr")
# the update launches of every other loop
OTHERS = ("ib_stitch_ddim_step", "ib_stitch_dpmpp_step", "ib_stitch_ddim_step_noise", "ib_ddim_step", "ib_ddim_cond_step",
          "ib_ddim_step_noise", "ib_ddim_cond_step_noise", "ib_dpmpp_step", "ib_dpmpp_cond_step")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from inferbiomechanics_amd import hip
    hip.lib()


@pytest.fixture(scope="module", params=[torch.float32, BF], ids=["fp32", "bf16"])
def model(request):
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    m = DiffusionTransformer(D, T, d_model=128, num_heads=2, dim_feedforward=256, num_layers=2, device=DEV,
                             compute_dtype=request.param)
    load_det(m)
    return m


def frame_mask():
    return cols()[None, :].expand(T, D).contiguous()


def test_eta_zero_is_dpmpp2m_in_every_class(model):
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion import ConditionalDDIMSampler, DDIMSampler, StitchedDDIMSampler, StochasticStitchedSampler
    z, obs = draws(T, 1)
    zt, obst = draws(2 * T, 2)
    base = dict(solver="dpmpp2m", spacing="logsnr")
    with hip.record_launches() as rec:
        a = DDIMSampler(model, S, eta=0.0, **SDE).sample(z)
        b = ConditionalDDIMSampler(model, S, eta=0.0, **SDE).sample(z, obs, frame_mask())
        c = StitchedDDIMSampler(model, S, hop=T // 2, **SDE).sample(zt, obst, cols())
        d = StochasticStitchedSampler(model, S, eta=0.0, hop=T // 2, **SDE).sample(zt, obst, cols(), trial_ids=[4, 5])
        torch.cuda.synchronize()
    assert NAME not in [n for n, _ in rec.calls]
    assert torch.equal(a, DDIMSampler(model, S, **base).sample(z))
    assert torch.equal(b, ConditionalDDIMSampler(model, S, **base).sample(z, obs, frame_mask()))
    want = StitchedDDIMSampler(model, S, hop=T // 2, **base).sample(zt, obst, cols())
    assert torch.equal(c, want) and torch.equal(d, want)


@pytest.mark.parametrize("eta", [0.5, 1.0])
def test_graph_replay_equals_eager_per_window(model, eta):
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion import ConditionalDDIMSampler, DDIMSampler
    z, obs = draws(T, 3)
    ids = [7, 2 ** 32 - 1]
    for cls, extra in ((DDIMSampler, ()), (ConditionalDDIMSampler, (obs, frame_mask()))):
        graph = cls(model, S, eta=eta, seed=31, **SDE)
        eager = cls(model, S, eta=eta, seed=31, use_graph=False, **SDE)
        with hip.record_launches() as rec:
            want = eager.sample(z, *extra, window_ids=ids)
            torch.cuda.synchronize()
        names = [n for n, _ in rec.calls]
        assert names.count(NAME) == S and not [n for n in names if n in OTHERS]
        got = graph.sample(z, *extra, window_ids=ids)
        assert graph._graph is not None and eager._graph is None
        assert bool(torch.isfinite(got).all()) and torch.equal(got, want), cls.__name__
        g0 = graph._graph
        other = graph.sample(z, *extra, window_ids=[8, 9])
        assert graph._graph is g0 and not torch.equal(other, got)
        assert torch.equal(other, eager.sample(z, *extra, window_ids=[8, 9]))
        assert torch.equal(graph.sample(z, *extra, window_ids=ids), got) and graph._graph is g0


@pytest.mark.parametrize("eta", [0.5, 1.0])
def test_one_window_is_the_conditional_sampler(model, eta):
    from inferbiomechanics_amd.diffusion import ConditionalDDIMSampler, DDIMSampler, StochasticStitchedSampler
    z, obs = draws(T, 1)
    ids = [7, 2 ** 32 - 1]
    ref = ConditionalDDIMSampler(model, S, eta=eta, seed=31, **SDE).sample(z, obs, frame_mask(), window_ids=ids)
    st = StochasticStitchedSampler(model, S, eta=eta, seed=31, **SDE)
    got = st.sample(z, obs, cols(), trial_ids=ids)
    assert got.shape == (N, T, D) and torch.equal(got, ref)
    assert not torch.equal(got, st.sample(z, obs, cols()))             # ids 0, 1: another trajectory
    assert torch.equal(StochasticStitchedSampler(model, S, eta=eta, seed=31, **SDE).sample(z, trial_ids=ids),
                       DDIMSampler(model, S, eta=eta, seed=31, **SDE).sample(z, window_ids=ids))
    # not the first-order loop of the same eta and keys
    assert not torch.equal(got, StochasticStitchedSampler(model, S, eta=eta, seed=31, spacing="logsnr").sample(
        z, obs, cols(), trial_ids=ids))


@pytest.mark.parametrize("eta", [0.5, 1.0])
def test_overlapping_windows_and_trial_ids(model, eta):
    """what tests/test_stitch_noise_sampler_gpu.py::test_overlapping_windows asserts for the DDIM loop"""
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion import StochasticStitchedSampler
    F = 2 * T
    z, obs = draws(F, 3)
    dt = model.compute_dtype
    graph = StochasticStitchedSampler(model, S, eta=eta, hop=T // 2, seed=5, **SDE)
    eager = StochasticStitchedSampler(model, S, eta=eta, hop=T // 2, seed=5, use_graph=False, **SDE)
    with hip.record_launches() as rec:
        want = eager.sample(z, obs, cols())
        torch.cuda.synchronize()
    names = [n for n, _ in rec.calls]
    assert names.count(NAME) == S and not [n for n in names if n in OTHERS]
    got = graph.sample(z, obs, cols())
    assert graph.layout["W"] == 3 and graph._graph is not None and eager._graph is None
    assert got.shape == (N, F, D) and bool(torch.isfinite(got).all())
    assert torch.equal(got[..., :C], obs[..., :C].to(dt)), "observed columns must equal the observation"
    assert torch.equal(got, want), "captured graph and eager launches disagree"
    g0 = graph._graph
    other = graph.sample(z, obs, cols(), trial_ids=[8, 9])
    assert graph._graph is g0, "new trial ids of the same shape replay the captured step"
    assert not torch.equal(other, got) and torch.equal(other[..., :C], got[..., :C])
    assert torch.equal(other, eager.sample(z, obs, cols(), trial_ids=[8, 9]))
    again = graph.sample(z, obs, cols(), trial_ids=[0, 1])
    assert graph._graph is g0 and torch.equal(again, got), "the same ids give the same result"
    assert not torch.equal(StochasticStitchedSampler(model, S, eta=eta, hop=T // 2, seed=6, **SDE).sample(z, obs, cols()), got)
    # without observations: the unconditional loop of the same class
    a = StochasticStitchedSampler(model, S, eta=eta, hop=T // 2, seed=5, **SDE).sample(z)
    b = StochasticStitchedSampler(model, S, eta=eta, hop=T // 2, seed=5, use_graph=False, **SDE).sample(z)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


@pytest.mark.parametrize("observations", ["noised", "clean"])
def test_masked_loop_ends_on_the_observation(model, observations):
    from inferbiomechanics_amd.diffusion import ConditionalDDIMSampler, StochasticStitchedSampler
    dt = model.compute_dtype
    z, obs = draws(T, 5)
    zt, obst = draws(2 * T, 6)
    old = getattr(model, "cond_cols", 0)
    model.cond_cols = C if observations == "clean" else 0
    try:
        for eta in (0.5, 1.0):
            got = ConditionalDDIMSampler(model, S, eta=eta, seed=3, observations=observations, **SDE).sample(z, obs, frame_mask())
            assert torch.equal(got[..., :C], obs[..., :C].to(dt)) and bool(torch.isfinite(got).all())
            got = StochasticStitchedSampler(model, S, eta=eta, hop=T // 2, seed=3, observations=observations, **SDE).sample(
                zt, obst, cols())
            assert torch.equal(got[..., :C], obst[..., :C].to(dt)) and bool(torch.isfinite(got).all())
    finally:
        model.cond_cols = old


def test_two_samplers_on_one_model_leave_each_other_alone(model):
    """one model's tables are shared by all its samplers, and the first-order (r, q) table differs from the new solver's at
    eta = 0.5: called alternately, each must keep giving what it gives alone"""
    from inferbiomechanics_amd.diffusion import ConditionalDDIMSampler
    z, obs = draws(T, 7)
    ids = [3, 9]
    alone_first = ConditionalDDIMSampler(model, S, eta=0.5, seed=2, spacing="logsnr").sample(z, obs, frame_mask(), window_ids=ids)
    alone_new = ConditionalDDIMSampler(model, S, eta=0.5, seed=2, **SDE).sample(z, obs, frame_mask(), window_ids=ids)
    assert not torch.equal(alone_first, alone_new)
    first = ConditionalDDIMSampler(model, S, eta=0.5, seed=2, spacing="logsnr")
    new = ConditionalDDIMSampler(model, S, eta=0.5, seed=2, **SDE)
    for _ in range(2):
        assert torch.equal(first.sample(z, obs, frame_mask(), window_ids=ids), alone_first)
        assert torch.equal(new.sample(z, obs, frame_mask(), window_ids=ids), alone_new)
    tabs = model.tables(model._flat.device)                            # the tables the samplers read, as they look them up
    assert tabs.sde_obs_noise_coef is not None and tabs.obs_noise_coef is None


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
    K = 3
    pred = DiffusionLabelPredictor(m, S, seed=3, eta=0.5, num_samples=K, **SDE)
    with hip.record_launches() as rec:
        out = pred.predict_trial_ensemble(inputs, hop=4, draw=2)
        torch.cuda.synchronize()
    assert NAME in [n for n, _ in rec.calls] and "ib_stitch_ddim_step_noise" not in [n for n, _ in rec.calls]
    std = pred.last_std
    assert list(out) == LOSS_KEY_ORDER and list(std) == LOSS_KEY_ORDER
    for k, w in zip(LOSS_KEY_ORDER, LOSS_KEY_WIDTHS):
        assert out[k].shape == std[k].shape == (2, 20, w) and out[k].dtype == std[k].dtype == torch.float32
        assert bool(torch.isfinite(out[k]).all()) and bool(torch.isfinite(std[k]).all()) and bool((std[k] >= 0).all())
        assert bool((std[k] > 0).any()), k                             # the label columns are free: the members differ
    again = pred.predict_trial_ensemble(inputs, hop=4, draw=2)
    for k in LOSS_KEY_ORDER:
        assert torch.equal(again[k], out[k])
