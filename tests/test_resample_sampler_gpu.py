"""RePaint resampling through the samplers on the GPU (diffusion/sampler.py over csrc/resample.hip).  -m gpu.

The small denoiser of tests/test_stitch_sampler_gpu.py (D = 44, T = 24, S = 5) in bf16 (the pitched state, 8-wide kernels) and
fp32 (no pitch, element-wise kernels), resample = (2, 2): 9 denoiser evaluations and 2 jumps per call.  Captured graph
against eager launches bit for bit, the launch names and counts, observed columns, what the result depends on, one-window
trials against the per-window sampler, overlapping windows, 'clean' observations and a guided call, resampling off against
today's sampler, the predictor's eta = 0 ensemble -- and the 2-D Gaussian problem of docs/EXPERIMENTS.md through the real
kernels: the resampled loop removes most of the bias of the plain one."""
import pytest
import torch

from tests import resample_restatement as RR
from tests.test_stitch_sampler_gpu import load_det

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
N, T, D, S, C = 2, 24, 44, 5, 14
RES = (2, 2)
NAME = "ib_resample_renoise"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from inferbiomechanics_amd import hip
    hip.lib()


_MODELS = {}


@pytest.fixture(params=[BF, torch.float32], ids=["bf16", "fp32"])
def model(request):
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    dt = request.param
    if dt not in _MODELS:
        m = DiffusionTransformer(D, T, d_model=128, num_heads=2, dim_feedforward=256, num_layers=2, device=DEV, compute_dtype=dt)
        load_det(m)
        _MODELS[dt] = m
    return _MODELS[dt]


def draws(F, seed, n=N):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, F, D, generator=g).to(DEV), torch.randn(n, F, D, generator=g).to(DEV)


def cols():
    c = torch.zeros(D, dtype=torch.bool)
    c[:C] = True
    return c


def mask():
    return cols()[None, :].expand(T, D).contiguous()


def test_graph_against_eager_names_and_what_the_result_depends_on(model):
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion import ConditionalDDIMSampler
    dt = model.compute_dtype
    z, obs = draws(T, 1)
    graph = ConditionalDDIMSampler(model, S, seed=5, resample=RES)
    eager = ConditionalDDIMSampler(model, S, seed=5, resample=RES, use_graph=False)
    with hip.record_launches() as rec:
        want = eager.sample(z, obs, mask(), window_ids=[7, 3])
    names = [n for n, _ in rec.calls]
    seq = [n for n in names if n in ("ib_ddim_cond_step", NAME, "ib_counter_add")]
    step, jump = ["ib_ddim_cond_step", "ib_counter_add"], [NAME, "ib_counter_add"]
    assert seq == 3 * step + jump + 4 * step + jump + 2 * step, "the launch sequence is resample_walk(5, 2, 2)"
    assert not [n for n in names if n.endswith(("_step", "_step_noise")) and n != "ib_ddim_cond_step"]
    got = graph.sample(z, obs, mask(), window_ids=[7, 3])
    assert graph._graph is not None and eager._graph is None
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got[..., :C], obs[..., :C].to(dt)), "observed columns must equal the observation"
    assert torch.equal(got, want), "captured graph and eager launches disagree"
    # the same ids: the same result, from the same capture; other ids, seeds: another one, on the free columns only
    g0 = graph._graph
    assert torch.equal(graph.sample(z, obs, mask(), window_ids=[7, 3]), got) and graph._graph is g0
    other = graph.sample(z, obs, mask(), window_ids=[7, 4])
    assert graph._graph is g0, "new ids replay the captured step"
    assert torch.equal(other[0], got[0]) and not torch.equal(other[1, :, C:], got[1, :, C:])
    assert torch.equal(other[..., :C], got[..., :C])
    # the result depends on (seed, id), not on the place in the batch
    flip = graph.sample(z.flip(0), obs.flip(0), mask(), window_ids=[3, 7])
    assert torch.equal(flip.flip(0), got), "a window's result must not depend on its batch position"
    reseed = ConditionalDDIMSampler(model, S, seed=6, resample=RES).sample(z, obs, mask(), window_ids=[7, 3])
    assert not torch.equal(reseed[..., C:], got[..., C:]) and torch.equal(reseed[..., :C], got[..., :C])
    # a plain loop from the same start is another trajectory: the jumps did something
    plain = ConditionalDDIMSampler(model, S, seed=5).sample(z, obs, mask())
    assert not torch.equal(plain[..., C:], got[..., C:])
    # steps= truncates after that many evaluations
    with hip.record_launches() as rec:
        eager.sample(z, obs, mask(), steps=4)
    names = [n for n, _ in rec.calls]
    assert names.count("ib_ddim_cond_step") == 4 and names.count(NAME) == 1


def test_off_is_todays_sampler_and_settings_change_on_one_capture(model):
    from inferbiomechanics_amd.diffusion import ConditionalDDIMSampler
    z, obs = draws(T, 2)
    today = ConditionalDDIMSampler(model, S, seed=5).sample(z, obs, mask())
    assert torch.equal(ConditionalDDIMSampler(model, S, seed=5, resample=None).sample(z, obs, mask()), today)
    assert torch.equal(ConditionalDDIMSampler(model, S, seed=5, resample=(2, 1)).sample(z, obs, mask()), today), "times = 1"
    smp = ConditionalDDIMSampler(model, S, seed=5, resample=RES)
    on = smp.sample(z, obs, mask())
    g0, sig = smp._graph, smp._sig
    smp.resample = None
    assert torch.equal(smp.sample(z, obs, mask()), today), "resampling turned off on a used sampler"
    smp.resample = (1, 3)
    other = smp.sample(z, obs, mask())
    assert torch.equal(other, ConditionalDDIMSampler(model, S, seed=5, resample=(1, 3)).sample(z, obs, mask()))
    smp.resample = RES
    assert torch.equal(smp.sample(z, obs, mask()), on) and not torch.equal(on, other)
    assert smp._graph is g0 and smp._sig == sig, "the step did not change: it is not captured again"


def test_one_window_trials_equal_the_per_window_sampler(model):
    """In fp32 the state is not pitched (ld = 44, no multiple of 8) and its buffers are aligned: the one geometry in which
    include/ib_hip_stitch.h states that ib_stitch_ddim_step does NOT equal ib_ddim_cond_step (the per-window kernel goes
    8-wide and rounds an observed element by its flat offset, the stitched one element-wise by column; with these shapes
    the PLAIN loops of the two classes differ in 471 of 2112 elements by at most 1.5e-5).  A resampled loop over one-window
    trials therefore updates with the per-window entry (DDIMSampler._one_window_step), and is equal at either pitch."""
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion import ConditionalDDIMSampler, StochasticStitchedSampler
    z, obs = draws(T, 3)
    ref = ConditionalDDIMSampler(model, S, seed=5, resample=RES).sample(z, obs, mask(), window_ids=[9, 4])
    st = StochasticStitchedSampler(model, S, eta=0.0, seed=5, resample=RES)
    got = st.sample(z, obs, cols(), trial_ids=[9, 4])
    print(f"{model.compute_dtype}: {int((got != ref).sum())} of {got.numel()} elements differ, max "
          f"{float((got.double() - ref.double()).abs().max()):.3e} at max |value| {float(ref.abs().max()):.1f}")
    assert st.layout["W"] == 1 and torch.equal(got, ref)
    with hip.record_launches() as rec:
        st.use_graph, st._graph = False, None
        again = st.sample(z, obs, cols(), trial_ids=[9, 4])
    names = [n for n, _ in rec.calls]
    assert names.count("ib_ddim_cond_step") == 9 and "ib_stitch_ddim_step" not in names and torch.equal(again, ref)
    # the setting goes off on the same object: the stitched entry again, captured anew, today's result
    st.use_graph, st.resample = True, None
    plain = st.sample(z, obs, cols())
    assert "one_window_step" not in st._sig
    assert torch.equal(plain, StochasticStitchedSampler(model, S, eta=0.0, seed=5).sample(z, obs, cols()))


def test_overlapping_windows_keep_their_copies_equal(model):
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion import StochasticStitchedSampler
    from inferbiomechanics_amd.diffusion.sampler import _cut, _join
    dt = model.compute_dtype
    F = 2 * T
    z, obs = draws(F, 4)
    graph = StochasticStitchedSampler(model, S, eta=0.0, hop=T // 2, seed=5, resample=RES)
    eager = StochasticStitchedSampler(model, S, eta=0.0, hop=T // 2, seed=5, resample=RES, use_graph=False)
    with hip.record_launches() as rec:
        want = eager.sample(z, obs, cols(), trial_ids=[11, 2])
    names = [n for n, _ in rec.calls]
    assert names.count("ib_stitch_ddim_step") == 9 and names.count(NAME) == 2
    got = graph.sample(z, obs, cols(), trial_ids=[11, 2])
    lay = graph.layout
    assert lay["W"] == 3 and got.shape == (N, F, D) and bool(torch.isfinite(got).all())
    assert torch.equal(got, want), "captured graph and eager launches disagree"
    assert torch.equal(got[..., :C], obs[..., :C].to(dt))
    x = graph._bufs["x"]
    assert torch.equal(x, _cut(lay, _join(lay, x, N))), "the copies came apart"
    # a jump alone, from consistent copies, leaves them consistent (the state mid-loop, right after the first jump)
    mid = eager.sample(z, obs, cols(), steps=4, trial_ids=[11, 2])
    x = eager._bufs["x"]
    assert torch.equal(x, _cut(lay, _join(lay, x, N))) and bool(torch.isfinite(mid).all())
    flip = graph.sample(z.flip(0), obs.flip(0), cols(), trial_ids=[2, 11])
    assert torch.equal(flip.flip(0), got), "a trial's result must not depend on its batch position"


def test_clean_observations_and_guided_call():
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion import ConditionalDDIMSampler
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    m = DiffusionTransformer(D, T, d_model=128, num_heads=2, dim_feedforward=256, num_layers=2, device=DEV, compute_dtype=BF)
    load_det(m)
    m.cond_cols, m.cond_drop = C, 0.1
    z, obs = draws(T, 5)
    clean = ConditionalDDIMSampler(m, S, seed=5, observations="clean", resample=RES)
    got = clean.sample(z, obs, mask())
    assert bool(torch.isfinite(got).all()) and torch.equal(got[..., :C], obs[..., :C].to(BF))
    assert torch.equal(got, ConditionalDDIMSampler(m, S, seed=5, observations="clean", resample=RES, use_graph=False)
                       .sample(z, obs, mask()))
    guided = ConditionalDDIMSampler(m, S, seed=5, observations="clean", guidance=1.5, resample=RES)
    eager = ConditionalDDIMSampler(m, S, seed=5, observations="clean", guidance=1.5, resample=RES, use_graph=False)
    with hip.record_launches() as rec:
        want = eager.sample(z, obs, mask(), steps=4)                   # three steps, the first jump, one more step
    names = [n for n, _ in rec.calls]
    at = names.index(NAME)
    assert names[at:at + 3] == [NAME, "ib_counter_add", "ib_cfg_mirror"], "a jump is followed by the counter and the mirror"
    out = guided.sample(z, obs, mask())
    assert bool(torch.isfinite(out).all()) and torch.equal(out[..., :C], obs[..., :C].to(BF))
    assert not torch.equal(out[..., C:], got[..., C:]), "guidance changed the free columns"
    assert torch.equal(out, eager.sample(z, obs, mask()))
    # the twins carry the state of the first half: free columns and timesteps
    for smp in (guided, eager):
        xin, t = smp._bufs["xin"], smp._bufs["t"]
        assert torch.equal(xin[N:, :, C:D], xin[:N, :, C:D]) and torch.equal(t[N:], t[:N])
        assert not xin[N:, :, :C].any() and not xin[N:, :, D:].any(), "the null condition stays zero"
    # right after a jump (the eager loop stopped one step later): the mirror copied the re-noised columns, and the step that
    # followed saw the jump's timestep in both halves
    eager.sample(z, obs, mask(), steps=4)
    from inferbiomechanics_amd.diffusion.schedule import sample_timesteps
    t2 = int(sample_timesteps(1000, S)[2])
    assert bool((eager._bufs["t"] == t2).all()), "after step 0 1 2, jump 3 -> 1, step 1: both halves at t[2]"
    assert bool(torch.isfinite(want).all())


def test_predictor_ensemble_at_eta_zero():
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import LOSS_KEY_ORDER, LOSS_KEY_WIDTHS, SyntheticWindowDataset
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    from inferbiomechanics_amd.models.DiffusionLabelPredictor import DiffusionLabelPredictor
    m = DiffusionTransformer(177, 10, d_model=128, num_heads=2, dim_feedforward=256, num_layers=2, device=DEV, compute_dtype=BF)
    load_det(m)
    ds = SyntheticWindowDataset(4, 50, 5)                              # windows of 10 frames
    items = [ds[i] for i in range(2)]
    inputs = {k: torch.stack([it[0][k] for it in items]).to(DEV) for k in items[0][0]}
    pred = DiffusionLabelPredictor(m, S, seed=11, num_samples=3, resample=RES)
    out = pred(inputs, draw=2)
    std = pred.last_std
    for k, w in zip(LOSS_KEY_ORDER, LOSS_KEY_WIDTHS):
        assert out[k].shape == (2, 10, w) and bool(torch.isfinite(out[k]).all())
        assert std[k].shape == (2, 10, w) and float(std[k].min()) >= 0.0 and float(std[k].mean()) > 0.0, \
            "K = 3 members at eta = 0 differ: by their start draws and by their re-noise draws"
    again = pred(inputs, draw=2)
    for k in LOSS_KEY_ORDER:
        assert torch.equal(again[k], out[k]) and torch.equal(pred.last_std[k], std[k]), "reproducible"
    # a window's labels do not depend on batching: the second window alone, at its own draw
    alone = pred({k: v[1:] for k, v in inputs.items()}, draw=3)
    single = DiffusionLabelPredictor(m, S, seed=11, resample=RES)
    one = single(inputs, draw=2)
    assert single.last_std is not None and float(max(single.last_std[k].max() for k in LOSS_KEY_ORDER)) == 0.0, "K = 1: the id path"
    for k in LOSS_KEY_ORDER:
        assert alone[k].shape == (1, 10, LOSS_KEY_WIDTHS[LOSS_KEY_ORDER.index(k)]) and bool(torch.isfinite(one[k]).all())
    with pytest.raises(ValueError, match="predict_trial_ensemble"):
        single.predict_trial({k: torch.cat([v[0], v[1]])[None] for k, v in inputs.items()}, hop=4)
    trial = pred.predict_trial_ensemble({k: torch.cat([v[0], v[1]])[None] for k, v in inputs.items()}, hop=4)
    assert all(bool(torch.isfinite(trial[k]).all()) for k in LOSS_KEY_ORDER) and float(pred.last_std[LOSS_KEY_ORDER[1]].mean()) > 0.0


def test_gaussian_problem_through_the_kernels():
    """The 2-D Gaussian inpainting problem (correlation 0.9, the first coordinate observed at 1.5; the posterior of the second
    is N(1.35, 0.436^2)) with ib_ddim_cond_step and ib_resample_renoise doing the loop, fp32: 2048 one-window trials of T = 8
    frames, D = 2, every frame an independent pair (16 384 pairs); the analytic optimal denoiser is computed with torch here.
    S = 20, (jump 2, times 10).  The mean error of the resampled loop is at most 0.25 x that of the plain loop on the same
    start draws.  The float64 restatement gives 0.09 against 0.68 (tests/test_resample_plumbing_cpu.py); the standard error of
    a mean of 16 384 pairs is 0.004."""
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion import schedule as sch
    Nn, Tt, S_, corr, a = 2048, 8, 20, 0.9, 1.5
    jump, times = 2, 10
    dev = torch.device(DEV)
    tabs = sch.DiffusionTables(dev, num_sample_steps=S_)
    tabs.set_resample(jump)
    ab = sch.alphas_cumprod(1000)
    ts = tabs.ddim_t.tolist()
    start, cover = (t.to(dev) for t in sch.stitch_layout(Tt, Tt, Tt)[:2])
    ids = torch.arange(Nn, dtype=torch.int64, device=dev)
    m = torch.zeros(Tt, 2, dtype=torch.uint8, device=dev)
    m[:, 0] = 1
    z0 = torch.randn(Nn, Tt, 2, generator=torch.Generator().manual_seed(3)).to(dev)
    x0 = torch.zeros(Nn, Tt, 2, device=dev)
    x0[..., 0] = a

    def eps_of(x, level):
        q = level * corr                                               # cov of x_t: [[1, q], [q, 1]]
        s = (1.0 - level) ** 0.5 / (1.0 - q * q)
        return torch.stack([s * (x[..., 0] - q * x[..., 1]), s * (x[..., 1] - q * x[..., 0])], dim=-1).contiguous()

    def loop(walk):
        x, z = z0.clone(), z0.clone()
        hip.ddim_cond_init(x, x0, z, m, tabs.obs_coef, D=2)
        ctr = torch.zeros(1, dtype=torch.int32, device=dev)
        t_vec = torch.full((Nn,), ts[0], dtype=torch.int64, device=dev)
        evals = 0
        for op in walk:
            if op[0] == "step":
                hip.ddim_cond_step(x, eps_of(x, float(ab[ts[op[1]]])), x0, z, m, tabs.ddim_coef, tabs.obs_coef, tabs.ddim_t,
                                   step_dev=ctr, t_out=t_vec, D=2)
                hip.counter_add(ctr, 1)
                evals += 1
                assert int(t_vec[0]) == (ts[op[1] + 1] if op[1] + 1 < S_ else 0)
            else:
                hip.resample_renoise(x.view(Nn, 1, Tt, 2), x0.view(Nn, 1, Tt, 2), z.view(Nn, 1, Tt, 2), m, tabs.resample_coef,
                                     tabs.obs_coef, tabs.ddim_t, start, cover, ids, 77, jump, op[2], t_vec, step_dev=ctr, D=2)
                hip.counter_add(ctr, -jump)
                assert int(t_vec[0]) == ts[op[1] - jump]
        torch.cuda.synchronize()
        assert int(ctr) == S_ and torch.equal(z, z0) and torch.equal(x[..., 0], x0[..., 0]), "the loop ends on the observation"
        return x[..., 1].double().flatten().cpu(), evals

    mean, std = RR.gaussian_problem(corr, a)
    plain, e0 = loop([("step", p) for p in range(S_)])
    res, e1 = loop(sch.resample_walk(S_, jump, times))
    assert (e0, e1) == (20, 182)
    err_plain, err_res = abs(float(plain.mean()) - mean), abs(float(res.mean()) - mean)
    print(f"plain: mean {float(plain.mean()):.4f} std {float(plain.std()):.4f} | (2, 10): mean {float(res.mean()):.4f} "
          f"std {float(res.std()):.4f} | posterior {mean:.4f} {std:.4f}")
    assert err_plain > 0.5, "the replacement method is biased on this problem"
    assert err_res <= 0.25 * err_plain
    assert abs(float(res.std()) - std) < abs(float(plain.std()) - std)
    # independent draws per trial, frame and visit: consecutive frames and consecutive trials are uncorrelated given the
    # common observation (5 standard errors of a sample correlation of n pairs, 1 / sqrt(n))
    r = (res - res.mean()).view(Nn, Tt)
    corr_of = lambda u, v: float((u * v).mean() / ((u ** 2).mean() * (v ** 2).mean()).sqrt())
    assert abs(corr_of(r[:, :-1], r[:, 1:])) <= 5 / (Nn * (Tt - 1)) ** 0.5
    assert abs(corr_of(r[:-1], r[1:])) <= 5 / ((Nn - 1) * Tt) ** 0.5
