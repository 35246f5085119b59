"""Sampling from a denoiser trained on clean conditioning columns (`train --cond-cols`): ConditionalDDIMSampler with
observations = 'clean' keeps every observed element equal to the observation, in the start state and after every step, for
every solver; the free elements take the update they take in 'noised' mode; a mask that is not the model's conditioning
columns is refused; switching modes re-captures; DiffusionLabelPredictor and `analyze` pick the mode from the model /
the checkpoint.  -m gpu."""
import os

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


def model_for(dt, D, T=24, cond=True):
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    m = DiffusionTransformer(D, T, d_model=128, num_heads=2, dim_feedforward=256, num_layers=2, device=DEV, compute_dtype=dt)
    load_det(m)
    if cond:
        m.cond_cols = D - 30
    return m


def prefix_mask(T, D, C):
    m = torch.zeros(T, D, dtype=torch.bool)
    m[:, :C] = True
    return m


SOLVERS = [("ddim", 0.0), ("ddim", 0.5), ("ddim", 1.0), ("dpmpp2m", 0.0)]


@pytest.mark.parametrize("solver,eta", SOLVERS)
@pytest.mark.parametrize("D", [44, 64])                  # bf16: 44 is pitched by the inference plan, 64 is not
@pytest.mark.parametrize("dt", [torch.float32, BF])
def test_clean_mode_pins_the_observation_after_every_step(dt, D, solver, eta):
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler
    B, T, S = 3, 24, 10
    model = model_for(dt, D, T)
    C = model.cond_cols
    m = prefix_mask(T, D, C)
    z = R.det_fill((B, T, D), 31, 1.0, torch.float32).to(DEV)
    obs = R.det_fill((B, T, D), 32, 2.0, torch.float32).to(DEV)
    want = obs.to(dt)[:, :, :C]
    smp = ConditionalDDIMSampler(model, S, eta=eta, seed=5, solver=solver, observations="clean")
    frees = []
    for k in (1, 2, 5, S):
        got = smp.sample(z, obs, m, steps=k)
        assert got.dtype == dt
        assert torch.equal(got[:, :, :C], want), f"observed elements differ from the observation after {k} steps"
        assert torch.isfinite(got).all()
        frees.append(got[:, :, C:].clone())
        # the state buffer itself (pitched [B, T, Dp]): observed part clean, pad columns 0
        xs = smp._bufs["x"]
        assert torch.equal(xs[:, :, :C], want) and not xs[:, :, D:].any()
    assert not torch.equal(frees[1], frees[0]) and not torch.equal(frees[-1], frees[1])


@pytest.mark.parametrize("solver,eta", SOLVERS)
@pytest.mark.parametrize("D,ld", [(44, 44), (44, 48), (300, 320), (177, 177)])
@pytest.mark.parametrize("dt", [torch.float32, BF])
def test_free_elements_take_the_noised_mode_update(dt, D, ld, solver, eta):
    """the update entry points on fixed eps tensors, once with the 'noised' observation table and once with the 'clean'
    one: the free elements' arithmetic is shared, so they are equal bit for bit; the observed ones are the observation"""
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion.schedule import DiffusionTables
    B, T, S, C = 2, 10, 10, D - 30
    g = torch.Generator().manual_seed(D + ld)
    mk = lambda: torch.randn(B, T, ld, generator=g).to(dt).to(DEV)
    x_start, x0, z0 = mk(), mk(), mk()
    for a in (x_start, x0, z0):
        a[:, :, D:] = 0
    mask = torch.zeros(T, ld, dtype=torch.uint8, device=DEV)
    mask[:, :C] = 1
    win = torch.arange(B, dtype=torch.int64, device=DEV)
    out = {}
    for mode in ("noised", "clean"):
        tabs = DiffusionTables(DEV)
        tabs.set_sampler(S, eta, solver, "time", observations=mode)
        assert tabs.observations == mode
        x, z = x_start.clone(), z0.clone()
        if mode == "clean":                    # the start state: observed <- the observation, free elements keep the draw
            xi = z0.clone()
            hip.ddim_cond_init(xi, x0, z0, mask, tabs.obs_coef, D=D)
            assert torch.equal(xi[:, :, :C], x0[:, :, :C]) and torch.equal(xi[:, :, C:], z0[:, :, C:])
        hist = torch.zeros((B, T, ld), dtype=torch.float32, device=DEV)
        t_vec = torch.zeros(B, dtype=torch.int64, device=DEV)
        ctr = torch.zeros(1, dtype=torch.int32, device=DEV)
        states = []
        for s in range(4):
            ge = torch.Generator().manual_seed(100 + s)
            eps = torch.randn(B, T, ld, generator=ge).to(dt).to(DEV)
            eps[:, :, D:] = 0
            if solver == "dpmpp2m":
                hip.dpmpp_cond_step(x, eps, hist, x0, z, mask, tabs.dpmpp_coef, tabs.obs_coef, tabs.ddim_t, step_dev=ctr,
                                    t_out=t_vec, D=D)
            elif eta == 0.0:
                hip.ddim_cond_step(x, eps, x0, z, mask, tabs.ddim_coef, tabs.obs_coef, tabs.ddim_t, step_dev=ctr, t_out=t_vec,
                                   D=D)
            else:
                hip.ddim_cond_step_noise(x, eps, x0, z, mask, tabs.ddim_coef_eta, tabs.obs_coef, tabs.obs_noise_coef,
                                         tabs.ddim_t, win, 9, step_dev=ctr, t_out=t_vec, D=D)
            hip.counter_add(ctr, 1)
            torch.cuda.synchronize()
            states.append(x.clone())
            if mode == "clean":
                assert torch.equal(x[:, :, :C], x0[:, :, :C]), f"step {s}: observed elements must be the observation"
        out[mode] = states
    for s, (a, b) in enumerate(zip(out["noised"], out["clean"])):
        assert torch.equal(a[:, :, C:], b[:, :, C:]), f"step {s}: free elements differ between the modes"


def test_clean_table_and_mask_checks():
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler
    B, T, D, S = 2, 24, 44, 10
    model = model_for(torch.float32, D, T)
    C = model.cond_cols
    z, obs = torch.randn(B, T, D, device=DEV), torch.randn(B, T, D, device=DEV)
    smp = ConditionalDDIMSampler(model, S, observations="clean")
    for bad in (prefix_mask(T, D, C - 1), prefix_mask(T, D, C + 1), torch.zeros(T, D, dtype=torch.bool),
                torch.ones(T, D, dtype=torch.bool)):
        with pytest.raises(ValueError, match="cond_cols"):
            smp.sample(z, obs, bad)
    holes = prefix_mask(T, D, C)
    holes[3, 2] = False
    with pytest.raises(ValueError, match="cond_cols"):
        smp.sample(z, obs, holes)
    smp.sample(z, obs, prefix_mask(T, D, C))                      # the right mask runs
    model.cond_cols = 0                                            # an unconditional model has no clean mode
    with pytest.raises(ValueError, match="cond_cols"):
        smp.sample(z, obs, prefix_mask(T, D, C))
    with pytest.raises(ValueError):
        ConditionalDDIMSampler(model, S, observations="pinned")
    # 'noised' takes any mask, as before
    ConditionalDDIMSampler(model, S).sample(z, obs, holes)


@pytest.mark.parametrize("dt", [torch.float32, BF])
def test_switching_modes_recaptures(dt):
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler
    B, T, D, S = 3, 24, 44, 10
    model = model_for(dt, D, T)
    C = model.cond_cols
    m = prefix_mask(T, D, C)
    z = R.det_fill((B, T, D), 41, 1.0, torch.float32).to(DEV)
    obs = R.det_fill((B, T, D), 42, 2.0, torch.float32).to(DEV)
    want = {mode: ConditionalDDIMSampler(model, S, observations=mode).sample(z, obs, m) for mode in ("noised", "clean")}
    assert not torch.equal(want["noised"][:, :, C:], want["clean"][:, :, C:])
    smp = ConditionalDDIMSampler(model, S)
    graphs, last = [], None                                        # every captured graph, held so that none is reused
    for mode in ("noised", "clean", "noised", "clean", "clean"):
        smp.observations = mode
        got = smp.sample(z, obs, m)
        assert smp._graph is not None
        if mode != last:
            assert all(smp._graph is not g for g in graphs), f"switching to {mode!r} replayed an earlier capture"
            graphs.append(smp._graph)
        else:
            assert smp._graph is graphs[-1], "the same mode again must replay its capture"
        last = mode
        assert torch.equal(got, want[mode]), mode
        assert model.tables(smp._bufs["x"].device).observations == mode
    assert len(graphs) == 4
    # truncated loops in the other mode still see that mode's table
    smp.observations = "noised"
    a = smp.sample(z, obs, m, steps=3)
    smp.observations = "clean"
    b = smp.sample(z, obs, m, steps=3)
    assert torch.equal(b[:, :, :C], obs.to(dt)[:, :, :C]) and not torch.equal(a[:, :, :C], b[:, :, :C])


@pytest.mark.parametrize("kw", [{}, {"eta": 1.0, "num_samples": 3}, {"solver": "dpmpp2m", "spacing": "logsnr"}])
@pytest.mark.parametrize("dt", [torch.float32, BF])
def test_label_predictor_pins_clean_for_a_conditional_model(dt, kw):
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import INPUT_KEY_ORDER, LOSS_KEY_ORDER, SyntheticWindowDataset
    from inferbiomechanics_amd.models.DiffusionLabelPredictor import DiffusionLabelPredictor
    ds = SyntheticWindowDataset(4, history_len=50, stride=5, seed=2)
    inputs = {k: torch.stack([ds[i][0][k] for i in range(2)]) for k in INPUT_KEY_ORDER}
    obs = DiffusionLabelPredictor.window_matrix(inputs)
    B, F, D = obs.shape
    model = model_for(dt, D, F)
    pred = DiffusionLabelPredictor(model, 10, seed=3, **kw)
    out = pred(inputs)
    assert pred.sampler.observations == "clean"
    K = kw.get("num_samples", 1)
    xs = pred.sampler._bufs["x"]                                    # the sampler's state after the loop
    want = obs.to(DEV).to(dt)[:, :, :D - 30].repeat_interleave(K, dim=0)
    assert xs.shape[0] == B * K and torch.equal(xs[:, :, :D - 30], want)
    for k in LOSS_KEY_ORDER:
        assert torch.isfinite(out[k]).all()
    # the unconditional model keeps the forward-noised observations
    model.cond_cols = 0
    pred(inputs)
    assert pred.sampler.observations == "noised"
    model.cond_cols = 7
    with pytest.raises(ValueError, match="cond_cols"):
        pred(inputs)


def test_checkpoint_round_trip_train_then_analyze(tmp_path, monkeypatch, capsys):
    from inferbiomechanics_amd.main import main
    from inferbiomechanics_amd.models.DiffusionLabelPredictor import DiffusionLabelPredictor
    ck = str(tmp_path / "ck")
    mt = "diffusion-transformer"
    common = ['--no-wandb', '--checkpoint-dir', ck, '--data-loading-workers', '0', '--model-type', mt]
    train = ['train', '--synthetic-windows', '16', '--feat-dim', '177', '--epochs', '1', '--max-steps', '2', '--batch-size',
             '8'] + common
    with pytest.raises(SystemExit):
        main(train + ['--cond-cols', '177'])
    assert main(train + ['--cond-cols', '147', '--ema-decay', '0.9'])
    files = sorted(os.listdir(os.path.join(ck, mt)))
    path = os.path.join(ck, mt, [f for f in files if f.endswith('.pt')][-1])
    saved = torch.load(path, map_location='cpu')
    assert saved['cond_cols'] == 147 and 'ema_state_dict' in saved

    seen = []
    orig = DiffusionLabelPredictor.__call__

    def spy(self, inputs, labels=None, draw=0):
        out = orig(self, inputs, labels, draw)
        seen.append((self.model.cond_cols, self.sampler.observations))
        return out

    monkeypatch.setattr(DiffusionLabelPredictor, '__call__', spy)
    analyze = ['analyze', '--synthetic-windows', '3', '--sample-steps', '10', '--sample-seed', '3'] + common
    assert main(analyze)                                            # no new flag: the checkpoint decides
    assert seen and set(seen) == {(147, 'clean')}
    seen.clear()
    assert main(analyze + ['--use-ema', '--sampler', 'dpmpp2m', '--sample-spacing', 'logsnr'])
    assert seen and set(seen) == {(147, 'clean')}
    # resuming with another value is refused, with the same value it goes on
    with pytest.raises(SystemExit):
        main(train + ['--epochs', '2'])
    assert main(train + ['--epochs', '2', '--cond-cols', '147', '--ema-decay', '0.9'])
    # an old-style checkpoint (no key) loads as 0
    for f in os.listdir(os.path.join(ck, mt)):
        if f.endswith('.pt'):
            p = os.path.join(ck, mt, f)
            c = torch.load(p, map_location='cpu')
            c.pop('cond_cols', None)
            torch.save(c, p)
    seen.clear()
    assert main(analyze)
    assert seen and set(seen) == {(0, 'noised')}
