"""The stochastic samplers (eta > 0) and the posterior ensembles of `analyze` on the GPU: both sampler loops against the
float64 oracle denoisers fed the same reference normals, the captured step replayed for a batch with other window ids,
eta = 0 unchanged, and DiffusionLabelPredictor / `main.py analyze` with --sample-eta / --num-samples.  -m gpu."""
import os

import pytest
import torch

import numpy as np

from oracle import ref_cpu as R
from oracle.fixture_inputs import det_state

pytestmark = pytest.mark.gpu

DEV = "cuda"
GEN_TOL = 2e-5                   # tests/test_noise_gpu.py: hardware log2 / sin / cos against float64, absolute


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


def ref_normals(T, D, seed, s, wid):
    """float64 [T, D] normals of a window at sampling step s (as tests/test_eta_kernels_gpu.py): oracle words of counter
    ((f D + d) / 4, s, wid, domain 2), Box-Muller in float64"""
    n = T * D
    nb = (n + 3) // 4
    w = (R.draw_words(nb, seed, s, wid, 2) >> np.uint32(8)).astype(np.float64)
    out = np.empty((nb, 4), dtype=np.float64)
    for a in (0, 2):
        r = np.sqrt(-2.0 * np.log((w[:, a] + 1.0) * 2.0 ** -24))
        th = 2.0 * np.pi * (w[:, a + 1] * 2.0 ** -24)
        out[:, a], out[:, a + 1] = r * np.cos(th), r * np.sin(th)
    return torch.from_numpy(out.reshape(-1)[:n].reshape(T, D).copy())


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from inferbiomechanics_amd import hip
    hip.lib()


def small_models():
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionMLP, DiffusionTransformer
    mlp = DiffusionMLP(44, [64, 64], device=DEV)
    tr = DiffusionTransformer(44, 24, d_model=128, num_heads=2, dim_feedforward=256, num_layers=2, device=DEV)
    load_det(mlp)
    load_det(tr)
    return {"mlp": mlp, "transformer": tr}


def loop64(eps_fn, xT, S, eta, seed, ids, obs=None, m=None):
    """float64 restatement of the stochastic loop (and of its masked form: observed elements carry their noise e)"""
    from inferbiomechanics_amd.diffusion import schedule as sch
    c = sch.ddim_coefficients_eta(1000, S, eta)
    oc = sch.observation_coefficients(1000, S)
    on = sch.observation_noise_coefficients(1000, S, eta)
    ts = R.ddim_timesteps(1000, S).tolist()
    B, T, D = xT.shape
    x, e = xT.clone(), xT.clone()
    if m is not None:
        x = torch.where(m, oc[0, 0] * obs + oc[0, 1] * e, x)
    for s, t in enumerate(ts):
        eps = eps_fn(x, torch.full((B,), t, dtype=torch.int64))
        n = torch.stack([ref_normals(T, D, seed, s, int(i)) for i in ids])
        free = c[s, 0] * x + c[s, 1] * eps + c[s, 2] * n
        if m is None:
            x = free
        else:
            if float(c[s, 2]) != 0.0:
                e = on[s, 0] * e + on[s, 1] * n
            x = torch.where(m, oc[s + 1, 0] * obs + oc[s + 1, 1] * e, free)
    return x, float(c[:, 2].sum())


@pytest.mark.parametrize("eta", [0.5, 1.0])
@pytest.mark.parametrize("kind", ["mlp", "transformer"])
def test_stochastic_loops_match_float64(kind, eta):
    """fp32, the shapes of the eta = 0 loop tests; their tolerance (2e-3 of the largest value) + 2e-5 sum_s sigma_s"""
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler, DDIMSampler
    model = small_models()[kind]
    B, T, D, S, seed = 3, 24, 44, 10, 12345
    ids = [11, 5, 2 ** 32 - 2]
    xT = R.det_fill((B, T, D), 11, 1.0, torch.float32)
    obs = R.det_fill((B, T, D), 15, 1.0, torch.float32)
    p = params64(model)
    fn = (lambda x, t: R.denoiser_mlp_forward(p, x, t, [64, 64])) if kind == "mlp" else \
        (lambda x, t: R.denoiser_transformer_forward(p, x, t, 2, 2))
    m = label_mask(T, D)
    for cond in (False, True):
        if cond:
            got = ConditionalDDIMSampler(model, S, eta=eta, seed=seed).sample(xT.to(DEV), obs.to(DEV), m, window_ids=ids)
        else:
            got = DDIMSampler(model, S, eta=eta, seed=seed).sample(xT.to(DEV), window_ids=ids)
        with torch.no_grad():
            want, sig_sum = loop64(fn, xT.double(), S, eta, seed, ids, obs.double() if cond else None, m if cond else None)
        err = float((got.cpu().double() - want).abs().max())
        tol = 2e-3 * float(want.abs().max()) + GEN_TOL * sig_sum
        print(f"{kind} eta={eta} cond={cond}: max err {err:.3e} (tol {tol:.3e}, sum sigma {sig_sum:.3f})")
        assert torch.isfinite(got).all() and err <= tol, (cond, err, tol)
        if cond:
            assert torch.equal(got.cpu()[:, m], obs[:, m]), "observed elements must equal the observation"


def test_second_batch_with_other_window_ids_replays_the_captured_step():
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler, DDIMSampler
    model = small_models()["transformer"]
    B, T, D, S = 3, 24, 44, 10
    z1, z2, o1, o2 = (R.det_fill((B, T, D), k, 1.0, torch.float32).to(DEV) for k in (21, 22, 23, 24))
    m1, m2 = label_mask(T, D), label_mask(T, D, free=12)
    smp = ConditionalDDIMSampler(model, S, eta=1.0, seed=5)
    a = smp.sample(z1, o1, m1)
    graph = smp._graph
    assert graph is not None
    b = smp.sample(z2, o2, m2, window_ids=[7, 8, 9])
    assert smp._graph is graph, "a batch of the same shape must replay the captured step"
    assert torch.equal(a, ConditionalDDIMSampler(model, S, eta=1.0, seed=5).sample(z1, o1, m1))
    assert torch.equal(b, ConditionalDDIMSampler(model, S, eta=1.0, seed=5).sample(z2, o2, m2, window_ids=[7, 8, 9]))
    assert not torch.equal(b, ConditionalDDIMSampler(model, S, eta=1.0, seed=5).sample(z2, o2, m2))        # ids 0, 1, 2
    assert not torch.equal(a, ConditionalDDIMSampler(model, S, eta=1.0, seed=6).sample(z1, o1, m1))
    unc = DDIMSampler(model, S, eta=0.5, seed=5)
    u1 = unc.sample(z1)
    g = unc._graph
    u2 = unc.sample(z1, window_ids=[3, 1, 0])
    assert unc._graph is g and not torch.equal(u1, u2)
    assert torch.equal(u2, DDIMSampler(model, S, eta=0.5, seed=5).sample(z1, window_ids=[3, 1, 0]))
    # window b of a batch = the same window alone, with its id (same kernels: T * D % 8 == 0)
    assert torch.equal(u2[2], DDIMSampler(model, S, eta=0.5, seed=5, use_graph=False).sample(z1, window_ids=[9, 9, 0])[2])


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_eta_zero_is_the_deterministic_sampler(dt):
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler, DDIMSampler
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    model = DiffusionTransformer(44, 24, d_model=128, num_heads=2, dim_feedforward=256, num_layers=2, device=DEV, compute_dtype=dt)
    load_det(model)
    B, T, D, S = 3, 24, 44, 10
    xT = R.det_fill((B, T, D), 11, 1.0, torch.float32).to(DEV)
    obs = R.det_fill((B, T, D), 12, 1.0, torch.float32).to(DEV)
    m = label_mask(T, D)
    want_u, want_c = DDIMSampler(model, S).sample(xT), ConditionalDDIMSampler(model, S).sample(xT, obs, m)
    with hip.record_launches() as rec:
        got_u = DDIMSampler(model, S, use_graph=False, eta=0.0, seed=99).sample(xT, window_ids=[4, 5, 6])
        got_c = ConditionalDDIMSampler(model, S, use_graph=False, eta=0.0, seed=99).sample(xT, obs, m, window_ids=[4, 5, 6])
        torch.cuda.synchronize()
    names = [n for n, _ in rec.calls]
    assert torch.equal(got_u, want_u) and torch.equal(got_c, want_c)
    assert names.count("ib_ddim_step") == S and names.count("ib_ddim_cond_step") == S
    assert "ib_ddim_step_noise" not in names and "ib_ddim_cond_step_noise" not in names
    # one stochastic loop beside them: the same launch count per step
    with hip.record_launches() as rec1:
        DDIMSampler(model, S, use_graph=False, eta=1.0).sample(xT)
        torch.cuda.synchronize()
    with hip.record_launches() as rec0:
        DDIMSampler(model, S, use_graph=False).sample(xT)
        torch.cuda.synchronize()
    assert len(rec1.calls) == len(rec0.calls) and [n for n, _ in rec1.calls].count("ib_ddim_step_noise") == S


# ---------------------------------------------------------------------------------------------------------------------
# predictor and analyze, on the tiny checkpoint recipe of tests/test_cond_analyze_gpu.py
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model_type", ["diffusion-mlp", "diffusion-transformer"])
def test_analyze_posterior_ensembles(tmp_path, monkeypatch, capsys, model_type):
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import LOSS_KEY_ORDER
    from inferbiomechanics_amd.main import main
    from inferbiomechanics_amd.models.DiffusionLabelPredictor import DiffusionLabelPredictor
    ck = str(tmp_path / "ck")
    common = ['--no-wandb', '--checkpoint-dir', ck, '--data-loading-workers', '0', '--model-type', model_type]
    if model_type == 'diffusion-mlp':
        common += ['--hidden-dims', '64', '64']
    assert main(['train', '--synthetic-windows', '16', '--feat-dim', '177', '--epochs', '1', '--max-steps', '2',
                 '--batch-size', '8'] + common)
    csv = lambda split: open(os.path.join(ck, model_type, f'{split}_analysis.csv')).read()

    # defaults: the flags at their default values change nothing that is written
    analyze = ['analyze', '--synthetic-windows', '6', '--sample-steps', '10', '--sample-seed', '3'] + common
    capsys.readouterr()
    assert main(analyze)
    plain, rows = capsys.readouterr().out, (csv('dev'), csv('train'))
    assert main(analyze + ['--sample-eta', '0', '--num-samples', '1'])
    assert capsys.readouterr().out == plain and 'Ensemble spread' not in plain
    assert (csv('dev'), csv('train')) == (rows[0] * 2, rows[1] * 2)

    calls = []
    orig = DiffusionLabelPredictor.__call__

    def spy(self, inputs, labels=None, draw=0):
        out = orig(self, inputs, labels, draw)
        calls.append((self, {k: v.clone() for k, v in inputs.items()}, draw, {k: v.detach().cpu().clone() for k, v in out.items()},
                      {k: v.detach().cpu().clone() for k, v in self.last_std.items()}))
        return out

    monkeypatch.setattr(DiffusionLabelPredictor, '__call__', spy)
    ens = analyze + ['--num-samples', '4', '--sample-eta', '1']
    assert main(ens)
    out1 = capsys.readouterr().out
    one = calls[:]
    calls.clear()
    assert main(ens + ['--sample-batch', '3'])
    out3 = capsys.readouterr().out
    assert len(one) == 12 and [c[2] for c in calls] == [0, 3, 0, 3]
    assert out1.count('Ensemble spread (') == 2 and f'Ensemble spread (dev, 4 samples per window): {LOSS_KEY_ORDER[0]}: mean std ' in out1
    worst = 0.0
    for split in range(2):
        for i in range(6):
            for which in (3, 4):                                   # the mean and the std
                a, e = calls[2 * split + i // 3][which], one[6 * split + i][which]
                for k in LOSS_KEY_ORDER:
                    worst = max(worst, float((a[k][i % 3] - e[k][0]).abs().max()))
    print(f"{model_type}: --sample-batch 3 against 1, largest difference of mean / std: {worst:.3e}")
    assert worst == 0.0, "--sample-batch must not change the ensembles"
    assert out1 == out3

    # the mean of K = 4 = the mean of four K = 1 calls with the members' window ids; the spread is there
    monkeypatch.setattr(DiffusionLabelPredictor, '__call__', orig)
    predictor, inputs, draw, mean, std = one[4]
    single = DiffusionLabelPredictor(predictor.model, 10, seed=3, eta=1.0)
    members = [single(inputs, draw=draw * 4 + k) for k in range(4)]
    for k in LOSS_KEY_ORDER:
        acc = torch.zeros_like(members[0][k])
        for mem in members:
            acc = acc + mem[k]
        ref = (acc / 4).cpu()
        amax = float(torch.stack([mem[k] for mem in members]).abs().max())
        assert float((mean[k] - ref).abs().max()) <= 5 * 2.0 ** -24 * amax, k     # test_ensemble_stats_against_float64: (K + 1) u max|x|
        assert bool((std[k] > 0).all()), k
        assert not torch.equal(members[0][k], members[1][k])
