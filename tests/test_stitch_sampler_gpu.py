"""StitchedDDIMSampler on the GPU: one window and disjoint windows against ConditionalDDIMSampler (bit for bit), overlapping
windows (finite, observations kept, captured graph against eager launches, replay for a new batch), and
DiffusionLabelPredictor.predict_trial.  The smallest denoiser of tests/test_cond_sampler_gpu.py, in bf16 with the pitched
state (44 columns in rows padded to the plan's pitch).  -m gpu."""
import pytest
import torch

from oracle.fixture_inputs import det_state

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
N, T, D, S, C = 2, 24, 44, 5, 14


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


@pytest.fixture(scope="module")
def model():
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    m = DiffusionTransformer(D, T, d_model=128, num_heads=2, dim_feedforward=256, num_layers=2, device=DEV, compute_dtype=BF)
    load_det(m)
    return m


def draws(F, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, F, D, generator=g).to(DEV), torch.randn(N, F, D, generator=g).to(DEV)


def cols():
    c = torch.zeros(D, dtype=torch.bool)
    c[:C] = True
    return c


@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
def test_one_window_is_the_conditional_sampler(model, solver):
    from inferbiomechanics_amd.diffusion import ConditionalDDIMSampler, StitchedDDIMSampler
    z, obs = draws(T, 1)
    ref = ConditionalDDIMSampler(model, S, solver=solver).sample(z, obs, cols()[None, :].expand(T, D).contiguous())
    st = StitchedDDIMSampler(model, S, solver=solver)
    got = st.sample(z, obs, cols())
    Dp = st._bufs["x"].shape[-1]
    assert st._bufs["x"].shape == (N, T, Dp) and Dp > D and Dp % 8 == 0 and "eps" in st._bufs, "the pitched state"
    assert got.shape == (N, T, D) and torch.equal(got, ref)


@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
def test_disjoint_windows_are_the_per_window_sampler(model, solver):
    from inferbiomechanics_amd.diffusion import ConditionalDDIMSampler, StitchedDDIMSampler
    z, obs = draws(2 * T, 2)
    ref = ConditionalDDIMSampler(model, S, solver=solver).sample(z.view(2 * N, T, D), obs.view(2 * N, T, D),
                                                                 cols()[None, :].expand(T, D).contiguous())
    st = StitchedDDIMSampler(model, S, hop=T, solver=solver)
    got = st.sample(z, obs, cols())
    assert st.layout["W"] == 2 and torch.equal(got, ref.view(N, 2 * T, D))


@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
def test_overlapping_windows(model, solver):
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion import StitchedDDIMSampler
    F = 2 * T
    z, obs = draws(F, 3)
    graph = StitchedDDIMSampler(model, S, hop=T // 2, solver=solver)
    eager = StitchedDDIMSampler(model, S, hop=T // 2, solver=solver, use_graph=False)
    name = "ib_stitch_dpmpp_step" if solver == "dpmpp2m" else "ib_stitch_ddim_step"
    with hip.record_launches() as rec:
        want = eager.sample(z, obs, cols())
    names = [n for n, _ in rec.calls]
    assert names.count(name) == S and not [n for n in names if n.endswith(("ddim_step", "ddim_cond_step", "dpmpp_step",
                                                                               "dpmpp_cond_step")) and n != name]
    got = graph.sample(z, obs, cols())
    assert graph.layout["W"] == 3 and graph._graph is not None and eager._graph is None
    assert got.shape == (N, F, D) and bool(torch.isfinite(got).all())
    assert torch.equal(got[..., :C], obs[..., :C].to(BF)), "observed columns must equal the observation"
    assert torch.equal(got, want), "captured graph and eager launches disagree"
    g0 = graph._graph
    z2, obs2 = draws(F, 4)
    got2 = graph.sample(z2, obs2, cols())
    assert graph._graph is g0, "a new batch of the same shape replays the captured step"
    assert torch.equal(got2, eager.sample(z2, obs2, cols())) and not torch.equal(got2, got)
    # without observations: the unconditional loop of the same class
    free = StitchedDDIMSampler(model, S, hop=T // 2, solver=solver)
    a, b = free.sample(z), StitchedDDIMSampler(model, S, hop=T // 2, solver=solver, use_graph=False).sample(z)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


def test_predict_trial_layout():
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import LOSS_KEY_ORDER, LOSS_KEY_WIDTHS, SyntheticWindowDataset
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    from inferbiomechanics_amd.models.DiffusionLabelPredictor import DiffusionLabelPredictor
    m = DiffusionTransformer(177, 10, d_model=128, num_heads=2, dim_feedforward=256, num_layers=2, device=DEV, compute_dtype=BF)
    load_det(m)
    ds = SyntheticWindowDataset(4, 50, 5)                              # windows of 10 frames
    items = [ds[i] for i in range(4)]
    inputs = {k: torch.stack([torch.cat([items[2 * n][0][k], items[2 * n + 1][0][k]]) for n in range(2)]).to(DEV)
              for k in items[0][0]}                                    # [2, 20, c]
    pred = DiffusionLabelPredictor(m, S)
    out = pred.predict_trial(inputs, hop=4)
    assert list(out) == LOSS_KEY_ORDER
    for k, w in zip(LOSS_KEY_ORDER, LOSS_KEY_WIDTHS):
        assert out[k].shape == (2, 20, w) and out[k].dtype == torch.float32 and bool(torch.isfinite(out[k]).all())
    again = pred.predict_trial(inputs, hop=4)                          # the captured step replayed: the same trajectory
    other = pred.predict_trial(inputs, hop=4, draw=5)                  # another start draw: another one
    for k in LOSS_KEY_ORDER:
        assert torch.equal(again[k], out[k]) and not torch.equal(other[k], out[k])


def test_visualize_trial_flags_run_both_samplers(tmp_path, capsys):
    """`visualize --trial-frames`: the denoiser the CLI builds (no checkpoint: its initial weights), one synthetic trial of 25
    frames as 4 windows of 10 every 5 frames next to its 3 disjoint windows; every printed figure is a finite number"""
    import re
    from inferbiomechanics_amd.main import main
    capsys.readouterr()
    assert main(["visualize", "--model-type", "diffusion-transformer", "--synthetic-windows", "4", "--compute-dtype", "bf16",
                 "--checkpoint-dir", str(tmp_path / "ck"), "--sample-steps", "10", "--trial-frames", "25", "--num-frames", "1"])
    out = capsys.readouterr().out
    assert "25 frames, stitched as 4 windows of 10 every 5 frames (ramp) | 3 disjoint windows" in out
    lines = out.splitlines()
    at = next(i for i, line in enumerate(lines) if line.startswith("trial 0 ("))
    rows = lines[at + 2:at + 27]
    values = [float(v) for line in rows for v in re.findall(r"[+-]\d+\.\d{3}", line)]
    assert len(values) == 25 * 12 and all(abs(v) < 1e3 for v in values) and any(v != 0.0 for v in values)
    assert "nan" not in out.lower() and "inf" not in out.lower().replace("inferred", "")
    assert len(re.findall(r"RMS stitched - per-window \d+\.\d+", out)) == 4 and "mean jump across the 2 per-window" in out
