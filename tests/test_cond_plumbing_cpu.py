"""Host-side plumbing of the masked DDIM sampler and of `analyze` for the diffusion denoisers (no GPU: the C-ABI in
dry-run mode where a test marshals launches, the real library where it checks argument validation)."""
import argparse
import ctypes
import os

import pytest
import torch

from oracle import ref_cpu as R


@pytest.fixture()
def dry():
    from inferbiomechanics_amd import hip
    hip.set_dry_run(True)
    yield hip
    hip.set_dry_run(False)


def test_window_layout_and_label_mask_follow_motion_window_view():
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import (LOSS_KEY_ORDER, LOSS_KEY_WIDTHS, MotionWindowView,
                                                                   SyntheticWindowDataset)
    from inferbiomechanics_amd.models.DiffusionLabelPredictor import DiffusionLabelPredictor, label_mask
    ds = SyntheticWindowDataset(3, 50, 5)
    view = MotionWindowView(ds)
    assert view.feat == 177 and view[0].shape == (10, 177)
    inputs, labels, _, _ = ds[1]
    x = view[1]
    c = 147
    for k, w in zip(LOSS_KEY_ORDER, LOSS_KEY_WIDTHS):          # the label block: the last 30 columns, in loss-key order
        assert torch.equal(x[:, c:c + w], labels[k])
        c += w
    assert c == 177
    m = label_mask(10, 177)
    assert m.dtype == torch.bool and m.shape == (10, 177)
    assert m[:, :147].all() and not m[:, 147:].any()
    batched = {k: v.unsqueeze(0) for k, v in inputs.items()}
    obs = DiffusionLabelPredictor.window_matrix(batched)
    assert torch.equal(obs[0, :, :147], x[:, :147]) and not obs[0, :, 147:].any()
    split = DiffusionLabelPredictor.split_labels(x.unsqueeze(0))
    assert list(split) == LOSS_KEY_ORDER
    for k in LOSS_KEY_ORDER:
        assert torch.equal(split[k][0], labels[k]) and split[k].is_contiguous()
    with pytest.raises(ValueError):
        label_mask(10, 30)


def test_predictor_outputs_dict_and_refusals(dry):
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import (LOSS_KEY_ORDER, LOSS_KEY_WIDTHS, MotionWindowView,
                                                                   SyntheticWindowDataset)
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionMLP, DiffusionTransformer
    from inferbiomechanics_amd.models.DiffusionLabelPredictor import DiffusionLabelPredictor
    ds = SyntheticWindowDataset(4, 50, 5)
    items = [ds[i] for i in range(4)]
    inputs = {k: torch.stack([it[0][k] for it in items]) for k in items[0][0]}
    labels = {k: torch.stack([it[1][k] for it in items]) for k in items[0][1]}
    for dt in (torch.float32, torch.bfloat16):
        for model in (DiffusionMLP(177, [32, 32], temb_dim=16, temb_hidden=24, compute_dtype=dt),
                      DiffusionTransformer(177, 10, d_model=32, num_heads=4, dim_feedforward=64, num_layers=1, temb_dim=16,
                                           temb_hidden=24, compute_dtype=dt)):
            dry.lib().calls.clear()
            out = DiffusionLabelPredictor(model, 5)(inputs, labels, draw=2)
            assert list(out) == LOSS_KEY_ORDER
            for k, w in zip(LOSS_KEY_ORDER, LOSS_KEY_WIDTHS):
                assert out[k].shape == (4, 10, w) and out[k].dtype == torch.float32
            calls = dry.lib().calls
            assert calls.count("ib_ddim_cond_init") == 1 and calls.count("ib_ddim_cond_step") == 5
            assert calls.count("ib_diffusion_draw") == 4 and "ib_ddim_step" not in calls
    with pytest.raises(ValueError, match="all_frames"):
        DiffusionLabelPredictor(DiffusionMLP(177, [32]), output_data_format='last_frame')
    with pytest.raises(ValueError, match="all_frames"):
        MotionWindowView(SyntheticWindowDataset(2, 50, 5, output_data_format='last_frame'))
    last = SyntheticWindowDataset(2, 50, 5, output_data_format='last_frame')
    lab1 = {k: v.unsqueeze(0) for k, v in last[0][1].items()}
    with pytest.raises(ValueError, match="all_frames"):
        DiffusionLabelPredictor(DiffusionMLP(177, [32]))({k: v.unsqueeze(0) for k, v in last[0][0].items()}, lab1)
    with pytest.raises(ValueError, match="feat_dim"):
        DiffusionLabelPredictor(DiffusionMLP(300, [32]))(inputs)


def test_conditional_sampler_plumbing_and_argument_checks(dry):
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler, DDIMSampler
    from inferbiomechanics_amd.diffusion.schedule import DiffusionTables
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    for dt, ld in ((torch.float32, 177), (torch.bfloat16, 192)):      # bf16: the transformer plan's pitched rows
        m = DiffusionTransformer(177, 10, d_model=32, num_heads=4, dim_feedforward=64, num_layers=1, temb_dim=16,
                                 temb_hidden=24, compute_dtype=dt)
        smp = ConditionalDDIMSampler(m, 4)
        mask = torch.zeros(10, 177, dtype=torch.bool)
        mask[:, :147] = True
        out = smp.sample(torch.randn(2, 10, 177), torch.randn(2, 10, 177), mask)
        assert out.shape == (2, 10, 177)
        assert smp._bufs["x0"].shape == smp._bufs["z"].shape == (2, 10, ld) and smp._bufs["mask"].shape == (10, ld)
        assert smp._bufs["mask"].dtype == torch.uint8
        assert torch.equal(smp._bufs["mask"][:, :177], mask.to(torch.uint8)) and not smp._bufs["mask"][:, 177:].any()
        with pytest.raises(ValueError):
            smp.sample(torch.randn(2, 10, 177), torch.randn(2, 10, 176), mask)
        with pytest.raises(ValueError):
            smp.sample(torch.randn(2, 10, 177), torch.randn(2, 10, 177), mask.to(torch.uint8))
        assert "x0" not in DDIMSampler(m, 4)._bufs
    tabs = DiffusionTables(torch.device("cpu"), num_sample_steps=4)
    x = torch.zeros(2, 10, 192)
    mk = torch.zeros(10, 192, dtype=torch.uint8)
    step = lambda **k: dry.ddim_cond_step(k.get("x", x), k.get("eps", x), k.get("x0", x), k.get("z", x), k.get("mask", mk),
                                          tabs.ddim_coef, k.get("oc", tabs.obs_coef), tabs.ddim_t, D=k.get("D", 177))
    step()
    for bad in (dict(mask=torch.zeros(10, 177, dtype=torch.uint8)), dict(mask=mk.bool()), dict(D=193),
                dict(x0=torch.zeros(2, 10, 177)), dict(eps=x.to(torch.bfloat16)), dict(oc=tabs.ddim_coef)):
        with pytest.raises(dry.HipError):
            step(**bad)


def test_masked_step_returns_error_codes_on_bad_arguments():
    from inferbiomechanics_amd import hip
    lib = hip.lib()
    buf = ctypes.create_string_buffer(4096)
    a = ctypes.cast(buf, ctypes.c_void_p).value // 16 * 16 + 16          # any aligned non-NULL address: nothing is launched
    P = lambda ok=True: ctypes.c_void_p(a) if ok else None
    step = lambda nulls=(), B=2, T=10, D=177, ld=192, S=4, dtype=1, t_out=False: lib.ib_ddim_cond_step(
        *[P(i not in nulls) for i in range(8)], S, 0, None, P() if t_out else None, B, T, D, ld, dtype, None)
    for i in range(7):                                            # x, eps, x0, z, mask, coef, obs_coef
        assert step(nulls=(i,)) == -1, i
    assert step(nulls=(7,), t_out=True) == -1                     # t_out without timesteps
    assert step(ld=176) == -1 and step(B=0) == -1 and step(T=0) == -1 and step(D=0) == -1 and step(S=0) == -1
    assert step(dtype=7) == -2
    init = lambda nulls=(), D=177, ld=192, dtype=1: lib.ib_ddim_cond_init(*[P(i not in nulls) for i in range(5)], 2, 10, D,
                                                                         ld, dtype, None)
    for i in range(5):
        assert init(nulls=(i,)) == -1, i
    assert init(ld=100) == -1 and init(dtype=7) == -2


def test_observation_coefficients_against_float64():
    from inferbiomechanics_amd.diffusion import schedule as S
    ab = R.alphas_cumprod(R.linear_beta_schedule(1000))
    for steps in (10, 100):
        ts = R.ddim_timesteps(1000, steps)
        oc = S.observation_coefficients(1000, steps)
        assert oc.dtype == torch.float64 and oc.shape == (steps + 1, 2)
        levels = [ab[ts[0]]] + [ab[ts[i + 1]] for i in range(steps - 1)] + [torch.tensor(1.0, dtype=torch.float64)]
        for r, a in enumerate(levels):
            assert float(oc[r, 0]) == float(torch.sqrt(a)) and float(oc[r, 1]) == float(torch.sqrt(1 - a)), r
        tabs = S.DiffusionTables(torch.device("cpu"), num_sample_steps=steps)
        assert tabs.obs_coef.dtype == torch.float32 and torch.equal(tabs.obs_coef, oc.to(torch.float32))
        assert tabs.obs_coef[-1].tolist() == [1.0, 0.0]
        # the DDIM update (c_x, c_eps) and the observation level agree: sqrt(ab_prev) = c_x sqrt(ab_t)
        cx = R.ddim_coeffs(1000, steps)[:, 0]
        assert torch.allclose(oc[1:, 0], cx * oc[:-1, 0], rtol=1e-12, atol=0)


def test_analyze_flags_and_diffusion_model_reconstruction(dry, tmp_path):
    from inferbiomechanics_amd.cli.analyze import AnalyzeCommand
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import MotionWindowView
    from inferbiomechanics_amd.main import main
    p = argparse.ArgumentParser()
    sp = p.add_subparsers(dest="command")
    cmd = AnalyzeCommand()
    cmd.register_subcommand(sp)
    a = p.parse_args(['analyze', '--model-type', 'diffusion-transformer', '--synthetic-windows', '4'])
    assert (a.sample_steps, a.sample_seed, a.sample_batch) == (100, 0, 1)
    a = p.parse_args(['analyze', '--model-type', 'diffusion-transformer', '--synthetic-windows', '4', '--sample-steps', '20',
                      '--sample-seed', '7', '--sample-batch', '16', '--compute-dtype', 'bf16'])
    assert (a.sample_steps, a.sample_seed, a.sample_batch) == (20, 7, 16)
    view = cmd.diffusion_view(a, 'dev', None)
    assert isinstance(view, MotionWindowView) and len(view) == 4 and view.feat == 177
    model = cmd.diffusion_model(a, view, 'cpu')
    assert (model.feat_dim, model.window, model.compute_dtype) == (177, 10, torch.bfloat16)
    a.model_type = 'diffusion-mlp'
    assert cmd.diffusion_model(a, view, 'cpu').feat_dim == 177
    a.output_data_format = 'last_frame'
    with pytest.raises(ValueError, match="all_frames"):
        cmd.diffusion_view(a, 'dev', None)

    # the whole command in dry-run: train the MLP denoiser on 177-wide motion windows, analyze 5 labelled windows per split
    ck = str(tmp_path / "ck")
    common = ['--no-wandb', '--checkpoint-dir', ck, '--data-loading-workers', '0', '--model-type', 'diffusion-mlp',
              '--hidden-dims', '32', '32']
    assert main(['train', '--synthetic-windows', '8', '--feat-dim', '177', '--epochs', '1', '--max-steps', '1',
                 '--batch-size', '4'] + common)
    dry.lib().calls.clear()
    assert main(['analyze', '--synthetic-windows', '5', '--sample-steps', '4', '--sample-batch', '2'] + common)
    rows = open(os.path.join(ck, 'diffusion-mlp', 'dev_analysis.csv')).read().strip().splitlines()
    assert rows == [f'synthetic_subject_0,window_{i}' for i in range(5)]
    assert len(open(os.path.join(ck, 'diffusion-mlp', 'train_analysis.csv')).read().strip().splitlines()) == 5
    calls = dry.lib().calls
    assert calls.count("ib_ddim_cond_init") == 6 and calls.count("ib_ddim_cond_step") == 6 * 4     # 3 sampler calls a split
    with pytest.raises(ValueError, match="all_frames"):
        main(['analyze', '--synthetic-windows', '2', '--output-data-format', 'last_frame'] + common)
