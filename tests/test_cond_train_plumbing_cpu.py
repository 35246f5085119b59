"""Host side of conditional training (`train --cond-cols`) without a GPU: the flag's validation, the bindings' shape / stride /
range checks and the launches of the trainer in dry-run mode, chain_ok at cond_cols > 0, the clean observation table,
DiffusionTables.serves and the sampler's capture signature across the two observation modes, the loss evaluator's and the
checkpoint's cond_cols plumbing."""
import argparse

import pytest
import torch

BF = torch.bfloat16


@pytest.fixture()
def dry():
    from inferbiomechanics_amd import hip
    hip.set_dry_run(True)
    yield hip
    hip.set_dry_run(False)


def test_new_entries_are_exported_and_declared():
    from inferbiomechanics_amd import hip
    lib = hip.lib()
    for name in ("ib_q_sample_cond", "ib_mse_loss_partial_cond", "ib_mse_loss_finalize_cond"):
        assert name in hip.declared_symbols() and name in hip._SIGS and hasattr(lib, name)
    # the conditional entries take their neighbours' arguments plus cond_cols (the finalize: the two counts apart)
    q = hip._SIGS["ib_q_sample"][1]
    assert hip._SIGS["ib_q_sample_cond"][1] == q[:-2] + [hip._i64] + q[-2:]
    p = hip._SIGS["ib_mse_loss_partial"][1]
    assert hip._SIGS["ib_mse_loss_partial_cond"][1] == p[:-2] + [hip._i64] + p[-2:]
    f = hip._SIGS["ib_mse_loss_finalize"][1]
    assert hip._SIGS["ib_mse_loss_finalize_cond"][1] == f[:-1] + [hip._i64] + f[-1:]
    # argument errors are reported before anything is launched (IB_E_ARG = -1)
    assert lib.ib_q_sample_cond(None, None, None, None, None, None, 8, 1, 1, 8, 1000, 3, 0, None) == -1
    assert lib.ib_mse_loss_partial_cond(None, 8, None, None, 8, None, 0, 1, 8, 3, 0, None) == -1
    assert lib.ib_mse_loss_finalize_cond(None, 0, None, 8, 5, None) == -1


def test_cond_cols_flag_validation():
    from inferbiomechanics_amd.cli.train import TrainCommand, check_cond_cols
    check_cond_cols("diffusion-mlp", 0)
    check_cond_cols("feedforward", 0)
    check_cond_cols("diffusion-transformer", 270, feat_dim=300)
    check_cond_cols("diffusion-transformer", 299, feat_dim=300)
    for mt, n, fd in (("feedforward", 5, None), ("groundlink", 1, None), ("diffusion-mlp", -1, None),
                      ("diffusion-mlp", 300, 300), ("diffusion-transformer", 1000, 300), ("diffusion-mlp", -3, 300)):
        with pytest.raises(SystemExit):
            check_cond_cols(mt, n, feat_dim=fd)
    parser = argparse.ArgumentParser()
    TrainCommand().register_subcommand(parser.add_subparsers(dest="command"))
    assert parser.parse_args(["train"]).cond_cols == 0
    assert parser.parse_args(["train", "--cond-cols", "270"]).cond_cols == 270


def _qs_operands(B=2, T=3, D=8, dt=torch.float32):
    x0, eps = torch.zeros(B, T, D, dtype=dt), torch.zeros(B, T, D, dtype=dt)
    t = torch.zeros(B, dtype=torch.int64)
    tab = torch.zeros(1000)
    return x0, eps, t, tab, tab.clone()


def test_q_sample_cond_binding_checks(dry):
    hip = dry
    x0, eps, t, a, s = _qs_operands()
    B, T, D = x0.shape
    lib = hip.lib()
    hip.q_sample_cond(x0, eps, t, a, s, torch.empty_like(x0), 3)
    hip.q_sample_cond(x0, eps, t, a, s, torch.empty(B * T, 12)[:, :D], D - 1)            # a padded row pitch
    hip.q_sample_cond(x0, eps, t, a, s, torch.empty_like(x0), 0)
    assert lib.calls == ["ib_q_sample_cond"] * 3
    for bad in (-1, D, D + 5):
        with pytest.raises(hip.HipError, match="cond_cols"):
            hip.q_sample_cond(x0, eps, t, a, s, torch.empty_like(x0), bad)
    with pytest.raises(hip.HipError):
        hip.q_sample_cond(x0, eps[:, :, :4], t, a, s, torch.empty_like(x0), 3)             # eps of another shape
    with pytest.raises(hip.HipError):
        hip.q_sample_cond(x0, eps, t, a, s, torch.empty(B * T, D + 1), 3)                   # x_t of another width
    with pytest.raises(hip.HipError):
        hip.q_sample_cond(x0, eps, t, a, s, torch.empty(B * T, 2 * D)[:, ::2], 3)           # inner stride 2
    with pytest.raises(hip.HipError):
        hip.q_sample_cond(x0, eps, t[:1], a, s, torch.empty_like(x0), 3)                    # one timestep per window
    with pytest.raises(hip.HipError):
        hip.q_sample_cond(x0, eps.to(BF), t, a, s, torch.empty_like(x0), 3)                 # one dtype
    with pytest.raises(hip.HipError):
        hip.q_sample_cond(x0, eps, t.to(torch.int32), a, s, torch.empty_like(x0), 3)
    assert lib.calls == ["ib_q_sample_cond"] * 3                                            # nothing else was launched


def test_mse_loss_cond_binding_checks(dry):
    hip = dry
    rows, D = 6, 8
    lib = hip.lib()
    pred, target = torch.zeros(rows, D), torch.zeros(rows, D)
    ws = torch.empty(hip.mse_loss_workspace_bytes(rows * D), dtype=torch.uint8)
    res = torch.zeros(1)
    hip.mse_loss_partial_cond(pred, target, ws, 3, dpred=torch.empty(rows, D))
    hip.mse_loss_partial_cond(torch.zeros(rows, 12)[:, :D], target, ws, 7, dpred=torch.empty(rows, 12)[:, :D])
    hip.mse_loss_partial_cond(pred, target, ws, 0)
    hip.mse_loss_finalize_cond(ws, res, rows * D, rows * (D - 3))
    assert lib.calls == ["ib_mse_loss_partial_cond"] * 3 + ["ib_mse_loss_finalize_cond"]
    for bad in (-1, D, D + 1):
        with pytest.raises(hip.HipError, match="cond_cols"):
            hip.mse_loss_partial_cond(pred, target, ws, bad)
    with pytest.raises(hip.HipError):
        hip.mse_loss_partial_cond(pred.view(-1), target, ws, 3)                             # 2-D: the columns carry the split
    with pytest.raises(hip.HipError):
        hip.mse_loss_partial_cond(pred, target[:, :4], ws, 3)
    with pytest.raises(hip.HipError):
        hip.mse_loss_partial_cond(pred, target, ws, 3, dpred=torch.empty(rows, D + 1))
    with pytest.raises(hip.HipError):
        hip.mse_loss_partial_cond(pred, target, ws, 3, dpred=torch.empty(rows, D, dtype=BF))
    with pytest.raises(hip.HipError):
        hip.mse_loss_partial_cond(pred, target, ws[:0], 3)                                  # workspace too small
    with pytest.raises(hip.HipError):
        hip.mse_loss_partial_cond(torch.zeros(rows, 2 * D)[:, ::2], target, ws, 3)
    for nl, nm in ((48, 0), (48, 49), (0, 0)):
        with pytest.raises(hip.HipError):
            hip.mse_loss_finalize_cond(ws, res, nl, nm)
    assert len(lib.calls) == 4


def _batch(B, T, D, dt, seed=1):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, T, D, generator=g).to(dt), torch.randint(0, 1000, (B,), generator=g),
            torch.randn(B, T, D, generator=g).to(dt))


def _models():
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionMLP, DiffusionTransformer
    return {
        "per-op MLP": (lambda: DiffusionMLP(30, [32, 48], temb_dim=16, temb_hidden=24), (3, 7, 30, torch.float32)),
        "chain MLP": (lambda: DiffusionMLP(48, [128, 128], temb_dim=32, temb_hidden=128, compute_dtype=BF), (5, 16, 48, BF)),
        "transformer": (lambda: DiffusionTransformer(48, 32, d_model=512, num_heads=4, dim_feedforward=1024, num_layers=3,
                                                     compute_dtype=BF), (128, 32, 48, BF)),
    }


def _step_names(hip, tr, batch):
    lib = hip.lib()
    lib.calls.clear()
    tr.step(batch)
    return list(lib.calls)


COND = {"ib_q_sample_cond", "ib_mse_loss_partial_cond", "ib_mse_loss_finalize_cond"}
PLAIN = {"ib_q_sample", "ib_mse_loss_partial", "ib_mse_loss_finalize"}


@pytest.mark.parametrize("which", ["per-op MLP", "chain MLP", "transformer"])
def test_trainer_launches(dry, which):
    """cond_cols = 0: exactly the launches of a trainer built without the argument.  cond_cols > 0: the same sequence with
    the two conditional entries in the places of q_sample / mse_loss_partial / mse_loss_finalize (per-op models), and the
    per-op sequence instead of the chain launch (bf16 MLP)"""
    from inferbiomechanics_amd._tuning import tuning as TU
    from inferbiomechanics_amd.engine import HipTrainer
    make, (B, T, D, dt) = _models()[which]
    batch = _batch(B, T, D, dt)
    torch.manual_seed(0)
    plain = _step_names(dry, HipTrainer(make(), "diffusion", "adam", 1e-3, use_graph=False), batch)
    torch.manual_seed(0)
    zero = _step_names(dry, HipTrainer(make(), "diffusion", "adam", 1e-3, use_graph=False, cond_cols=0), batch)
    assert zero == plain and not COND & set(plain)
    torch.manual_seed(0)
    tr = HipTrainer(make(), "diffusion", "adam", 1e-3, use_graph=False, cond_cols=D - 30 if D > 30 else 5)
    cond = _step_names(dry, tr, batch)
    assert COND <= set(cond) and not PLAIN & set(cond)
    assert [cond.count(n) for n in sorted(COND)] == [1, 1, 1]
    if which == "chain MLP":
        assert "ib_mlp_chain_train" in plain and "ib_mlp_chain_train" not in cond
        assert tr.plan.chain_ok(D) and not tr.plan.chain_ok(D, 1) and not tr.plan.chain_ok(D, D - 30)
        # ... the per-op sequence TU.no_chain selects, with the conditional pair in it
        old = TU.no_chain
        TU.no_chain = True
        try:
            torch.manual_seed(0)
            perop = _step_names(dry, HipTrainer(make(), "diffusion", "adam", 1e-3, use_graph=False), batch)
        finally:
            TU.no_chain = old
        plain = perop
    ren = {"ib_q_sample_cond": "ib_q_sample", "ib_mse_loss_partial_cond": "ib_mse_loss_partial",
           "ib_mse_loss_finalize_cond": "ib_mse_loss_finalize"}
    assert [ren.get(n, n) for n in cond] == plain


def test_trainer_validates_cond_cols(dry):
    from inferbiomechanics_amd.engine import HipTrainer
    from inferbiomechanics_amd.models.FeedForwardRegressionBaseline import FeedForwardBaseline
    make, (B, T, D, dt) = _models()["per-op MLP"]
    with pytest.raises(ValueError):
        HipTrainer(make(), "diffusion", "sgd", 1e-2, use_graph=False, cond_cols=-2)
    for bad in (D, D + 3):
        tr = HipTrainer(make(), "diffusion", "sgd", 1e-2, use_graph=False, cond_cols=bad)
        with pytest.raises(ValueError, match="cond_cols"):
            tr.step(_batch(B, T, D, dt))                       # D is known with the first batch
    args = argparse.Namespace(predict_grf_components=list(range(6)), predict_cop_components=list(range(6)),
                              predict_moment_components=list(range(6)), predict_wrench_components=list(range(12)))
    m = FeedForwardBaseline(23, 2, 50, "all_frames", "sigmoid", 5, 10, hidden_dims=[32])
    with pytest.raises(ValueError):
        HipTrainer(m, "regression", "sgd", 1e-2, args=args, use_graph=False, cond_cols=4)


def test_clean_observation_table_is_all_one_zero():
    from inferbiomechanics_amd.diffusion import schedule as S
    for steps, spacing in ((10, "time"), (100, "time"), (1000, "time"), (20, "logsnr"), (7, "logsnr")):
        tab = S.clean_observation_coefficients(1000, steps, spacing)
        assert tab.dtype == torch.float64 and tab.shape == S.observation_coefficients(1000, steps, spacing).shape
        assert torch.equal(tab[:, 0], torch.ones(steps + 1, dtype=torch.float64))
        assert torch.equal(tab[:, 1], torch.zeros(steps + 1, dtype=torch.float64))
    with pytest.raises(ValueError):
        S.clean_observation_coefficients(1000, 30, "time")     # the grid's own errors
    tabs = S.DiffusionTables(torch.device("cpu"))
    noised = tabs.obs_coef.clone()
    assert tabs.observations == "noised"
    assert torch.equal(noised, S.observation_coefficients(1000, 100).to(torch.float32))
    tabs.set_sampler(10, observations="clean")
    assert tabs.observations == "clean" and tabs.obs_coef.dtype == torch.float32 and tabs.obs_coef.shape == (11, 2)
    assert torch.equal(tabs.obs_coef[:, 0], torch.ones(11)) and torch.equal(tabs.obs_coef[:, 1], torch.zeros(11))
    tabs.set_sampler(10)
    assert tabs.observations == "noised"
    assert torch.equal(tabs.obs_coef, S.observation_coefficients(1000, 10).to(torch.float32))
    with pytest.raises(ValueError):
        tabs.set_sampler(10, observations="pinned")


def test_serves_distinguishes_the_observation_modes():
    from inferbiomechanics_amd.diffusion.schedule import DiffusionTables
    tabs = DiffusionTables(torch.device("cpu"))
    tabs.set_sampler(10)
    assert tabs.serves(10) and tabs.serves(10, observations="noised") and not tabs.serves(10, observations="clean")
    tabs.set_sampler(10, observations="clean")
    assert tabs.serves(10, observations="clean") and not tabs.serves(10, observations="noised")
    assert tabs.serves(10)                                     # a loop that reads no observation table does not care
    assert not tabs.serves(20, observations="clean")
    tabs.set_sampler(10, eta=0.5, observations="clean")
    assert tabs.serves(10, 0.5, observations="clean") and not tabs.serves(10, 0.5, observations="noised")
    tabs.set_sampler(10, solver="dpmpp2m", spacing="logsnr", observations="clean")
    assert tabs.serves(10, 0.0, "dpmpp2m", "logsnr", "clean") and not tabs.serves(10, 0.0, "dpmpp2m", "logsnr", "noised")


def test_sampler_modes_in_dry_run(dry):
    """the capture signature carries the table's kind, the mask is checked against model.cond_cols in clean mode only, and
    both modes issue the same launches"""
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionMLP
    B, T, D, C = 2, 6, 40, 10
    model = DiffusionMLP(D, [32, 32], temb_dim=16, temb_hidden=24)
    z, obs = torch.randn(B, T, D), torch.randn(B, T, D)
    m = torch.zeros(T, D, dtype=torch.bool)
    m[:, :C] = True
    lib = dry.lib()
    smp = ConditionalDDIMSampler(model, 10)
    assert smp.observations == "noised"
    smp.sample(z, obs, m, steps=2)
    sig_noised, calls_noised = smp._sig, list(lib.calls)
    assert "noised" in sig_noised
    smp.observations = "clean"
    with pytest.raises(ValueError, match="cond_cols"):         # model.cond_cols is 0
        smp.sample(z, obs, m, steps=2)
    model.cond_cols = C
    lib.calls.clear()
    smp.sample(z, obs, m, steps=2)
    assert smp._sig != sig_noised and "clean" in smp._sig and list(lib.calls) == calls_noised
    assert model.tables(torch.device("cpu")).observations == "clean"
    wrong = m.clone()
    wrong[:, C] = True
    with pytest.raises(ValueError, match="cond_cols"):
        smp.sample(z, obs, wrong, steps=2)
    smp.observations = "noised"
    smp.sample(z, obs, wrong, steps=2)                        # any mask, as before
    assert "noised" in smp._sig and "clean" not in smp._sig
    with pytest.raises(ValueError):
        ConditionalDDIMSampler(model, 10, observations="other")


def test_loss_evaluator_cond_cols(dry):
    from inferbiomechanics_amd.loss.DiffusionLossEvaluator import DiffusionLossEvaluator
    lib = dry.lib()
    pred, eps = torch.zeros(2, 3, 8, requires_grad=True), torch.zeros(2, 3, 8)
    ev = DiffusionLossEvaluator("dev")
    assert ev.cond_cols == 0 and ev.split == "dev"
    ev(pred, eps)
    assert lib.calls == ["ib_mse_loss"]
    lib.calls.clear()
    ev = DiffusionLossEvaluator("train", cond_cols=5)
    assert ev.cond_cols == 5
    loss = ev(pred, eps)
    assert lib.calls == ["ib_mse_loss_partial_cond", "ib_mse_loss_finalize_cond"] and len(ev.losses) == 1
    loss.backward()
    assert pred.grad is not None and pred.grad.shape == pred.shape
    assert len(lib.calls) == 3                                 # + the in-place scaling by the upstream gradient
    loss2 = ev(pred, eps)
    loss2.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="already run"):     # consume-once, as the unconditional loss
        loss2.backward()
    with pytest.raises(ValueError):
        DiffusionLossEvaluator("train", cond_cols=8)(pred, eps)
    with pytest.raises(ValueError):
        DiffusionLossEvaluator("train", cond_cols=-1)


def test_checkpoint_carries_cond_cols(tmp_path):
    from inferbiomechanics_amd.cli.abstract_command import AbstractCommand
    from inferbiomechanics_amd.cli.train import save_checkpoint
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionMLP

    class Opt:
        def state_dict(self):
            return {}

    make = lambda: DiffusionMLP(40, [32], temb_dim=16, temb_hidden=24)
    m = make()
    assert m.cond_cols == 0
    d0, d1 = str(tmp_path / "plain"), str(tmp_path / "cond")
    assert set(torch.load(save_checkpoint(d0, 0, 1, m, Opt()))) == {"epoch", "model_state_dict", "optimizer_state_dict"}
    m.cond_cols = 10
    saved = torch.load(save_checkpoint(d1, 0, 1, m, Opt()))
    assert saved["cond_cols"] == 10
    cmd = AbstractCommand()
    fresh = make()
    cmd.load_latest_checkpoint(fresh, checkpoint_dir=d1)
    assert fresh.cond_cols == 10
    cmd.load_latest_checkpoint(fresh, checkpoint_dir=d0)       # no key: 0
    assert fresh.cond_cols == 0
