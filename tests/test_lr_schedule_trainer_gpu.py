"""The learning-rate schedule in the fused trainer (HipTrainer(lr_schedule=...)) on the GPU: 20 steps of a cosine schedule
with w = 5, T = 15, m = 0.1 -- warmup, decay and the clamp beyond T -- replayed from the captured hipGraph after the first
two steps, so the rate of a step can only come from the device step counter.

The yardstick is code older than the schedule: a second trainer with use_graph=False and no schedule, whose `lr` attribute
the test sets to LrSchedule.lr_at(base, k) before step k.

  * losses and the flat parameters after every step are bitwise equal between the two (with ema_decay = 0.999 on one model,
    the EMA too);
  * a checkpoint taken at step 10 and loaded into a fresh scheduled trainer continues bitwise;
  * lr_schedule=None and a constant schedule without warmup record the launch names of a trainer built without the argument
    and train bitwise the same 20 steps;
  * current_lr() equals the device probe's value for the next step.

Models: MLP denoiser per-op (fp32) and chain kernel (bf16), transformer denoiser small and at the headline shape (bf16,
B = 256, T = 50), the regression feedforward.  -m gpu."""
import argparse

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
STEPS = 20
W, T_TOTAL, M = 5, 15, 0.1


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def sched():
    from inferbiomechanics_amd.lr_schedule import LrSchedule
    return LrSchedule("cosine", W, T_TOTAL, M)


def reg_args():
    return argparse.Namespace(predict_grf_components=list(range(6)), predict_cop_components=list(range(6)),
                              predict_moment_components=list(range(6)), predict_wrench_components=list(range(12)))


def _diff_batches(B, T, D, dt):
    def make(n, seed=5):
        g = torch.Generator().manual_seed(seed)
        return [(torch.randn(B, T, D, generator=g).to(DEV, dt), torch.randint(0, 1000, (B,), generator=g).to(DEV),
                 torch.randn(B, T, D, generator=g).to(DEV, dt)) for _ in range(n)]
    return make


def _reg_batches(n, seed=5):
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import SyntheticWindowDataset
    ds = SyntheticWindowDataset(8 * n, 50, 5, seed=seed)
    out = []
    for i in range(n):
        inputs, labels, _, _ = torch.utils.data.default_collate([ds[8 * i + j] for j in range(8)])
        out.append(({k: v.to(DEV) for k, v in inputs.items()}, {k: v.to(DEV) for k, v in labels.items()}))
    return out


def _model(name):
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionMLP, DiffusionTransformer
    from inferbiomechanics_amd.models.FeedForwardRegressionBaseline import FeedForwardBaseline
    torch.manual_seed(7)
    bf, f32 = torch.bfloat16, torch.float32
    if name == "mlp_perop_fp32":
        return DiffusionMLP(44, [64, 96], temb_dim=32, temb_hidden=48, device=DEV), "diffusion", "adam", _diff_batches(8, 10, 44, f32)
    if name == "mlp_chain_bf16":
        return DiffusionMLP(48, [128, 128], temb_dim=32, temb_hidden=128, device=DEV, compute_dtype=bf), "diffusion", "adam", \
            _diff_batches(6, 16, 48, bf)
    if name == "transformer_small_bf16":
        return DiffusionTransformer(48, 32, d_model=512, num_heads=8, dim_feedforward=512, num_layers=2, device=DEV,
                                    compute_dtype=bf), "diffusion", "adam", _diff_batches(128, 32, 48, bf)
    if name == "transformer_headline_bf16":
        return DiffusionTransformer(300, 50, d_model=512, num_heads=8, dim_feedforward=2048, num_layers=4, device=DEV,
                                    compute_dtype=bf), "diffusion", "rmsprop", _diff_batches(256, 50, 300, bf)
    assert name == "feedforward_fp32"
    return FeedForwardBaseline(23, 2, 50, 'all_frames', 'sigmoid', 5, 10, hidden_dims=[64, 32], device=DEV), "regression", \
        "sgd", lambda n, seed=5: _reg_batches(n, seed)


MODELS = ["mlp_perop_fp32", "mlp_chain_bf16", "transformer_small_bf16", "transformer_headline_bf16", "feedforward_fp32"]


def _trainer(name, use_graph=True, **kw):
    from inferbiomechanics_amd.engine import HipTrainer
    model, task, opt, mk = _model(name)
    lr = 1e-2 if opt == "sgd" else 1e-3
    tr = HipTrainer(model, task, opt, lr, args=reg_args() if task == "regression" else None, use_graph=use_graph, **kw)
    if name == "mlp_chain_bf16":
        assert tr.plan.chain_ok(48)
    return tr, mk, lr


def _bits(t):
    return t.view(torch.int32)


def _run(tr, batches, host_rates=None, first=1):
    """losses, flat parameters and EMA after every step; host_rates: the yardstick -- tr.lr is set before each step"""
    losses, flats, emas = [], [], []
    for k, b in enumerate(batches):
        if host_rates is not None:
            tr.lr = host_rates(first + k)
        tr.step(b)
        torch.cuda.synchronize()
        losses.append(tr.loss_value())
        flats.append(tr.flat.detach().cpu().clone())
        emas.append(None if tr.ema is None else tr.ema.detach().cpu().clone())
    return losses, flats, emas


def _same(a, b, what):
    (la, fa, ea), (lb, fb, eb) = a, b
    assert la == lb, (what, la, lb)
    for k in range(len(fa)):
        assert torch.equal(_bits(fa[k]), _bits(fb[k])), (what, "parameters after step", k + 1)
        assert (ea[k] is None) == (eb[k] is None)
        if ea[k] is not None:
            assert torch.equal(_bits(ea[k]), _bits(eb[k])), (what, "ema after step", k + 1)


@pytest.mark.parametrize("name", MODELS)
def test_scheduled_graph_replay_is_the_host_set_rate_step_by_step(name):
    from inferbiomechanics_amd import hip
    sch = sched()
    ref, mk, base = _trainer(name, use_graph=False)
    batches = mk(STEPS)
    want = _run(ref, batches, host_rates=lambda k: sch.lr_at(base, k))
    del ref
    tr, _, _ = _trainer(name, lr_schedule=sch)
    probe = hip.lr_schedule_eval(base, sch, torch.arange(1, STEPS + 2, dtype=torch.int32, device=DEV)).cpu()
    losses, flats, emas = [], [], []
    for k, b in enumerate(batches):
        assert tr.current_lr() == float(probe[k]), (name, k + 1)          # the rate of the step about to run
        tr.step(b)
        torch.cuda.synchronize()
        losses.append(tr.loss_value())
        flats.append(tr.flat.detach().cpu().clone())
        emas.append(None)
    assert tr._rec is not None, "the step was captured into a hipGraph: the later steps were replays"
    assert tr.lr == base and tr.current_lr() == float(probe[STEPS]) == sch.lr_at(base, T_TOTAL), "the floor, m lr"
    _same((losses, flats, emas), want, name)
    # the schedule did something: the same run at the constant base rate differs from the first step on (lr / 5 there)
    plain, _, _ = _trainer(name)
    plain.step(batches[0])
    torch.cuda.synchronize()
    assert not torch.equal(plain.flat.cpu(), flats[0]), name


def test_scheduled_run_with_the_ema_is_bitwise_too():
    name, sch = "transformer_small_bf16", sched()
    ref, mk, base = _trainer(name, use_graph=False, ema_decay=0.999)
    batches = mk(STEPS)
    want = _run(ref, batches, host_rates=lambda k: sch.lr_at(base, k))
    del ref
    tr, _, _ = _trainer(name, lr_schedule=sch, ema_decay=0.999)
    got = _run(tr, batches)
    assert tr._rec is not None and got[2][-1] is not None and not torch.equal(got[2][-1], got[1][-1])
    _same(got, want, name)


def test_checkpoint_at_step_10_continues_bitwise(tmp_path):
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.cli.abstract_command import AbstractCommand
    from inferbiomechanics_amd.cli.train import save_checkpoint
    from inferbiomechanics_amd.lr_schedule import LrSchedule
    name, sch = "mlp_perop_fp32", sched()
    whole, mk, base = _trainer(name, lr_schedule=sch)
    batches = mk(STEPS)
    want = _run(whole, batches)
    first, _, _ = _trainer(name, lr_schedule=sch)
    _run(first, batches[:10])
    d = str(tmp_path / "ck")
    save_checkpoint(d, 0, 9, first.model, first)
    saved = torch.load(f"{d}/epoch_0_batch_9.pt", map_location="cpu")["optimizer_state_dict"]
    assert saved["lr_schedule"] == sch.fields() and saved["lr"] == base and saved["step"] == 10
    resumed, _, _ = _trainer(name, lr_schedule=sched())
    assert AbstractCommand().load_latest_checkpoint(resumed.model, optimizer=resumed, checkpoint_dir=d) == (0, 9)
    assert int(resumed.step_dev.cpu()) == 10 and resumed.current_lr() == sch.lr_at(base, 11)
    got = _run(resumed, batches[10:])
    _same(got, tuple(x[10:] for x in want), name)
    other, _, _ = _trainer(name, lr_schedule=LrSchedule("cosine", W, T_TOTAL + 1, M))
    with pytest.raises(hip.HipError, match="differs"):
        AbstractCommand().load_latest_checkpoint(other.model, optimizer=other, checkpoint_dir=d)


@pytest.mark.parametrize("name", ["mlp_chain_bf16", "transformer_small_bf16"])
def test_schedule_off_is_todays_trainer(name):
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.lr_schedule import LrSchedule

    def run(**kw):
        tr, mk, _ = _trainer(name, **kw)
        batches = mk(STEPS)
        with hip.record_launches() as rec:
            tr.step(batches[0])
        torch.cuda.synchronize()
        names = [n for n, _ in rec.calls]
        first = (tr.loss_value(), tr.flat.detach().cpu().clone())
        losses, flats, emas = _run(tr, batches[1:])
        assert tr._rec is not None
        return names, ([first[0]] + losses, [first[1]] + flats, [None] + emas)
    names_today, today = run()
    assert not any(n.endswith("_sched") for n in names_today) and any(n.startswith("ib_optim_step") for n in names_today)
    for off in (None, LrSchedule("constant", 0, 0, 0.0), LrSchedule("constant", 0, 1000, 0.5)):
        names, got = run(lr_schedule=off)
        assert names == names_today, (name, off)
        _same(got, today, (name, off))
    names_on, _ = run(lr_schedule=sched())
    assert [n[:-len("_sched")] if n.endswith("_sched") else n for n in names_on] == \
        [n[:-len("_ema")] if n.endswith("_ema") else n for n in names_today], "the same launches, scheduled"
    assert sum(n.endswith("_sched") for n in names_on) == sum(n.startswith("ib_optim_step") for n in names_today)
