"""Clipping to a global gradient norm in the fused trainer (HipTrainer(max_grad_norm=...)) on the GPU, 6 steps, bitwise.

The yardstick is the step form older than the clip: a trainer with max_grad_norm = 0 built and run with the tuning switches
no_opt_fuse and no_early_opt on, so that its whole gradient is in `trainer.grad` before its one optimizer launch.

  * max_grad_norm = inf is that trainer: loss and flat parameters bitwise equal after every step, and grad_norm() within
    1 fp32 ulp of float32(sqrt(sum(float64(grad)^2))) of its gradient;
  * a finite max_grad_norm below the first step's norm: the graph-replayed and the use_graph=False run equal, bitwise, the
    yardstick whose `hip.optim_step` the test wraps to pass grad_scale = gs, gs read from the probe (ib_grad_norm_eval) on
    that step's gradient; Adam, and Adam with cosine schedule, EMA and weight decay; clip_coef() < 1 on step 1;
  * max_grad_norm = 0 is today's trainer: the same launch names, bitwise the same steps;
  * a checkpoint taken mid-run continues bitwise; another value is refused.  -m gpu."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
STEPS = 6
WD = 0.1
INF = float("inf")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def sched():
    from inferbiomechanics_amd.lr_schedule import LrSchedule
    return LrSchedule("cosine", 2, 5, 0.1)               # six steps: warmup, peak, decay, floor


def _diff_batches(B, T, D, dt):
    def make(n, seed=5):
        g = torch.Generator().manual_seed(seed)
        return [(torch.randn(B, T, D, generator=g).to(DEV, dt), torch.randint(0, 1000, (B,), generator=g).to(DEV),
                 torch.randn(B, T, D, generator=g).to(DEV, dt)) for _ in range(n)]
    return make


def _model(name):
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionMLP, DiffusionTransformer
    torch.manual_seed(7)
    if name == "mlp_perop_fp32":
        return DiffusionMLP(44, [64, 96], temb_dim=32, temb_hidden=48, device=DEV), _diff_batches(8, 10, 44, torch.float32)
    assert name == "transformer_small_bf16"
    return DiffusionTransformer(48, 32, d_model=512, num_heads=8, dim_feedforward=512, num_layers=2, device=DEV,
                                compute_dtype=torch.bfloat16), _diff_batches(128, 32, 48, torch.bfloat16)


MODELS = ["mlp_perop_fp32", "transformer_small_bf16"]
VARIANTS = {"adam": {}, "adam_cosine_ema_decay": {"lr_schedule": sched(), "ema_decay": 0.999, "weight_decay": WD}}


def _trainer(name, use_graph=True, **kw):
    from inferbiomechanics_amd.engine import HipTrainer
    model, mk = _model(name)
    return HipTrainer(model, "diffusion", "adam", 1e-3, use_graph=use_graph, **kw), mk


def _bits(t):
    return t.view(torch.int32)


def _run(tr, batches, after=None):
    losses, flats, emas = [], [], []
    for b in batches:
        tr.step(b)
        torch.cuda.synchronize()
        losses.append(tr.loss_value())
        flats.append(tr.flat.detach().cpu().clone())
        emas.append(None if tr.ema is None else tr.ema.detach().cpu().clone())
        if after is not None:
            after(tr)
    return losses, flats, emas


def _same(a, b, what):
    (la, fa, ea), (lb, fb, eb) = a, b
    assert la == lb, (what, la, lb)
    for k in range(len(fa)):
        assert torch.equal(_bits(fa[k]), _bits(fb[k])), (what, "parameters after step", k + 1,
                                                         int((_bits(fa[k]) != _bits(fb[k])).sum()))
        assert (ea[k] is None) == (eb[k] is None)
        if ea[k] is not None:
            assert torch.equal(_bits(ea[k]), _bits(eb[k])), (what, "ema after step", k + 1)


def ulps(a, b):
    ia, ib = (int(np.float32(v).view(np.int32)) for v in (a, b))
    return abs(ia - ib)


def materialised(name, batches, monkeypatch, max_norm=None, **kw):
    """the run of a trainer without the clip in the materialised step form (no_opt_fuse + no_early_opt) -> its results, the
    float32 norm of its gradient after every step and, with max_norm, the coefficients the wrapped launch used"""
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd._tuning import tuning as TU
    norms, coefs = [], []
    real = hip.optim_step

    def wrapped(opt_, p, g, *a, **k):
        assert p.numel() == ref.flat.numel() and k.get("sources") is None and k.get("max_grad_norm", 0.0) == 0.0
        _, stats = hip.grad_norm_eval(hip.grad_sumsq(g), k["grad_scale"], max_norm)
        stats = stats.cpu()
        coefs.append(float(stats[1]))
        k["grad_scale"] = float(stats[2])
        return real(opt_, p, g, *a, **k)
    with monkeypatch.context() as mp:
        mp.setattr(TU, "no_opt_fuse", True)
        mp.setattr(TU, "no_early_opt", True)
        if max_norm is not None:
            mp.setattr(hip, "optim_step", wrapped)
        ref, _ = _trainer(name, use_graph=False, **kw)
        out = _run(ref, batches, after=lambda tr: norms.append(
            float(np.float32(math.sqrt(float((tr.grad.detach().cpu().double() ** 2).sum()))))))
    return out, norms, coefs


@pytest.fixture(scope="module")
def first_norm():
    """the norm of the first step's gradient per model, measured by a max_grad_norm = inf trainer"""
    out = {}
    for name in MODELS:
        tr, mk = _trainer(name, max_grad_norm=INF)
        tr.step(mk(1)[0])
        torch.cuda.synchronize()
        out[name] = tr.grad_norm()
        assert out[name] > 0 and tr.clip_coef() == 1.0
    return out


@pytest.mark.parametrize("name", MODELS)
def test_measuring_only_is_the_materialised_trainer(name, monkeypatch):
    _, mk = _model(name)
    batches = mk(STEPS)
    want, norms, _ = materialised(name, batches, monkeypatch)
    seen = []
    tr, _ = _trainer(name, max_grad_norm=INF)
    got = _run(tr, batches, after=lambda t: seen.append((t.grad_norm(), t.clip_coef())))
    assert tr._rec is not None, "the later steps were replays of the captured graph"
    _same(got, want, name)
    print("norms:", [s[0] for s in seen], "host:", norms)
    for (norm, coef), ref in zip(seen, norms):
        assert ulps(norm, ref) <= 1 and coef == 1.0, (name, norm, ref, coef)
    assert len(set(s[0] for s in seen)) > 1, "the norm follows the replayed steps"


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_clipped_trainer_is_the_materialised_trainer_with_the_probes_scale(name, variant, first_norm, monkeypatch):
    kw = VARIANTS[variant]
    _, mk = _model(name)
    batches = mk(STEPS)
    max_norm = float(np.float32(0.5 * first_norm[name]))
    want, _, coefs = materialised(name, batches, monkeypatch, max_norm=max_norm, **kw)
    assert len(coefs) == STEPS and coefs[0] < 1.0, coefs
    for use_graph in (True, False):
        seen = []
        tr, _ = _trainer(name, use_graph=use_graph, max_grad_norm=max_norm, **kw)
        got = _run(tr, batches, after=lambda t: seen.append(t.clip_coef()))
        assert (tr._rec is not None) == use_graph
        _same(got, want, (name, variant, use_graph))
        assert seen == coefs and seen[0] < 1.0, (seen, coefs)
    plain, _ = _trainer(name, **kw)
    plain.step(batches[0])
    torch.cuda.synchronize()
    assert not torch.equal(plain.flat.cpu(), want[1][0]), "the clip did something"


@pytest.mark.parametrize("name", MODELS)
def test_max_grad_norm_zero_is_todays_trainer(name):
    from inferbiomechanics_amd import hip

    def run(**kw):
        tr, mk = _trainer(name, **kw)
        batches = mk(STEPS)
        with hip.record_launches() as rec:
            tr.step(batches[0])
        torch.cuda.synchronize()
        names = [n for n, _ in rec.calls]
        first = (tr.loss_value(), tr.flat.detach().cpu().clone())
        losses, flats, emas = _run(tr, batches[1:])
        assert tr._rec is not None
        return names, ([first[0]] + losses, [first[1]] + flats, [None] + emas), tr
    names_today, today, _ = run()
    new = lambda n: n.startswith("ib_grad_") or n == "ib_optim_step_gradnorm"
    assert not any(new(n) for n in names_today) and any(n.startswith("ib_optim_step") for n in names_today)
    names, got, tr = run(max_grad_norm=0.0)
    assert names == names_today and tr.norm_slots is None and tr.norm_stats is None
    _same(got, today, name)
    names_on, _, _ = run(max_grad_norm=1.0)
    assert names_on[-2:] == ["ib_grad_sumsq", "ib_optim_step_gradnorm"] and sum(new(n) for n in names_on) == 2
    assert sum(n.startswith("ib_optim_step") for n in names_on) == 1 and not any("_sources" in n for n in names_on)


def test_checkpoint_mid_run_continues_bitwise(tmp_path, first_norm):
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.cli.abstract_command import AbstractCommand
    from inferbiomechanics_amd.cli.train import save_checkpoint
    name = "mlp_perop_fp32"
    mgn = float(np.float32(0.5 * first_norm[name]))
    kw = dict(VARIANTS["adam_cosine_ema_decay"], max_grad_norm=mgn)
    whole, mk = _trainer(name, **kw)
    batches = mk(STEPS)
    want = _run(whole, batches)
    first, _ = _trainer(name, **kw)
    _run(first, batches[:3])
    d = str(tmp_path / "ck")
    save_checkpoint(d, 0, 2, first.model, first)
    saved = torch.load(f"{d}/epoch_0_batch_2.pt", map_location="cpu")["optimizer_state_dict"]
    assert saved["max_grad_norm"] == first.max_grad_norm == mgn and saved["step"] == 3
    resumed, _ = _trainer(name, **kw)
    assert AbstractCommand().load_latest_checkpoint(resumed.model, optimizer=resumed, checkpoint_dir=d) == (0, 2)
    lg, fg, _ = _run(resumed, batches[3:])
    assert lg == want[0][3:]
    for k in range(3):
        assert torch.equal(_bits(fg[k]), _bits(want[1][3 + k])), ("parameters after step", 4 + k)
    for other in (2 * mgn, 0.0, INF):
        t2, _ = _trainer(name, **dict(kw, max_grad_norm=other))
        with pytest.raises(hip.HipError, match="gradient-norm clip"):
            AbstractCommand().load_latest_checkpoint(t2.model, optimizer=t2, checkpoint_dir=d)
