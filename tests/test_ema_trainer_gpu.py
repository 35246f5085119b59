"""The EMA of the weights in the fused trainer (HipTrainer(ema_decay=D)) on the GPU, 20 steps, graph-replayed after the
first two:

  * losses and the flat parameters are bitwise those of the same run without the EMA;
  * after every step the EMA is within 1e-6 * max|p| of a float64 recurrence over the recorded parameter trajectory,
    e_k = d_k e_(k-1) + (1 - d_k) p_k with the warmup decay of step k (D = 0.5 without warmup: a range updated twice or
    never in a step is off by a factor of two);
  * graph replay and eager launches give bitwise the same EMA;
  * a checkpoint written at step 10 and resumed continues bitwise as the uninterrupted run; a checkpoint without EMA
    starts the EMA from the loaded weights.

Models: MLP denoiser per-op (fp32, bf16) and chain kernel (bf16), transformer denoiser small and at the headline shape
(bf16, B = 256, T = 50), the regression feedforward.  -m gpu."""
import argparse

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
STEPS = 20


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def reg_args():
    return argparse.Namespace(predict_grf_components=list(range(6)), predict_cop_components=list(range(6)),
                              predict_moment_components=list(range(6)), predict_wrench_components=list(range(12)))


# name: (builder, task, optimizer, batch maker)
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
    if name == "mlp_perop_bf16":
        return DiffusionMLP(44, [64, 96], temb_dim=32, temb_hidden=48, device=DEV, compute_dtype=bf), "diffusion", "rmsprop", \
            _diff_batches(8, 10, 44, bf)
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


MODELS = ["mlp_perop_fp32", "mlp_perop_bf16", "mlp_chain_bf16", "transformer_small_bf16", "transformer_headline_bf16",
          "feedforward_fp32"]


def _trainer(name, use_graph=True, **kw):
    from inferbiomechanics_amd.engine import HipTrainer
    model, task, opt, mk = _model(name)
    lr = 1e-2 if opt == "sgd" else 1e-3
    tr = HipTrainer(model, task, opt, lr, args=reg_args() if task == "regression" else None, use_graph=use_graph, **kw)
    if name == "mlp_chain_bf16":
        assert tr.plan.chain_ok(48)
    return tr, mk


def _run(tr, batches, record=False):
    losses, flats, emas = [], [], []
    for b in batches:
        tr.step(b)
        torch.cuda.synchronize()
        losses.append(tr.loss_value())
        if record:
            flats.append(tr.flat.detach().cpu().clone())
            emas.append(None if tr.ema is None else tr.ema.detach().cpu().clone())
    torch.cuda.synchronize()
    return losses, flats, emas


def _decay(D, warmup, step):
    return float(np.float32(min(D, (1.0 + step) / (10.0 + step)) if warmup else D))


@pytest.mark.parametrize("name", MODELS)
def test_ema_follows_the_parameter_trajectory(name):
    base, mk = _trainer(name)
    batches = mk(STEPS)
    ref_losses, ref_flats, _ = _run(base, batches, record=True)
    assert base._rec is not None                                   # the step was captured into a hipGraph
    p0 = None
    for D, warmup in ((0.9, True), (0.5, False)):
        tr, _ = _trainer(name, ema_decay=D, ema_warmup=warmup)
        e = tr.ema.detach().cpu().double().clone()
        if p0 is None:
            p0 = tr.flat.detach().cpu().clone()
        assert torch.equal(tr.ema.cpu(), p0)
        losses, flats, emas = _run(tr, batches, record=True)
        assert losses == ref_losses, (name, D)                     # the EMA does not touch the step
        for k in range(STEPS):
            assert torch.equal(flats[k].view(torch.int32), ref_flats[k].view(torch.int32)), (name, D, k)
            d = _decay(D, warmup, k + 1)
            e = d * e + float(np.float32(1.0) - np.float32(d)) * flats[k].double()
            err = float((emas[k].double() - e).abs().max())
            assert err <= 1e-6 * float(flats[k].abs().max()), (name, D, warmup, k, err)
        # eager launches, same EMA bit for bit
        eager, _ = _trainer(name, use_graph=False, ema_decay=D, ema_warmup=warmup)
        _, _, emas_e = _run(eager, batches[:6], record=True)
        for k in range(6):
            assert torch.equal(emas_e[k].view(torch.int32), emas[k].view(torch.int32)), (name, D, "eager", k)
        del tr, eager


def test_checkpoint_round_trip_is_bitwise(tmp_path):
    from inferbiomechanics_amd.cli.abstract_command import AbstractCommand
    from inferbiomechanics_amd.cli.train import save_checkpoint
    name = "mlp_perop_fp32"
    whole, mk = _trainer(name, ema_decay=0.9)
    batches = mk(STEPS)
    _run(whole, batches)
    first, _ = _trainer(name, ema_decay=0.9)
    _run(first, batches[:10])
    d = str(tmp_path / "ck")
    save_checkpoint(d, 0, 9, first.model, first)
    resumed, _ = _trainer(name, ema_decay=0.9)
    assert AbstractCommand().load_latest_checkpoint(resumed.model, optimizer=resumed, checkpoint_dir=d) == (0, 9)
    assert torch.equal(resumed.ema, first.ema) and int(resumed.step_dev.cpu()) == 10
    _run(resumed, batches[10:])
    assert torch.equal(resumed.flat.view(torch.int32), whole.flat.view(torch.int32))
    assert torch.equal(resumed.ema.view(torch.int32), whole.ema.view(torch.int32))
    # a checkpoint without EMA: the EMA starts from the loaded weights
    plain, _ = _trainer(name)
    _run(plain, batches[:3])
    d2 = str(tmp_path / "plain")
    save_checkpoint(d2, 0, 2, plain.model, plain)
    assert set(torch.load(f"{d2}/epoch_0_batch_2.pt")) == {'epoch', 'model_state_dict', 'optimizer_state_dict'}
    again, _ = _trainer(name, ema_decay=0.99)
    AbstractCommand().load_latest_checkpoint(again.model, optimizer=again, checkpoint_dir=d2)
    assert torch.equal(again.ema, plain.flat) and torch.equal(again.flat, plain.flat)
