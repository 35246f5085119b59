"""HipTrainer(loss_weight=LossWeight(...)): the diffusion step with its loss weighted by each window's noise level.

A table of ones is the trainer without a weight bit for bit (parameters and optimizer state; transformer fp32 / bf16, graph and
no graph, cond_cols 0 and 14; the bf16 MLP denoiser against the unweighted trainer with the chain kernel switched off, since a
weighted step takes the per-op path).  Min-SNR (gamma = 5) is held against a float64 autograd restatement of
mean(w_t (eps_hat - eps)^2) built as tests/test_cond_trainer_gpu.py builds its reference, within that file's bounds: fp32 the
loss within 1e-3 and every parameter within 2e-3 max|e| + 2e-5; bf16 the loss within 2 %.  Runs are bitwise reproducible, graph
replay equals the uncaptured step, level_loss() equals the host's recomputation from the batches' t, step_drawn agrees with
step on the drawn batch.  -m gpu."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as R  # noqa: E402
from oracle.fixture_inputs import det_state  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
LR = 1e-2
B, T, D = 8, 12, 44
NB = 8


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def load_det(module):
    sd = module.state_dict()
    new = det_state({k: tuple(v.shape) for k, v in sd.items()})
    module.load_state_dict({k: v.to(sd[k].dtype) for k, v in new.items()})


def batches(n, dtype, seed=0):
    """t mixes low noise levels (SNR above gamma = 5: weight below 1) with levels drawn over the whole range"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        t = torch.randint(0, 1000, (B,), generator=g)
        t[:4] = torch.randint(0, 60, (4,), generator=g)
        out.append((torch.randn(B, T, D, generator=g).to(dtype), t, torch.randn(B, T, D, generator=g).to(dtype)))
    return out


def make(kind, dtype):
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionMLP, DiffusionTransformer
    if kind == "transformer":
        torch.manual_seed(0)
        m = DiffusionTransformer(D, T, d_model=128, num_heads=4, dim_feedforward=256, num_layers=2, device=DEV,
                                 compute_dtype=dtype)
        fwd = lambda p, x, t: R.denoiser_transformer_forward(p, x, t, 2, 4)
    else:
        m = DiffusionMLP(D, [128, 128], temb_dim=32, temb_hidden=128, device=DEV, compute_dtype=dtype)
        load_det(m)
        fwd = lambda p, x, t: R.denoiser_mlp_forward(p, x, t, [128, 128], temb_dim=32)
    return m, fwd


def min_snr64(gamma=5.0, n=1000):
    """the closed form in float64, written here: min(1, gamma / snr), snr = ab / (1 - ab), linear betas 1e-4 .. 0.02"""
    ab = torch.cumprod(1.0 - torch.linspace(1e-4, 0.02, n, dtype=torch.float64), dim=0)
    return torch.minimum(torch.ones_like(ab), gamma * (1.0 - ab) / ab)


def ones_weight():
    from inferbiomechanics_amd.loss_weight import LossWeight
    return LossWeight("table", table=np.ones(1000))


def reference_run(p0, fwd, bs, C, steps, dtype, w64):
    """float64 SGD over mean(w_t (eps_hat - eps)^2) on the free columns.  bf16: the forward reads the matrices rounded to
    bf16 (the trainer's shadow of its fp32 master weights), the gradient goes to the master"""
    p = {k: v.clone().requires_grad_(True) for k, v in p0.items()}
    tabs = R.schedule_tables()
    losses, plain = [], []
    for i in range(steps):
        x0, t, eps = (a.double() if a.is_floating_point() else a for a in bs[i % len(bs)])
        for v in p.values():
            v.grad = None
        xt = R.q_sample(x0, t, eps, tabs)
        xt = torch.cat([x0[..., :C], xt[..., C:]], dim=-1)
        if dtype == BF:
            xt = xt.to(BF).double()
            pf = {k: (v + (v.detach().to(BF).double() - v.detach())) if v.dim() >= 2 else v for k, v in p.items()}
        else:
            pf = p
        pred = fwd(pf, xt, t)
        sq = (pred[..., C:] - eps[..., C:]) ** 2
        loss = (w64[t][:, None, None] * sq).mean()
        loss.backward()
        losses.append(float(loss))
        plain.append(float(sq.mean()))
        with torch.no_grad():
            for v in p.values():
                v -= LR * v.grad
    return losses, plain, {k: v.detach() for k, v in p.items()}


@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("kind,dtype,C", [("transformer", torch.float32, 0), ("transformer", torch.float32, 14),
                                          ("transformer", BF, 14), ("mlp", BF, 0)])
def test_min_snr_step_matches_float64(kind, dtype, C, steps):
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.engine import HipTrainer
    from inferbiomechanics_amd.loss_weight import LossWeight
    model, fwd = make(kind, dtype)
    p0 = {k: v.detach().cpu().double().clone() for k, v in model.state_dict().items()}
    bs = batches(3, dtype, seed=7)
    ref_losses, ref_plain, ref_p = reference_run(p0, fwd, bs, C, steps, dtype, min_snr64())
    tr = HipTrainer(model, "diffusion", "sgd", LR, use_graph=False, cond_cols=C, loss_weight=LossWeight("min_snr", gamma=5.0))
    if kind == "mlp":
        assert tr.plan.chain_ok(D) and not tr.plan.chain_ok(D, 0, weighted=True), "the weighted MLP step leaves the chain kernel"
    got, plain = [], []
    with hip.record_launches() as rec:
        for i in range(steps):
            x0, t, eps = bs[i % len(bs)]
            tr.step((x0.to(DEV), t.to(DEV), eps.to(DEV)))
            got.append(tr.loss_value())
            plain.append(float(tr.result[1].cpu()))
    names = [n for n, _ in rec.calls]
    assert names.count("ib_mse_loss_weighted_partial") == steps == names.count("ib_mse_loss_weighted_finalize")
    assert not {"ib_mse_loss_partial", "ib_mse_loss_finalize", "ib_mse_loss_partial_cond", "ib_mse_loss_finalize_cond",
                "ib_mlp_chain_train"} & set(names), names
    lt = 1e-3 if dtype == torch.float32 else 2e-2
    print(kind, dtype, C, "weighted", got, "float64", ref_losses, "unweighted", plain, "float64", ref_plain)
    for a, e, pa, pe in zip(got, ref_losses, plain, ref_plain):
        assert abs(a - e) <= lt * abs(e), (got, ref_losses)
        assert abs(pa - pe) <= lt * abs(pe), (plain, ref_plain)
        assert a < 0.95 * pa, "the weights of the low noise levels must show in the optimised loss"
    if dtype == torch.float32:
        for k, v in model.state_dict().items():
            a, e = v.detach().cpu().double(), ref_p[k]
            err = (a - e).abs().max().item()
            assert err <= 2e-3 * max(e.abs().max().item(), 1e-6) + 2e-5, (k, err)


def _run(kw, use_graph, dtype, steps=6, kind="transformer"):
    from inferbiomechanics_amd.engine import HipTrainer
    model, _ = make(kind, dtype)
    tr = HipTrainer(model, "diffusion", "adam", 1e-3, use_graph=use_graph, **kw)
    bs = batches(3, dtype, seed=11)
    losses = []
    for i in range(steps):
        x0, t, eps = bs[i % 3]
        tr.step((x0.to(DEV), t.to(DEV), eps.to(DEV)))
        losses.append((tr.loss_value(), float(tr.result[1].cpu()) if tr.loss_weight is not None else None))
    torch.cuda.synchronize()
    return losses, tr.flat.detach().clone(), tr.s1.detach().clone(), tr.s2.detach().clone(), tr, bs


@pytest.mark.parametrize("C", [0, 14])
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_ones_table_is_the_unweighted_transformer_trainer_bitwise(dtype, use_graph, C):
    a = _run({"cond_cols": C}, use_graph, dtype)
    b = _run({"cond_cols": C, "loss_weight": ones_weight()}, use_graph, dtype)
    for x, y in zip(a[1:4], b[1:4]):
        assert torch.equal(x, y)
    for (la, _), (lw, lu) in zip(a[0], b[0]):
        assert lw == lu and abs(lu - la) <= 1e-5 * abs(la)
    if use_graph:
        assert b[4]._rec is not None, "the weighted step was never captured"


@pytest.mark.parametrize("use_graph", [False, True])
def test_ones_table_is_the_per_op_mlp_trainer_bitwise(use_graph, monkeypatch):
    from inferbiomechanics_amd._tuning import tuning as TU
    b = _run({"loss_weight": ones_weight()}, use_graph, BF, kind="mlp")
    monkeypatch.setattr(TU, "no_chain", True, raising=False)       # the yardstick takes the per-op path too
    a = _run({}, use_graph, BF, kind="mlp")
    assert not a[4].plan.chain_ok(D)
    for x, y in zip(a[1:4], b[1:4]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("kind,dtype", [("transformer", BF), ("mlp", BF), ("transformer", torch.float32)])
def test_weighted_runs_are_bitwise_reproducible(kind, dtype, use_graph):
    from inferbiomechanics_amd.loss_weight import LossWeight
    a = _run({"cond_cols": 14, "loss_weight": LossWeight("min_snr")}, use_graph, dtype, kind=kind)
    b = _run({"cond_cols": 14, "loss_weight": LossWeight("min_snr")}, use_graph, dtype, kind=kind)
    assert a[0] == b[0]
    for x, y in zip(a[1:4], b[1:4]):
        assert torch.equal(x, y)
    c = _run({"cond_cols": 14}, use_graph, dtype, kind=kind)
    assert not torch.equal(a[1], c[1]), "the weighted run must differ from the unweighted one"


def test_graph_replay_equals_the_uncaptured_step():
    from inferbiomechanics_amd.loss_weight import LossWeight
    a = _run({"loss_weight": LossWeight("min_snr")}, False, BF)
    b = _run({"loss_weight": LossWeight("min_snr")}, True, BF)
    assert b[4]._rec is not None, "the step was never captured"
    assert a[0] == b[0] and torch.equal(a[1], b[1])
    ra, rb = a[4].level_loss(reset=False), b[4].level_loss(reset=False)
    assert ra == rb, "the running total must advance in a replayed graph as in the uncaptured step"


@pytest.mark.parametrize("use_graph", [False, True])
def test_level_loss_is_the_hosts_recomputation(use_graph):
    from inferbiomechanics_amd.loss_weight import LossWeight, band_edges, level_band
    C, steps = 14, 5
    losses, _, _, _, tr, bs = _run({"cond_cols": C, "loss_weight": LossWeight("min_snr")}, use_graph, torch.float32, steps=steps)
    rep = tr.level_loss(reset=True)
    ts = torch.cat([bs[i % 3][1] for i in range(steps)]).numpy()
    counts = np.bincount(level_band(ts, 1000), minlength=NB).tolist()
    assert rep["windows"] == counts and rep["steps"] == steps and sum(counts) == steps * B
    w_mean, u_mean = np.mean([l[0] for l in losses]), np.mean([l[1] for l in losses])
    assert abs(rep["weighted"] - w_mean) <= 1e-6 * w_mean and abs(rep["unweighted"] - u_mean) <= 1e-6 * u_mean
    assert [(lo, hi) for lo, hi, _ in rep["bands"]] == band_edges(1000) == [(125 * k, 125 * (k + 1)) for k in range(NB)]
    total = 0.0
    for (lo, hi, mean), cnt in zip(rep["bands"], counts):
        assert (mean is None) == (cnt == 0)
        if cnt:
            assert mean > 0
            total += mean * cnt * T * (D - C)
    expect = sum(l[1] for l in losses) * B * T * (D - C)                   # the unweighted sums of squared error
    assert abs(total - expect) <= 1e-5 * expect
    after = tr.level_loss(reset=True)
    assert after["windows"] == [0] * NB and after["steps"] == 0 and all(m is None for _, _, m in after["bands"])
    assert after["weighted"] is None and after["unweighted"] is None
    x0, t, eps = bs[0]
    tr.step((x0.to(DEV), t.to(DEV), eps.to(DEV)))                           # the total starts again behind a reset
    again = tr.level_loss(reset=False)
    assert again["steps"] == 1 and again["windows"] == np.bincount(level_band(t.numpy(), 1000), minlength=NB).tolist()
    assert abs(again["unweighted"] - float(tr.result[1].cpu())) <= 1e-6 * again["unweighted"]


def test_level_loss_needs_a_loss_weight():
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.engine import HipTrainer
    from inferbiomechanics_amd.loss_weight import LossWeight
    model, _ = make("transformer", torch.float32)
    tr = HipTrainer(model, "diffusion", "sgd", LR, use_graph=False)
    assert tr.loss_weight is None and tr.level_table is None and tr.level_accum is None
    with pytest.raises(hip.HipError):
        tr.level_loss()
    with pytest.raises(ValueError, match="1000"):
        HipTrainer(model, "diffusion", "sgd", LR, loss_weight=LossWeight("table", table=np.ones(999)))


@pytest.mark.parametrize("kind", ["transformer", "mlp"])
def test_step_drawn_agrees_with_step_on_the_drawn_batch(kind):
    from inferbiomechanics_amd.data.WindowCache import DeviceMotionCache
    from inferbiomechanics_amd.engine import HipTrainer
    from inferbiomechanics_amd.loss_weight import LossWeight
    C = 14
    g = torch.Generator().manual_seed(3)
    windows = torch.randn(32, T, D, generator=g)
    idx = torch.arange(B, device=DEV)
    ma, _ = make(kind, BF)
    mb, _ = make(kind, BF)
    mb.load_state_dict(ma.state_dict())
    cache = DeviceMotionCache(windows, DEV, BF)
    ta = HipTrainer(ma, "diffusion", "sgd", LR, use_graph=False, cond_cols=C, loss_weight=LossWeight("min_snr"))
    tb = HipTrainer(mb, "diffusion", "sgd", LR, use_graph=False, cond_cols=C, loss_weight=LossWeight("min_snr"))
    assert torch.equal(ta.flat, tb.flat)
    ta.step_drawn(cache, idx)
    la = ta.loss_value()
    x0, t, eps = (a.clone() for a in ta.drawn_batch())
    tb.step((x0, t, eps))
    assert la == tb.loss_value()
    assert torch.equal(ta.flat, tb.flat)
    assert ta.level_loss() == tb.level_loss()
