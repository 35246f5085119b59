"""HipTrainer(cond_cols = C > 0): the training step of a denoiser conditioned on the first C columns of every frame, against
a float64 autograd restatement (conditioning columns of x_t clean, the oracle's forward, the mean over the free columns
only) for one and three SGD steps of the transformer denoiser (fp32, bf16) and of the bf16 MLP denoiser (which must take the
per-op path: the chain kernel noises and scores every column).  cond_cols = 0 is the unconditional trainer bit for bit,
with and without graph capture; runs at C > 0 are bitwise reproducible; step_drawn agrees with step on the drawn batch.

Bounds.  fp32: the loss within 1e-3 and every parameter within 2e-3 max|e| + 2e-5, the bounds of
tests/test_trainer_gpu.py::test_fused_trainer_matches_oracle_trajectory_fp32.  bf16: the loss within 2 %, that file's bound
on a bf16 loss curve; it bounds no bf16 parameters, so the parameter MOVEMENT w' - w (lr times the summed gradients) is held
to 6e-2 in relative norm, the bound smoke() puts on the bf16 transformer step's gradient.  -m gpu."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as R  # noqa: E402
from oracle.fixture_inputs import det_state  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
LR = 1e-2


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def load_det(module):
    sd = module.state_dict()
    new = det_state({k: tuple(v.shape) for k, v in sd.items()})
    module.load_state_dict({k: v.to(sd[k].dtype) for k, v in new.items()})


def batches(n, B, T, D, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(B, T, D, generator=g).to(dtype), torch.randint(0, 1000, (B,), generator=g),
             torch.randn(B, T, D, generator=g).to(dtype)) for _ in range(n)]


def make(kind, dtype, D, T):
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


def reference_run(p0, fwd, bs, C, steps, dtype):
    """float64 SGD over the conditional loss.  bf16: the forward reads the matrices rounded to bf16 (the trainer's shadow of
    its fp32 master weights), the gradient goes to the master (straight through the rounding)"""
    p = {k: v.clone().requires_grad_(True) for k, v in p0.items()}
    tabs = R.schedule_tables()
    losses = []
    for i in range(steps):
        x0, t, eps = (a.double() if a.is_floating_point() else a for a in bs[i % len(bs)])
        for v in p.values():
            v.grad = None
        xt = R.q_sample(x0, t, eps, tabs)
        xt = torch.cat([x0[..., :C], xt[..., C:]], dim=-1)                  # conditioning columns clean
        if dtype == BF:
            xt = xt.to(BF).double()                                          # x_t is stored in the compute dtype
            pf = {k: (v + (v.detach().to(BF).double() - v.detach())) if v.dim() >= 2 else v for k, v in p.items()}
        else:
            pf = p
        pred = fwd(pf, xt, t)
        loss = ((pred[..., C:] - eps[..., C:]) ** 2).mean()                  # free columns only
        loss.backward()
        losses.append(float(loss))
        with torch.no_grad():
            for v in p.values():
                v -= LR * v.grad
    return losses, {k: v.detach() for k, v in p.items()}


@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("kind,dtype", [("transformer", torch.float32), ("transformer", BF), ("mlp", BF)])
def test_conditional_step_matches_float64(kind, dtype, steps):
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.engine import HipTrainer
    B, T, D, C = 8, 12, 44, 14
    model, fwd = make(kind, dtype, D, T)
    p0 = {k: v.detach().cpu().double().clone() for k, v in model.state_dict().items()}
    bs = batches(3, B, T, D, dtype, seed=7)
    ref_losses, ref_p = reference_run(p0, fwd, bs, C, steps, dtype)
    tr = HipTrainer(model, "diffusion", "sgd", LR, use_graph=False, cond_cols=C)
    if kind == "mlp":
        assert tr.plan.chain_ok(D) and not tr.plan.chain_ok(D, C), "the conditional MLP step must leave the chain kernel"
    got = []
    with hip.record_launches() as rec:
        for i in range(steps):
            x0, t, eps = bs[i % len(bs)]
            tr.step((x0.to(DEV), t.to(DEV), eps.to(DEV)))
            got.append(tr.loss_value())
    names = [n for n, _ in rec.calls]
    assert names.count("ib_q_sample_cond") == steps and names.count("ib_mse_loss_partial_cond") == steps
    assert names.count("ib_mse_loss_finalize_cond") == steps
    assert not {"ib_q_sample", "ib_mse_loss_partial", "ib_mse_loss_finalize", "ib_mlp_chain_train"} & set(names), names
    lt = 1e-3 if dtype == torch.float32 else 2e-2
    print(kind, dtype, "losses", got, "float64", ref_losses)
    for a, e in zip(got, ref_losses):
        assert abs(a - e) <= lt * abs(e), (got, ref_losses)
    worst = 0.0
    for k, v in model.state_dict().items():
        a, e, w0 = v.detach().cpu().double(), ref_p[k], p0[k]
        if dtype == torch.float32:
            err = (a - e).abs().max().item()
            assert err <= 2e-3 * max(e.abs().max().item(), 1e-6) + 2e-5, (k, err)
        else:
            mv = (e - w0).norm().item()
            if mv > 0:
                rel = ((a - w0) - (e - w0)).norm().item() / mv
                worst = max(worst, rel)
                assert rel <= 6e-2, (k, rel)
    print(kind, dtype, "worst relative movement error", worst)


def _run(cond_kw, use_graph, dtype, steps=6, kind="transformer", B=8, T=12, D=44):
    from inferbiomechanics_amd.engine import HipTrainer
    model, _ = make(kind, dtype, D, T)
    tr = HipTrainer(model, "diffusion", "adam", 1e-3, use_graph=use_graph, **cond_kw)
    bs = batches(3, B, T, D, dtype, seed=11)
    losses = []
    for i in range(steps):
        x0, t, eps = bs[i % 3]
        tr.step((x0.to(DEV), t.to(DEV), eps.to(DEV)))
        losses.append(tr.loss_value())
    torch.cuda.synchronize()
    return losses, tr.flat.detach().clone(), tr.s1.detach().clone(), tr.s2.detach().clone(), tr


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("kind,dtype", [("transformer", torch.float32), ("transformer", BF), ("mlp", BF)])
def test_cond_cols_zero_is_the_unconditional_trainer_bitwise(kind, dtype, use_graph):
    from inferbiomechanics_amd import hip
    a = _run({}, use_graph, dtype, kind=kind)
    if use_graph:
        b = _run({"cond_cols": 0}, use_graph, dtype, kind=kind)
    else:
        with hip.record_launches() as rec:
            b = _run({"cond_cols": 0}, use_graph, dtype, kind=kind)
        names = {n for n, _ in rec.calls}
        assert not {"ib_q_sample_cond", "ib_mse_loss_partial_cond", "ib_mse_loss_finalize_cond"} & names
    assert a[0] == b[0]
    for x, y in zip(a[1:4], b[1:4]):
        assert torch.equal(x, y)
    if use_graph:
        assert b[4]._rec is not None


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("kind,dtype", [("transformer", BF), ("mlp", BF), ("transformer", torch.float32)])
def test_conditional_runs_are_bitwise_reproducible(kind, dtype, use_graph):
    a = _run({"cond_cols": 14}, use_graph, dtype, kind=kind)
    b = _run({"cond_cols": 14}, use_graph, dtype, kind=kind)
    assert a[0] == b[0]
    for x, y in zip(a[1:4], b[1:4]):
        assert torch.equal(x, y)
    c = _run({}, use_graph, dtype, kind=kind)
    assert a[0] != c[0], "the conditional loss must differ from the unconditional one"


def test_graph_replay_equals_eager_at_cond_cols():
    a = _run({"cond_cols": 14}, False, BF)
    b = _run({"cond_cols": 14}, True, BF)
    assert b[4]._rec is not None, "the step was never captured"
    assert a[0] == b[0] and torch.equal(a[1], b[1])


def test_dpred_is_zero_on_the_conditioning_columns_every_step():
    from inferbiomechanics_amd.engine import HipTrainer
    B, T, D, C = 8, 12, 44, 14
    model, _ = make("transformer", BF, D, T)
    tr = HipTrainer(model, "diffusion", "sgd", LR, use_graph=False, cond_cols=C)
    bs = batches(2, B, T, D, BF, seed=5)
    for i in range(2):
        x0, t, eps = bs[i]
        tr.step((x0.to(DEV), t.to(DEV), eps.to(DEV)))
        torch.cuda.synchronize()
        Dp = tr.plan.train_pitch(D, B * T) if hasattr(tr.plan, "train_pitch") else (D + 7) // 8 * 8
        dpred = tr.plan.buf.get("tr.dpred", (B * T, Dp), BF)
        xt = tr.plan.buf.get("tr.xt", (B * T, Dp), BF)
        assert torch.equal(dpred[:, :C], torch.zeros_like(dpred[:, :C]))
        assert dpred[:, C:D].abs().max().item() > 0
        assert torch.equal(xt[:, :C], x0.to(DEV).view(B * T, D)[:, :C]), "conditioning columns must reach the network clean"
        if i == 0:
            dpred[:, :C] = 5.0          # garbage: the next step must clear it


def test_cond_cols_is_validated_on_the_first_batch():
    from inferbiomechanics_amd.engine import HipTrainer
    model, _ = make("transformer", torch.float32, 44, 12)
    with pytest.raises(ValueError):
        HipTrainer(model, "diffusion", "sgd", LR, cond_cols=-1)
    tr = HipTrainer(model, "diffusion", "sgd", LR, use_graph=False, cond_cols=44)
    x0, t, eps = batches(1, 4, 12, 44, torch.float32)[0]
    with pytest.raises(ValueError, match="cond_cols"):
        tr.step((x0.to(DEV), t.to(DEV), eps.to(DEV)))


@pytest.mark.parametrize("kind", ["transformer", "mlp"])
def test_step_drawn_agrees_with_step_on_the_drawn_batch(kind):
    """device-made batches at C > 0: the step over (x0 gathered, t / eps drawn on the device) is the step fed that batch"""
    from inferbiomechanics_amd.data.WindowCache import DeviceMotionCache
    from inferbiomechanics_amd.engine import HipTrainer
    B, T, D, C = 8, 12, 44, 14
    g = torch.Generator().manual_seed(3)
    windows = torch.randn(32, T, D, generator=g)
    idx = torch.arange(B, device=DEV)
    ma, _ = make(kind, BF, D, T)
    mb, _ = make(kind, BF, D, T)
    mb.load_state_dict(ma.state_dict())
    cache = DeviceMotionCache(windows, DEV, BF)
    ta = HipTrainer(ma, "diffusion", "sgd", LR, use_graph=False, cond_cols=C)
    tb = HipTrainer(mb, "diffusion", "sgd", LR, use_graph=False, cond_cols=C)
    assert torch.equal(ta.flat, tb.flat)
    ta.step_drawn(cache, idx)
    la = ta.loss_value()
    x0, t, eps = (a.clone() for a in ta.drawn_batch())
    tb.step((x0, t, eps))
    assert la == tb.loss_value()
    assert torch.equal(ta.flat, tb.flat)
