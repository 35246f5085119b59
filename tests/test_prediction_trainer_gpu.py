"""HipTrainer(prediction='x0' | 'v'): the diffusion step whose network predicts the clean window or v.

Tiny fp32 MLP and transformer denoisers, cond_cols 0 and 14, with and without Min-SNR (gamma = 5, in the form of the kind), the
step uncaptured and from the replayed graph, are held against a float64 autograd restatement of mean(w_t (out - target)^2)
built as tests/test_loss_weight_trainer_gpu.py builds its reference, within that file's bounds: the loss within 1e-3 and every
parameter within 2e-3 max|e| + 2e-5.  result[1], the error in noise units, is held to the same restatement's mean(u_t q^2).

Training and sampling agree on the convention: on the trainer's own buffers, result[1] equals the eps-MSE obtained by
converting the output with hip.pred_to_eps at x_t and scoring it against eps with the existing ib_mse_loss entries, within a
difference derived below from the per-element roundings of the two paths.  level_loss() works without a loss_weight, and a
resumed trainer must give the same kind.  -m gpu."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as R  # noqa: E402
from oracle.fixture_inputs import det_state  # noqa: E402

DEV = "cuda"
LR = 1e-2
B, T, D = 8, 12, 44
NB = 8
STEPS = 4                                        # two uncaptured steps, the capture, one more replay


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def load_det(module):
    sd = module.state_dict()
    new = det_state({k: tuple(v.shape) for k, v in sd.items()})
    module.load_state_dict({k: v.to(sd[k].dtype) for k, v in new.items()})


def batches(n, seed=0):
    """t mixes low noise levels (SNR above gamma = 5) with levels drawn over the whole range, 0 and 999 among them"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        t = torch.randint(0, 1000, (B,), generator=g)
        t[:3] = torch.randint(0, 60, (3,), generator=g)
        t[3], t[4] = 0, 999
        out.append((torch.randn(B, T, D, generator=g), t, torch.randn(B, T, D, generator=g)))
    return out


def make(kind):
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionMLP, DiffusionTransformer
    if kind == "transformer":
        torch.manual_seed(0)
        m = DiffusionTransformer(D, T, d_model=128, num_heads=4, dim_feedforward=256, num_layers=2, device=DEV,
                                 compute_dtype=torch.float32)
        fwd = lambda p, x, t: R.denoiser_transformer_forward(p, x, t, 2, 4)
    else:
        m = DiffusionMLP(D, [128, 128], temb_dim=32, temb_hidden=128, device=DEV, compute_dtype=torch.float32)
        load_det(m)
        fwd = lambda p, x, t: R.denoiser_mlp_forward(p, x, t, [128, 128], temb_dim=32)
    return m, fwd


def schedule64(n=1000):
    """alpha_bar in float64, written here: linear betas 1e-4 .. 0.02"""
    return torch.cumprod(1.0 - torch.linspace(1e-4, 0.02, n, dtype=torch.float64), dim=0)


def tables64(pred, min_snr, gamma=5.0):
    """(w, u): the weight of the kind's own squared error and its factor into noise units, closed forms in float64"""
    ab = schedule64()
    snr = ab / (1.0 - ab)
    u = snr if pred == "x0" else ab
    if not min_snr:
        return torch.ones_like(ab), u
    m = torch.minimum(snr, torch.full_like(snr, gamma))
    return (m if pred == "x0" else m / (snr + 1.0)), u


_REF = {}


def reference_run(model_kind, pred, C, min_snr, p0, fwd, bs):
    """float64 SGD over mean(w_t (out - target)^2) on the free columns, STEPS steps: per step (loss, mean(u_t q^2), the
    parameters after it).  Made once per case and shared by the uncaptured and the captured test."""
    key = (model_kind, pred, C, min_snr)
    if key in _REF:
        return _REF[key]
    w64, u64 = tables64(pred, min_snr)
    ab = schedule64()
    p = {k: v.clone().requires_grad_(True) for k, v in p0.items()}
    tabs = R.schedule_tables()
    out = []
    for i in range(STEPS):
        x0, t, eps = (a.double() if a.is_floating_point() else a for a in bs[i % len(bs)])
        for v in p.values():
            v.grad = None
        xt = R.q_sample(x0, t, eps, tabs)
        xt = torch.cat([x0[..., :C], xt[..., C:]], dim=-1)
        a, s = torch.sqrt(ab[t])[:, None, None], torch.sqrt(1.0 - ab[t])[:, None, None]
        target = x0 if pred == "x0" else a * eps - s * x0
        sq = (fwd(p, xt, t)[..., C:] - target[..., C:]) ** 2
        loss = (w64[t][:, None, None] * sq).mean()
        loss.backward()
        with torch.no_grad():
            for v in p.values():
                v -= LR * v.grad
        out.append((float(loss.detach()), float((u64[t][:, None, None] * sq).detach().mean()),
                    {k: v.detach().clone() for k, v in p.items()}))
    _REF[key] = out
    return out


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "captured"])
@pytest.mark.parametrize("min_snr", [False, True], ids=["plain", "min_snr"])
@pytest.mark.parametrize("C", [0, 14])
@pytest.mark.parametrize("pred", ["x0", "v"])
@pytest.mark.parametrize("model_kind", ["mlp", "transformer"])
def test_step_matches_float64(model_kind, pred, C, min_snr, use_graph):
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.engine import HipTrainer
    from inferbiomechanics_amd.loss_weight import LossWeight
    model, fwd = make(model_kind)
    p0 = {k: v.detach().cpu().double().clone() for k, v in model.state_dict().items()}
    bs = batches(3, seed=7)
    ref = reference_run(model_kind, pred, C, min_snr, p0, fwd, bs)
    tr = HipTrainer(model, "diffusion", "sgd", LR, use_graph=use_graph, cond_cols=C, prediction=pred,
                    loss_weight=LossWeight("min_snr", gamma=5.0) if min_snr else None)
    steps = STEPS if use_graph else 1
    got = []
    with hip.record_launches() as rec:
        for i in range(steps):
            x0, t, eps = bs[i % len(bs)]
            tr.step((x0.to(DEV), t.to(DEV), eps.to(DEV)))
            got.append((tr.loss_value(), float(tr.result[1].cpu())))
    names = [n for n, _ in rec.calls]
    assert "ib_mse_loss_pred_partial" in names and "ib_mse_loss_weighted_finalize" in names
    assert not {"ib_mse_loss_partial", "ib_mse_loss_finalize", "ib_mse_loss_partial_cond", "ib_mse_loss_finalize_cond",
                "ib_mse_loss_weighted_partial", "ib_mlp_chain_train"} & set(names), names
    if use_graph:
        assert tr._rec is not None, "the step was never captured"
    print(model_kind, pred, C, min_snr, use_graph, "got", got, "float64", [(l, u) for l, u, _ in ref[:steps]])
    for (a, ua), (e, ue, _) in zip(got, ref):
        assert abs(a - e) <= 1e-3 * abs(e), (got, ref[0][:2])
        assert abs(ua - ue) <= 1e-3 * abs(ue), "result[1] is the eps-MSE the output implies"
    ref_p = ref[steps - 1][2]
    for k, v in model.state_dict().items():
        a, e = v.detach().cpu().double(), ref_p[k]
        err = (a - e).abs().max().item()
        assert err <= 2e-3 * max(e.abs().max().item(), 1e-6) + 2e-5, (k, err)
    rep = tr.level_loss(reset=False)                 # kept without a loss_weight too
    assert rep["steps"] == steps and sum(rep["windows"]) == steps * B
    assert abs(rep["unweighted"] - np.mean([u for _, u in got])) <= 1e-6 * rep["unweighted"]


@pytest.mark.parametrize("C", [0, 14])
@pytest.mark.parametrize("pred", ["x0", "v"])
def test_training_and_sampling_agree_on_the_convention(pred, C):
    """result[1] against ib_pred_to_eps + ib_mse_loss on the trainer's own x_t and output, fp32.

    With the fp32 tables a, s, is, u read as reals, o the output, x the stored x_t = a x0 + s eps + dx, q = o - target exact,
    and v = 2^-24 one rounding, the two paths square A = sqrt(u) q_A and B = e - eps, which differ per element by at most
      v:   B = a q - g eps + s dx + d1,  g = a^2 + s^2 - 1, |g| <= 2 v (two table roundings), |d1| <= v (|s x| + |e|);
           q_A = q + dq, |dq| <= v (|s x0| + |target| + |q_A|);  sqrt(u) = a (1 + h), |h| <= 1.5 v
           -> |A - B| <= a |dq| + 1.5 v a |q| + 2 v |eps| + s |dx| + |d1| + v |B|
      x0:  B = -(a / s) q + dx / s + d2,  |d2| <= 3 v |r| is + v |e|  (r = x - a o: its rounding, the entry is = (1 / s)(1 + 2 v), and
           the final rounding);  q_A = q + dq, |dq| <= v |q_A|;  sqrt(u) = (a / s)(1 + h), |h| <= 2.5 v
           -> |A - B| <= (a / s) |dq| + 2.5 v (a / s) |q| + |dx| / s + |d2| + v |B|
      |dx| <= v (|s eps| + |x|)  (ib_q_sample: one rounded product, one fused multiply-add).
    The means then differ by at most sum |A - B| (|A| + |B|) / n, plus the roundings inside each fp32 sum of squares: two per
    term and fewer than 62 additions on any path from a term to the result (8 in a thread, 7 in a wave, 3 in a workgroup, a
    strided sum and an 8-level tree in the finalize), so 64 v of each sum."""
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.engine import HipTrainer
    model, _ = make("mlp")
    tr = HipTrainer(model, "diffusion", "sgd", LR, use_graph=False, cond_cols=C, prediction=pred)
    x0, t, eps = (a.to(DEV) for a in batches(1, seed=21)[0])
    tr.step((x0, t, eps))
    reported = float(tr.result[1].cpu())
    tabs = model.tables(torch.device(DEV))
    M = B * T
    buf = tr.plan.buf
    Dp = (D + 7) // 8 * 8
    xt_full, pred_full = buf.get("tr.xt", (M, Dp), torch.float32), buf.get("tr.pred", (M, Dp), torch.float32)
    o = pred_full.clone()
    conv = o.clone().view(B, T, Dp)
    hip.pred_to_eps(xt_full.view(B, T, Dp), conv, t, tabs.sqrt_ab, tabs.sqrt_1mab, tabs.inv_sqrt_1mab, pred, D=D)
    e2 = conv.view(M, Dp)[:, :D]
    ws = torch.zeros(hip.mse_loss_workspace_bytes(M * D), dtype=torch.uint8, device=DEV)
    res = torch.zeros(1, dtype=torch.float32, device=DEV)
    if C:
        hip.mse_loss_partial_cond(e2, eps.view(M, D), ws, C)
        hip.mse_loss_finalize_cond(ws, res, M * D, M * (D - C))
    else:
        hip.mse_loss_partial(e2, eps.view(M, D), ws)
        hip.mse_loss_finalize(ws, res, M * D)
    converted = float(res.cpu())
    # ---- the allowed difference, in float64 from the same buffers
    v = 2.0 ** -24
    row = lambda tab: tab.double()[t].repeat_interleave(T)[:, None]
    a, s, inv, u = row(tabs.sqrt_ab), row(tabs.sqrt_1mab), row(tabs.inv_sqrt_1mab), row(tr.units_table)
    sl = slice(C, D)
    o64, x64 = o[:, sl].double(), xt_full[:, sl].double()
    x064, eps64 = x0.view(M, D)[:, sl].double(), eps.view(M, D)[:, sl].double()
    dx = v * ((s * eps64).abs() + x64.abs())
    Bv = (e2[:, sl].double() - eps64).abs()
    if pred == "v":
        target = a * eps64 - s * x064
        q = (o64 - target).abs()
        dq = v * ((s * x064).abs() + target.abs() + q)
        d1 = v * ((s * x64).abs() + e2[:, sl].double().abs())
        diff = a * dq + 1.5 * v * a * q + 2 * v * eps64.abs() + s * dx + d1 + v * Bv
    else:
        q = (o64 - x064).abs()
        r = (x64 - a * o64).abs()
        d2 = 3 * v * r * inv + v * e2[:, sl].double().abs()
        diff = (a * inv) * v * q + 2.5 * v * (a * inv) * q + dx * inv + d2 + v * Bv
    Av = torch.sqrt(u) * q
    n = M * (D - C)
    allowed = float((diff * (Av + Bv + diff)).sum() / n) + 64 * v * (reported + converted)
    print("convention", pred, C, "reported", reported, "converted", converted, "difference", abs(reported - converted),
          "allowed", allowed)
    assert reported > 0 and abs(reported - converted) <= allowed
    assert allowed <= 1e-4 * reported, "the bound itself must stay a rounding-level statement"


def test_a_resumed_trainer_must_give_the_same_kind():
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.engine import HipTrainer
    mk = lambda kind: HipTrainer(make("mlp")[0], "diffusion", "adam", 1e-3, use_graph=False, prediction=kind)
    tr = mk("v")
    x0, t, eps = (a.to(DEV) for a in batches(1, seed=3)[0])
    tr.step((x0, t, eps))
    sd = tr.optimizer_state_dict()
    assert sd["prediction"] == "v"
    again = mk("v")
    again.load_optimizer_state_dict(sd)
    assert again.steps_done == 1 and torch.equal(again.s1, tr.s1)
    for other in ("eps", "x0"):
        t2 = mk(other)
        with pytest.raises(hip.HipError, match="checkpoint's prediction"):
            t2.load_optimizer_state_dict(sd)
        assert t2.steps_done == 0
    assert "prediction" not in mk("eps").optimizer_state_dict()
