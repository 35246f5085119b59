"""HipTrainer(velocity_loss=VelocityLoss(...)): the diffusion step with the velocity term in its loss seam.

A tiny fp32 transformer denoiser and the fp32 MLP denoiser, kinds eps and v, cond_cols 0 and 14, with and without Min-SNR.  One
step's reported loss and level report are held against velocity_loss.velocity_terms64 evaluated in float64 on the trainer's own
buffers -- the output the forward left in its pred buffer and the batch it staged -- within LOSS_RT = 1e-5 of
tests/test_loss_weight_kernels_gpu.py (the sums are fp32 sums of fp32 terms; the float64 target of kind v differs from the
kernel's fp32 one by 2^-24 per element, far inside that).  A captured graph replayed three times advances the float64 report by
three steps' worth, the parameters after one step differ from the step without the term, two fresh trainers give the same bits,
a checkpoint goes round and a different weight or gamma is refused, and without the term the state dict has no new key.
-m gpu."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.fixture_inputs import det_state  # noqa: E402

DEV = "cuda"
LR = 1e-2
B, T, D = 8, 12, 44
NB = 8
LOSS_RT = 1e-5


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def batch(seed=0):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, 1000, (B,), generator=g)
    t[:3] = torch.randint(0, 60, (3,), generator=g)
    t[3], t[4] = 0, 999
    return tuple(a.to(DEV) for a in (torch.randn(B, T, D, generator=g), t, torch.randn(B, T, D, generator=g)))


def make(kind):
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionMLP, DiffusionTransformer
    torch.manual_seed(0)
    if kind == "transformer":
        return DiffusionTransformer(D, T, d_model=128, num_heads=4, dim_feedforward=256, num_layers=2, device=DEV,
                                    compute_dtype=torch.float32)
    m = DiffusionMLP(D, [128, 128], temb_dim=32, temb_hidden=128, device=DEV, compute_dtype=torch.float32)
    sd = m.state_dict()
    m.load_state_dict({k: v.to(sd[k].dtype) for k, v in det_state({k: tuple(v.shape) for k, v in sd.items()}).items()})
    return m


def trainer(model_kind, pred="eps", C=0, min_snr=False, vl="on", use_graph=False, opt="sgd"):
    from inferbiomechanics_amd.engine import HipTrainer
    from inferbiomechanics_amd.loss_weight import LossWeight
    from inferbiomechanics_amd.velocity_loss import VelocityLoss
    if vl == "on":
        vl = VelocityLoss(0.5, gamma=5.0)
    return HipTrainer(make(model_kind), "diffusion", opt, LR, use_graph=use_graph, cond_cols=C, prediction=pred,
                      loss_weight=LossWeight("min_snr", gamma=5.0) if min_snr else None, velocity_loss=vl)


def pred_buffer(tr):
    """the trainer's own pred buffer as the step's forward left it, [B * T, D]"""
    M = B * T
    Dp = tr.plan.train_pitch(D, M) if hasattr(tr.plan, "train_pitch") else (D + 7) // 8 * 8
    return tr.plan.buf.get("tr.pred", (M, Dp), torch.float32)[:, :D]


def rel(a, e):
    return abs(a - e) / max(abs(e), 1e-30)


@pytest.mark.parametrize("min_snr", [False, True], ids=["plain", "min_snr"])
@pytest.mark.parametrize("C", [0, 14])
@pytest.mark.parametrize("pred", ["eps", "v"])
@pytest.mark.parametrize("model_kind", ["mlp", "transformer"])
def test_one_step_matches_the_restatement(model_kind, pred, C, min_snr):
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion.schedule import alphas_cumprod
    from inferbiomechanics_amd.velocity_loss import velocity_terms64
    tr = trainer(model_kind, pred, C, min_snr)
    x0, t, eps = batch(7)
    with hip.record_launches() as rec:
        tr.step((x0, t, eps))
    names = [n for n, _ in rec.calls]
    assert names.count("ib_vel_loss_partial") == 1 == names.count("ib_vel_loss_finalize")
    assert not {"ib_mse_loss_partial", "ib_mse_loss_finalize", "ib_mse_loss_partial_cond", "ib_mse_loss_finalize_cond",
                "ib_mse_loss_weighted_partial", "ib_mse_loss_weighted_finalize", "ib_mse_loss_pred_partial",
                "ib_mlp_chain_train"} & set(names), names
    staged = {k[0] if isinstance(k, tuple) else k: v for k, v in tr._static.items()}
    for name, mine in (("x0", x0), ("eps", eps), ("t", t)):
        assert torch.equal(staged[name], mine), "the staged batch is the batch"
    e = velocity_terms64(pred_buffer(tr).double().reshape(B, T, D), staged["x0"], staged["eps"], staged["t"],
                         alphas_cumprod(1000), pred, tr.level_table, tr.units_table, tr.vel_table, tr.vel_units_table,
                         cond_cols=C)
    r = tr.result.cpu().double().tolist()
    figures = {"total": (r[hip.VEL_R_TOTAL], float(e["loss"])), "mse": (r[hip.VEL_R_MSE], float(e["mse"])),
               "eps": (r[hip.VEL_R_EPS], float(e["eps_mse"])), "vel": (r[hip.VEL_R_VEL], float(e["vel"])),
               "x0": (r[hip.VEL_R_X0], float(e["x0_vel"]))}
    print(model_kind, pred, C, min_snr, {k: (v, rel(*v)) for k, v in figures.items()})
    for k, (a, b) in figures.items():
        assert b > 0 and rel(a, b) <= LOSS_RT, (k, a, b)
    assert tr.loss_value() == r[hip.VEL_R_TOTAL], "the trainer reads the optimised total where it reads its loss"
    counts = e["counts"].cpu().tolist()
    rep = tr.level_loss(reset=False)
    assert rep["steps"] == 1 and rep["windows"] == counts and sum(counts) == B
    assert rep["weighted"] == r[hip.VEL_R_TOTAL] and rep["unweighted"] == r[hip.VEL_R_EPS], "float64 += (double)fp32, once"
    assert rep["mse"] == r[hip.VEL_R_MSE] and rep["velocity"] == r[hip.VEL_R_VEL] and rep["x0_velocity"] == r[hip.VEL_R_X0]
    for k, ((lo, hi, mean), (lo2, hi2, vmean)) in enumerate(zip(rep["bands"], rep["x0_velocity_bands"])):
        assert (lo, hi) == (lo2, hi2)
        if counts[k]:
            assert rel(mean, float(e["bands"][k]) / (counts[k] * T * (D - C))) <= LOSS_RT
            assert rel(vmean, float(e["x0_bands"][k]) / (counts[k] * (T - 1) * (D - C))) <= LOSS_RT
        else:
            assert mean is None and vmean is None


@pytest.mark.parametrize("pred", ["eps", "v"])
@pytest.mark.parametrize("model_kind", ["mlp", "transformer"])
def test_replayed_graph_advances_the_report(model_kind, pred):
    from inferbiomechanics_amd import hip
    tr = trainer(model_kind, pred, C=14, use_graph=True)
    b = batch(9)
    for _ in range(3):                               # two uncaptured steps, the capture with its first replay
        tr.step(b)
    assert tr._rec is not None, "the step was never captured"
    before = tr.level_loss(reset=False)
    base = tr.level_accum.cpu().clone()
    seen = []
    for _ in range(3):
        tr.step(b)
        seen.append(tr.result.cpu().double().clone())
    after = tr.level_loss(reset=False)
    assert after["steps"] == before["steps"] + 3 == 6 and sum(after["windows"]) == sum(before["windows"]) + 3 * B
    grown = tr.level_accum.cpu() - base
    want = sum(s[:hip.VEL_RESULT_LEN] for s in seen)
    assert torch.allclose(grown, want, rtol=1e-12, atol=0), "accum += (double)result once per replay"
    assert len({float(s[hip.VEL_R_TOTAL]) for s in seen}) == 3 and all(float(s[hip.VEL_R_VEL]) > 0 for s in seen), \
        "each replay is a training step of its own"
    assert tr.level_loss(reset=True)["steps"] == 6 and tr.level_loss()["steps"] == 0
    assert float(tr.level_accum.abs().sum().cpu()) == 0.0


@pytest.mark.parametrize("model_kind", ["mlp", "transformer"])
def test_the_term_changes_the_step_and_is_reproducible(model_kind):
    b = batch(11)
    after = {}
    for name, vl in (("on", "on"), ("again", "on"), ("off", None)):
        tr = trainer(model_kind, "v", vl=vl)
        tr.step(b)
        torch.cuda.synchronize()
        after[name] = ({k: v.detach().clone() for k, v in tr.model.state_dict().items()}, tr.result.clone())
    for k in after["on"][0]:
        assert torch.equal(after["on"][0][k], after["again"][0][k]), f"two fresh trainers must give the same bits: {k}"
    assert torch.equal(after["on"][1].view(torch.int32), after["again"][1].view(torch.int32))
    assert any(not torch.equal(after["on"][0][k], after["off"][0][k]) for k in after["on"][0]), \
        "the parameters after one step must differ from the step without the term"
    assert float(after["on"][1][0]) > float(after["off"][1][0]), "total = the MSE term + a positive velocity term"


def test_checkpoint_round_trip_and_refusals():
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.velocity_loss import VelocityLoss
    mk = lambda vl: trainer("mlp", "v", vl=vl, opt="adam")
    tr = mk(VelocityLoss(0.5, gamma=4.0))
    tr.step(batch(3))
    sd = tr.optimizer_state_dict()
    assert sd["velocity_loss"] == {"weight": 0.5, "gamma": 4.0, "table": None}
    again = mk(VelocityLoss(0.5, gamma=4.0))
    again.load_optimizer_state_dict(sd)
    assert again.steps_done == 1 and torch.equal(again.s1, tr.s1)
    for other in (VelocityLoss(0.25, gamma=4.0), VelocityLoss(0.5, gamma=5.0), None):
        t2 = mk(other)
        with pytest.raises(hip.HipError, match="checkpoint's velocity loss"):
            t2.load_optimizer_state_dict(sd)
        assert t2.steps_done == 0
    plain = mk(None)
    plain.step(batch(3))
    assert "velocity_loss" not in plain.optimizer_state_dict(), "without the term the state dict has no new key"
    assert plain.vel_table is None and plain.level_accum.numel() == 2 + 2 * NB, "a v trainer's report as it was"
