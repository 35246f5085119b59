"""The two kernels of the conditional training step on the GPU: ib_q_sample_cond (conditioning columns copied clean, free
columns ib_q_sample's bit for bit, pad columns untouched) and ib_mse_loss_partial_cond + ib_mse_loss_finalize_cond (free-column
mean, dpred exactly 0 on the conditioning columns on every launch, cond_cols = 0 bit for bit the unconditional pair, fixed
summation order).  D = 300 / 64 take the 4-wide kernels (D = 300, C = 270 splits a vector; C = 1, 2, D - 1 too), D = 7 the
element-wise ones; ld = D + pad exercises the row pitch (pad 4: still 4-wide; pad 1: element-wise).  -m gpu."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
# the tolerances tests/test_hip_kernels.py::test_mse_loss applies: the loss 1e-5, dpred TIGHT[dtype]
LOSS_RT = 1e-5
TIGHT = {torch.float32: 2e-5, BF: 3e-2}


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from inferbiomechanics_amd import hip as h
    h.lib()
    return h


def cases():
    out = []
    for D in (300, 64, 7):
        cs = [0, 1, 2, D - 1] + ([270] if D == 300 else [])
        for C in cs:
            for pad in (0, 4, 1):
                out.append((D, C, pad))
    return out


def rnd(shape, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64).to(dtype)


def close(actual, expected, rtol, what):
    a, e = actual.detach().to("cpu", torch.float64), expected.detach().to("cpu", torch.float64)
    assert a.shape == e.shape, (what, a.shape, e.shape)
    assert torch.isfinite(a).all(), f"{what}: non-finite values"
    err, ref = (a - e).abs().max().item(), max(e.abs().max().item(), 1e-30)
    assert err <= rtol * ref, f"{what}: max err {err:.3e} > {rtol:.1e} * {ref:.3e}"


@pytest.mark.parametrize("dtype", [torch.float32, BF])
@pytest.mark.parametrize("D,C,pad", cases())
def test_q_sample_cond(hip, dtype, D, C, pad):
    from inferbiomechanics_amd.diffusion.schedule import DiffusionTables
    B, T = 5, 9
    tabs = DiffusionTables(DEV)
    x0, eps = rnd((B, T, D), 1, dtype).to(DEV), rnd((B, T, D), 2, dtype).to(DEV)
    t = torch.tensor([0, 17, 500, 998, 999], device=DEV)
    ld = D + pad
    SENT = 7.0
    full_ref = torch.full((B * T, ld), SENT, dtype=dtype, device=DEV)
    full = torch.full((B * T, ld), SENT, dtype=dtype, device=DEV)
    hip.q_sample(x0, eps, t, tabs.sqrt_ab, tabs.sqrt_1mab, full_ref[:, :D])
    hip.q_sample_cond(x0, eps, t, tabs.sqrt_ab, tabs.sqrt_1mab, full[:, :D], C)
    torch.cuda.synchronize()
    got, ref, x2 = full[:, :D], full_ref[:, :D], x0.view(B * T, D)
    assert torch.equal(got[:, :C], x2[:, :C]), "conditioning columns must be x0's"
    assert torch.equal(got[:, C:], ref[:, C:]), "free columns must be ib_q_sample's bit for bit"
    assert torch.equal(full[:, D:], torch.full((B * T, pad), SENT, dtype=dtype, device=DEV)), "pad columns were touched"
    # the bit patterns too (torch.equal takes -0 == +0): the conditioning columns are a copy
    as_int = lambda v: v.contiguous().view(torch.int16 if dtype == BF else torch.int32)
    assert torch.equal(as_int(got[:, :C]), as_int(x2[:, :C]))
    if pad == 0:                                            # the contiguous [B, T, D] form of x_t
        xt3 = torch.empty_like(x0)
        hip.q_sample_cond(x0, eps, t, tabs.sqrt_ab, tabs.sqrt_1mab, xt3, C)
        assert torch.equal(xt3.view(B * T, D), got)


def cond_loss(hip, pred, target, C, dpred):
    rows, D = pred.shape
    ws = torch.empty(hip.mse_loss_workspace_bytes(rows * D), dtype=torch.uint8, device=DEV)
    res = torch.zeros(1, dtype=torch.float32, device=DEV)
    hip.mse_loss_partial_cond(pred, target, ws, C, dpred=dpred)
    hip.mse_loss_finalize_cond(ws, res, rows * D, rows * (D - C))
    return res


@pytest.mark.parametrize("dtype", [torch.float32, BF])
@pytest.mark.parametrize("D,C,pad", cases())
def test_mse_loss_cond(hip, dtype, D, C, pad):
    rows = 1236 if D != 300 else 450            # several blocks of partial sums; 1236 * 7 is a multiple of 4
    ld = D + pad
    pbuf = torch.zeros((rows, ld), dtype=dtype, device=DEV)
    pbuf[:, :D] = rnd((rows, D), 3, dtype).to(DEV)
    pred, target = pbuf[:, :D], rnd((rows, D), 4, dtype).to(DEV)
    GARBAGE = float("nan")
    dbuf = torch.full((rows, ld), GARBAGE, dtype=dtype, device=DEV)
    res = cond_loss(hip, pred, target, C, dbuf[:, :D])
    torch.cuda.synchronize()
    dp = dbuf[:, :D]
    assert torch.isnan(dbuf[:, D:]).all(), "pad columns of dpred were touched"
    # exactly 0 on the conditioning columns although the buffer held garbage
    assert torch.equal(dp[:, :C], torch.zeros((rows, C), dtype=dtype, device=DEV))
    d = pred.double().cpu()[:, C:] - target.double().cpu()[:, C:]
    n = rows * (D - C)
    print(f"D={D} C={C} pad={pad} {dtype}: loss {float(res):.8f} vs float64 {float((d * d).mean()):.8f}")
    close(res, (d * d).mean().reshape(1), LOSS_RT, "cond mse")
    close(dp[:, C:], 2 * d / n, TIGHT[dtype], "cond dmse")
    # a second launch on the same inputs, over another garbage fill: the same bits
    dbuf2 = torch.full((rows, ld), -3.0, dtype=dtype, device=DEV)
    res2 = cond_loss(hip, pred, target, C, dbuf2[:, :D])
    assert torch.equal(res, res2) and torch.equal(dbuf2[:, :D], dp)
    # no dpred: the same loss
    assert torch.equal(cond_loss(hip, pred, target, C, None), res)
    if C == 0:
        ws = torch.empty(hip.mse_loss_workspace_bytes(rows * D), dtype=torch.uint8, device=DEV)
        res0 = torch.zeros(1, dtype=torch.float32, device=DEV)
        d0 = torch.full((rows, ld), GARBAGE, dtype=dtype, device=DEV)
        hip.mse_loss_partial(pred, target, ws, dpred=d0[:, :D])
        hip.mse_loss_finalize(ws, res0, rows * D)
        assert torch.equal(res0, res), "cond_cols = 0 must be the unconditional loss bit for bit"
        assert torch.equal(d0[:, :D], dp), "cond_cols = 0 must be the unconditional dpred bit for bit"
