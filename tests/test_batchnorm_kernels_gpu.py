"""The BatchNorm1d kernels (ib_batchnorm_fwd / ib_batchnorm_bwd, csrc/batchnorm.hip) through hip.batchnorm_fwd / _bwd, every
output held ELEMENTWISE to the bound derived in tests/batchnorm_cases.py (float64 reference on the stored inputs; the table,
n, S and every term are defined there, and tests/test_batchnorm_bounds_cpu.py shows that the bound admits a correct
implementation and rejects nine one-line bugs).

Memory hygiene: every matrix is a [B, C] view of pitch ld inside a larger allocation with one guard row above and below.
Inputs carry NaN in the padding columns and guard rows (a read outside [B, C] that reaches a live column poisons a result);
outputs start as NaN inside (an element left unwritten fails) and a sentinel in the padding and guards, which must survive
bit for bit.  The backward is handed the float64 reference's mean and rstd rounded to fp32, so it is tested on its own.
The largest error / bound of each (case, dtype) is printed (pytest -rP) and asserted only to be <= 1."""
import pytest
import torch

from tests.batchnorm_cases import (ACTS, BY_NAME, CASES, DT, EPS, MOMENTUM, TRAIN_CASES, bound_bwd, bound_fwd, make_inputs,
                                   reference_bwd, reference_fwd, saved_stats, violations)

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 1536.0                          # exact in bf16 and fp32
NBT0 = 41
PARAMS = [(c, dt) for c in CASES for dt in ("fp32", "bf16")]
TRAIN_PARAMS = [(c, dt) for c in TRAIN_CASES for dt in ("fp32", "bf16")]
_id = lambda p: f"{p[0].name}-{p[1]}"
FWD_KEYS = ("y", "save_mean", "save_rstd", "running_mean", "running_var")


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from inferbiomechanics_amd import hip as h
    h.lib()
    return h


class _Mat:
    """a [B, C] view of pitch ld with a guard row on each side; `fill`: a [B, C] tensor (an input: NaN around it) or None (an
    output: NaN inside, the sentinel around it)"""

    def __init__(self, c, dtype, fill=None):
        self.guard = float("nan") if fill is not None else SENT
        self.buf = torch.full((c.B + 2, c.ld), self.guard, dtype=dtype, device=DEV)
        self.view = self.buf[1:c.B + 1, :c.C]
        if fill is not None:
            self.view.copy_(fill.to(dtype))
        else:
            self.view.fill_(float("nan"))
        assert self.view.stride(1) == 1 and self.view.stride(0) == c.ld

    def padding_intact(self):
        b = self.buf.clone()
        b[1:-1, :self.view.shape[1]] = SENT
        return torch.equal(b, torch.full_like(b, SENT))


def _vec(t):
    return t.clone().to(DEV)


def _forward(hip, c, dt, inp, training):
    x, y = _Mat(c, DT[dt], inp.x), _Mat(c, DT[dt])
    o = {"running_mean": _vec(inp.running_mean), "running_var": _vec(inp.running_var),
         "save_mean": torch.full((c.C,), float("nan"), device=DEV), "save_rstd": torch.full((c.C,), float("nan"), device=DEV),
         "nbt": torch.tensor(NBT0, dtype=torch.int64, device=DEV)}
    hip.batchnorm_fwd(x.view, _vec(inp.gamma), _vec(inp.beta), o["running_mean"], o["running_var"], o["nbt"], y.view,
                      o["save_mean"], o["save_rstd"], training, MOMENTUM, EPS)
    torch.cuda.synchronize()
    assert y.padding_intact(), f"{c.name}: the forward wrote outside y[:, :C]"
    o["y"] = y.view
    return o


def _held(tag, got, ref, bnd, keys):
    msgs, worst = [], 0.0
    for k in keys:
        msg, r = violations(f"{tag} {k}", got[k], ref[k], bnd[k])
        worst = max(worst, r)
        if msg:
            msgs.append(msg)
    assert not msgs, "\n".join(msgs)
    return worst


@pytest.mark.parametrize("p", TRAIN_PARAMS, ids=_id)
def test_training_forward(hip, p):
    c, dt = p
    inp = make_inputs(c, dt)
    got = _forward(hip, c, dt, inp, True)
    worst = _held(f"{c.name} {dt} training", got, reference_fwd(inp, True), bound_fwd(inp, dt, True), FWD_KEYS)
    print(f"kernel error / bound  {c.name:15s} {dt}  training forward {worst:.3f}")
    assert int(got["nbt"]) == NBT0 + 1
    again = _forward(hip, c, dt, inp, True)
    for k in FWD_KEYS + ("nbt",):
        assert torch.equal(got[k], again[k]), f"{k} is not bitwise repeatable"


@pytest.mark.parametrize("p", PARAMS, ids=_id)
def test_eval_forward(hip, p):
    c, dt = p
    inp = make_inputs(c, dt)
    got = _forward(hip, c, dt, inp, False)
    worst = _held(f"{c.name} {dt} eval", got, reference_fwd(inp, False), bound_fwd(inp, dt, False), FWD_KEYS)
    print(f"kernel error / bound  {c.name:15s} {dt}  eval forward {worst:.3f}")
    assert torch.equal(got["running_mean"].cpu(), inp.running_mean) and torch.equal(got["running_var"].cpu(), inp.running_var)
    assert int(got["nbt"]) == NBT0
    assert torch.equal(got["save_mean"].cpu(), inp.running_mean)
    again = _forward(hip, c, dt, inp, False)
    assert torch.equal(got["y"], again["y"]) and torch.equal(got["save_rstd"], again["save_rstd"])


def _backward(hip, c, dt, inp, training, act, sm, sr, accumulate=False, want_dx=True, want_dparams=True):
    dy, x = _Mat(c, DT[dt], inp.dy), _Mat(c, DT[dt], inp.x)
    aux = _Mat(c, DT[dt], inp.aux[act]) if act != "none" else None
    dx = _Mat(c, DT[dt]) if want_dx else None
    nan = lambda: torch.full((c.C,), float("nan"), device=DEV)
    dg = (_vec(inp.dgamma_old) if accumulate else nan()) if want_dparams else None
    db = (_vec(inp.dbeta_old) if accumulate else nan()) if want_dparams else None
    hip.batchnorm_bwd(dy.view, x.view, _vec(inp.gamma), sm.to(DEV), sr.to(DEV), dx.view if dx else None, dg, db, training,
                      accumulate=accumulate, act_below=act, aux=aux.view if aux else None)
    torch.cuda.synchronize()
    if dx:
        assert dx.padding_intact(), f"{c.name}: the backward wrote outside dx[:, :C]"
    return {"dx": dx.view if dx else None, "dgamma": dg, "dbeta": db}


@pytest.mark.parametrize("p", PARAMS, ids=_id)
def test_backward(hip, p):
    c, dt = p
    inp = make_inputs(c, dt)
    worst = 0.0
    for training in ((True, False) if c.B > 1 else (False,)):
        sm, sr = saved_stats(inp, training)
        for act in ACTS:
            tag = f"{c.name} {dt} backward training={training} act={act}"
            got = _backward(hip, c, dt, inp, training, act, sm, sr)
            worst = max(worst, _held(tag, got, reference_bwd(inp, training, act, sm, sr),
                                     bound_bwd(inp, dt, training, act, sm, sr), ("dx", "dgamma", "dbeta")))
            again = _backward(hip, c, dt, inp, training, act, sm, sr)
            assert all(torch.equal(got[k], again[k]) for k in got), f"{tag}: not bitwise repeatable"
            # accumulate: the column sums have a fixed order, so the result is fp32(old + the plain call's value), exactly
            acc = _backward(hip, c, dt, inp, training, act, sm, sr, accumulate=True)
            assert torch.equal(acc["dgamma"], inp.dgamma_old.to(DEV) + got["dgamma"]), f"{tag}: accumulate dgamma"
            assert torch.equal(acc["dbeta"], inp.dbeta_old.to(DEV) + got["dbeta"]), f"{tag}: accumulate dbeta"
            assert torch.equal(acc["dx"], got["dx"]), f"{tag}: accumulate changed dx"
            worst = max(worst, _held(tag + " accumulate", acc, reference_bwd(inp, training, act, sm, sr, True),
                                     bound_bwd(inp, dt, training, act, sm, sr, True), ("dgamma", "dbeta")))
            nodx = _backward(hip, c, dt, inp, training, act, sm, sr, want_dx=False)
            assert torch.equal(nodx["dgamma"], got["dgamma"]) and torch.equal(nodx["dbeta"], got["dbeta"]), f"{tag}: dx=None"
            nodp = _backward(hip, c, dt, inp, training, act, sm, sr, want_dparams=False)
            assert torch.equal(nodp["dx"], got["dx"]), f"{tag}: dgamma=None, dbeta=None"
    print(f"kernel error / bound  {c.name:15s} {dt}  backward {worst:.3f}")


def test_backward_on_the_kernels_own_statistics(hip):
    """as training runs it: the backward is handed what the kernel's forward saved"""
    for dt in ("fp32", "bf16"):
        c = BY_NAME["mid"]
        inp = make_inputs(c, dt)
        f = _forward(hip, c, dt, inp, True)
        sm, sr = f["save_mean"].cpu(), f["save_rstd"].cpu()
        got = _backward(hip, c, dt, inp, True, "silu", sm, sr)
        _held(f"mid {dt}", got, reference_bwd(inp, True, "silu", sm, sr), bound_bwd(inp, dt, True, "silu", sm, sr),
              ("dx", "dgamma", "dbeta"))


def test_refusals(hip):
    c = BY_NAME["eval_one_row"]
    inp = make_inputs(c, "fp32")
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        _forward(hip, c, "fp32", inp, True)
    # the C entry point refuses it too, and touches nothing
    x, y = _Mat(c, torch.float32, inp.x), _Mat(c, torch.float32)
    v = [_vec(t) for t in (inp.gamma, inp.beta, inp.running_mean, inp.running_var, inp.running_mean, inp.running_var)]
    nbt = torch.tensor(NBT0, dtype=torch.int64, device=DEV)
    rc = hip.lib().ib_batchnorm_fwd(x.view.data_ptr(), c.ld, *(t.data_ptr() for t in v[:4]), nbt.data_ptr(), y.view.data_ptr(),
                                    c.ld, v[4].data_ptr(), v[5].data_ptr(), c.B, c.C, MOMENTUM, EPS, 1, hip.dtype_code(torch.float32),
                                    hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and int(nbt) == NBT0 and torch.isnan(y.view).all() and torch.equal(v[2].cpu(), inp.running_mean)

    c = BY_NAME["ragged_waves"]
    inp = make_inputs(c, "fp32")
    f32 = lambda n=c.C: torch.zeros(n, device=DEV)
    x, y = _Mat(c, torch.float32, inp.x), _Mat(c, torch.float32)
    good = dict(x=x.view, gamma=f32(), beta=f32(), running_mean=f32(), running_var=f32() + 1, num_batches_tracked=None, y=y.view,
                save_mean=f32(), save_rstd=f32(), training=True)
    hip.batchnorm_fwd(**good)                                                      # the arguments below differ in one thing each
    for bad in (dict(y=y.buf[1:c.B, :c.C]), dict(y=y.buf[1:c.B + 1, :c.C - 1]), dict(gamma=f32().double()),
                dict(gamma=f32().to(torch.bfloat16)), dict(gamma=f32(c.C + 1)), dict(y=y.view.to(torch.bfloat16))):
        with pytest.raises(hip.HipError):
            hip.batchnorm_fwd(**{**good, **bad})
    dx = _Mat(c, torch.float32)
    bgood = dict(dy=x.view, x=x.view, gamma=f32(), save_mean=f32(), save_rstd=f32(), dx=dx.view, dgamma=f32(), dbeta=f32(),
                 training=True)
    hip.batchnorm_bwd(**bgood)
    for bad in (dict(act_below="silu"), dict(act_below="relu", aux=None), dict(act_below="tanh", aux=x.buf[1:c.B, :c.C]),
                dict(gamma=f32().double()), dict(dx=dx.buf[1:c.B, :c.C]), dict(x=x.buf[1:c.B + 1, :c.C - 1])):
        with pytest.raises(hip.HipError):
            hip.batchnorm_bwd(**{**bgood, **bad})
    torch.cuda.synchronize()
