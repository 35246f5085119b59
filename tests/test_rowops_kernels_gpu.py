"""The row-wise kernels of csrc/rowops.hip on the GPU.

1. LayerNorm (ib_layernorm_fwd / _bwd / _bwd_reduce through hip.layernorm_*): every case of tests/rowops_cases.py in every
   dtype of the case, every output element (y, mean, rstd, dx, dres, dgamma, dbeta) held to the bound derived there (float64
   reference on the stored inputs; tests/test_rowops_bounds_cpu.py shows that the bound admits a correct kernel and rejects
   thirteen one-line bugs).  The backward is handed the reference's mean and rstd rounded to fp32, so it is tested on its
   own.  Memory hygiene: every tensor is a contiguous view inside a larger buffer, G elements of guard on each side (and one
   more in front where the case asks for a misaligned tensor); inputs carry NaN in the guards, outputs start as NaN inside
   and the sentinel SENT in the guards, which must survive bit for bit.  The backward's workspace is NaN-filled, and what
   lies beyond the 2 parts N floats the launcher asks for must still be NaN afterwards.
2. ib_segment_colsum, elementwise: ceil(cnt / RL) additions per lane and RL through LDS, each on a partial sum no larger
   than the sum of the absolute terms (rowops_cases.colsum_adds), times S.
3. ib_cast2d / ib_cast and 4. ib_concat_keys: bit for bit against torch on the CPU.
The largest error / bound of each case is printed (pytest -rP) and asserted only to be <= 1."""
import math

import pytest
import torch

from tests.rowops_cases import (BY_NAME, DT, EPS, PARAMS, S, U32, add_col0, bound_bwd, bound_fwd, case_id, colsum_adds, colsum_rl,
                                dispatch_of, inputs_to, ld_add_of, ln_bwd_parts, make_inputs, reference_bwd, reference_fwd,
                                saved_stats, violations)

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 1536.0                          # exact in bf16 and fp32
G = 8                                  # guard elements: 16 bytes of bf16, 32 of fp32, so an aligned view stays aligned
NAN = float("nan")
IB_E_ARG, IB_E_WORKSPACE, IB_E_UNSUPPORTED = -1, -4, -5
WS_TAIL = 64                           # floats handed over beyond what the launcher needs


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from inferbiomechanics_amd import hip as h
    h.lib()
    return h


class _Buf:
    """a contiguous view of `shape` inside a 1-D buffer with G guard elements on each side, one element further in when
    `mis`; fill: a tensor (an input: NaN around it) or None (an output: NaN inside, the sentinel around it)"""

    def __init__(self, shape, dtype, fill=None, mis=False):
        n = math.prod(shape)
        self.buf = torch.full((n + 2 * G + 1,), NAN if fill is not None else SENT, dtype=dtype, device=DEV)
        self.lo = G + (1 if mis else 0)
        self.view = self.buf[self.lo:self.lo + n].view(shape)
        if fill is not None:
            self.view.copy_(fill.to(dtype))
        else:
            self.view.fill_(NAN)
        assert self.view.is_contiguous() and (self.view.data_ptr() % 16 == 0) == (not mis)

    def intact(self):
        b = self.buf.clone()
        b[self.lo:self.lo + self.view.numel()] = SENT
        return bool((b == SENT).all())


def _add_div(c, inp, dtype):
    """add_div as a column slice of a wider NaN-filled matrix of pitch ld_add_of(c)"""
    if c.add is None:
        return None
    wide = torch.full((inp.add.shape[0], ld_add_of(c)), NAN, dtype=dtype, device=DEV)
    view = wide[:, add_col0(c):add_col0(c) + c.N]
    view.copy_(inp.add)
    assert view.stride(0) == ld_add_of(c) and view.data_ptr() % 16 == 0
    return view


def _cpu(d):
    return {k: v.cpu() for k, v in d.items()}


def _held(tag, got, ref, bnd, keys):
    msgs, worst = [], 0.0
    for k in keys:
        msg, r = violations(f"{tag} {k}", got[k], ref[k], bnd[k])
        worst = max(worst, r)
        if msg:
            msgs.append(msg)
    assert not msgs, "\n".join(msgs)
    return worst


def _forward(hip, c, dt, inp):
    t, f32 = DT[dt], torch.float32
    x = _Buf((c.M, c.N), t, inp.x, "x" in c.mis)
    res = _Buf((c.M, c.N), t, inp.res, "res" in c.mis) if c.res else None
    y = _Buf((c.M, c.N), t, None, "y" in c.mis)
    gamma, beta = _Buf((c.N,), f32, inp.gamma, "gamma" in c.mis), _Buf((c.N,), f32, inp.beta, "beta" in c.mis)
    mean, rstd = _Buf((c.M,), f32), _Buf((c.M,), f32)
    hip.layernorm_fwd(x.view, gamma.view, beta.view, y.view, mean.view, rstd.view, res=res.view if res else None, act=c.act,
                      eps=EPS, add_div=_add_div(c, inp, t), seg=c.seg)
    torch.cuda.synchronize()
    for name, b in (("y", y), ("mean", mean), ("rstd", rstd)):
        assert b.intact(), f"{c.name}: the forward wrote outside {name}"
    return {"y": y.view, "mean": mean.view, "rstd": rstd.view}


def _backward(hip, c, dt, inp, mean, rstd, mode="plain"):
    """mode: plain (dgamma, dbeta start as NaN), accumulate (they start as dgamma_old, dbeta_old) or deferred (None, then
    ib_layernorm_bwd_reduce)"""
    t, f32 = DT[dt], torch.float32
    M, N = c.M, c.N
    x, dy = _Buf((M, N), t, inp.x, "x" in c.mis), _Buf((M, N), t, inp.dy, "dy" in c.mis)
    res = _Buf((M, N), t, inp.res, "res" in c.mis) if c.res else None
    dx = _Buf((M, N), t, None, "dx" in c.mis)
    dres = _Buf((M, N), t, None, "dres" in c.mis) if c.dres else None
    gamma = _Buf((N,), f32, inp.gamma, "gamma" in c.mis)
    dg = _Buf((N,), f32, inp.dgamma_old if mode == "accumulate" else None)
    db = _Buf((N,), f32, inp.dbeta_old if mode == "accumulate" else None)
    if mode == "accumulate":                                         # inputs AND outputs: the sentinel around them
        for b in (dg, db):
            keep = b.view.clone()
            b.buf.fill_(SENT)
            b.view.copy_(keep)
    need = 2 * ln_bwd_parts(M) * N
    assert hip.layernorm_bwd_workspace_bytes(M, N) == 4 * need
    ws = torch.full((need + WS_TAIL,), NAN, dtype=f32, device=DEV)
    assert ws.data_ptr() % 16 == 0
    now = mode != "deferred"
    hip.layernorm_bwd(dy.view, x.view, gamma.view, mean.to(DEV), rstd.to(DEV), dx.view, dg.view if now else None,
                      db.view if now else None, ws, res=res.view if res else None, dres=dres.view if dres else None, act=c.act,
                      accumulate=mode == "accumulate", add_div=_add_div(c, inp, t), seg=c.seg)
    if not now:
        hip.layernorm_bwd_reduce(ws, dg.view, db.view, M, N)
    torch.cuda.synchronize()
    for name, b in (("dx", dx), ("dres", dres), ("dgamma", dg), ("dbeta", db)):
        assert b is None or b.intact(), f"{c.name}: the backward wrote outside {name}"
    assert torch.isnan(ws[need:]).all(), f"{c.name}: the backward wrote past the 2 parts N floats of its workspace"
    assert torch.isfinite(ws[:need]).all(), f"{c.name}: a partial row was left unwritten"
    return {"dx": dx.view, "dres": dres.view if dres else None, "dgamma": dg.view, "dbeta": db.view}


def _on_device(c, dt):
    """(inputs on the CPU, the same on the GPU: the float64 reference and bound of the big cases are computed there)"""
    inp = make_inputs(c, dt)
    return inp, inputs_to(inp, DEV)


# ---- 1. LayerNorm ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", PARAMS, ids=case_id)
def test_layernorm_forward(hip, p):
    c, dt = p
    inp, dinp = _on_device(c, dt)
    got = _forward(hip, c, dt, dinp)
    ref, bnd = _cpu(reference_fwd(c, dinp, dt)), _cpu(bound_fwd(c, dinp, dt))
    worst = _held(f"{c.name} {dt} forward", got, ref, bnd, ("y", "mean", "rstd"))
    print(f"kernel error / bound  {c.name:34s} {dt}  forward {worst:.3f}  {dispatch_of(c, 'fwd', dt)}")
    zero_g = inp.gamma == 0
    y = got["y"].float().cpu()
    assert torch.equal(y[:, zero_g], inp.beta[zero_g].expand(c.M, -1)), "gamma = 0: y must be beta exactly"
    if c.values in ("const", "gamma0"):
        assert torch.equal(y, inp.beta.expand(c.M, -1)), f"{c.values}: y must be beta exactly"


@pytest.mark.parametrize("p", PARAMS, ids=case_id)
def test_layernorm_backward(hip, p):
    c, dt = p
    inp, dinp = _on_device(c, dt)
    mean, rstd = saved_stats(c, dinp, dt)
    keys = ("dx", "dgamma", "dbeta") + (("dres",) if c.dres else ())
    got = _backward(hip, c, dt, dinp, mean, rstd)
    ref, bnd = _cpu(reference_bwd(c, dinp, dt, mean, rstd)), _cpu(bound_bwd(c, dinp, dt, mean, rstd))
    worst = _held(f"{c.name} {dt} backward", got, ref, bnd, keys)
    # accumulate into non-zero dgamma / dbeta: held to its own bound, and exactly fp32(old + the plain call's value)
    acc = _backward(hip, c, dt, dinp, mean, rstd, "accumulate")
    worst = max(worst, _held(f"{c.name} {dt} backward accumulate", acc, _cpu(reference_bwd(c, dinp, dt, mean, rstd, True)),
                             _cpu(bound_bwd(c, dinp, dt, mean, rstd, True)), ("dgamma", "dbeta")))
    assert torch.equal(acc["dgamma"], dinp.dgamma_old + got["dgamma"]) and torch.equal(acc["dbeta"], dinp.dbeta_old + got["dbeta"])
    # the deferred form is the immediate one, bit for bit
    late = _backward(hip, c, dt, dinp, mean, rstd, "deferred")
    for k in keys:
        assert torch.equal(late[k], got[k]), f"{c.name} {dt}: deferred {k} differs from the immediate one"
        assert torch.equal(acc[k], got[k]) or k in ("dgamma", "dbeta"), f"{c.name} {dt}: accumulate changed {k}"
    print(f"kernel error / bound  {c.name:34s} {dt}  backward {worst:.3f}  {dispatch_of(c, 'bwd', dt)}")
    if c.values == "gamma0":
        assert (got["dx"] == 0).all() and (got["dres"] == 0).all(), "gamma = 0: dx and dres must be exactly 0"
    if c.values == "dy0":
        assert all((got[k] == 0).all() for k in keys), "dy = 0: every gradient must be exactly 0"


def test_layernorm_backward_on_the_kernels_own_statistics(hip):
    """as training runs it: the backward is handed what the kernel's forward saved"""
    for name, dt in (("flags_264_silu_res_dres", "fp32"), ("flags_520_elu_res_dres", "bf16"), ("fast_4097_res", "bf16")):
        c = BY_NAME[name]
        _, dinp = _on_device(c, dt)
        f = _forward(hip, c, dt, dinp)
        mean, rstd = f["mean"].clone(), f["rstd"].clone()
        got = _backward(hip, c, dt, dinp, mean, rstd)
        _held(f"{name} {dt}", got, _cpu(reference_bwd(c, dinp, dt, mean, rstd)), _cpu(bound_bwd(c, dinp, dt, mean, rstd)),
              ("dx", "dgamma", "dbeta") + (("dres",) if c.dres else ()))


@pytest.mark.parametrize("name", ["fast_4097_res", "fast_4099"])
def test_fast_agrees_with_generic(hip, name):
    """the same rows through the fast kernels (M >= 4096) and, in two halves of fewer than 4096 rows, through the generic
    ones: y, mean, rstd and dx agree to within the sum of the two bounds"""
    c, dt = BY_NAME[name], "bf16"
    _, dinp = _on_device(c, dt)
    assert dispatch_of(c, "fwd", dt)[0] == dispatch_of(c, "bwd", dt)[0] == "fast512"
    mean, rstd = saved_stats(c, dinp, dt)
    fast = {**_forward(hip, c, dt, dinp), **_backward(hip, c, dt, dinp, mean, rstd)}
    bf = {**_cpu(bound_fwd(c, dinp, dt)), **_cpu(bound_bwd(c, dinp, dt, mean, rstd))}
    for lo, hi in ((0, 2048), (2048, c.M)):
        h = c._replace(name=f"{name}[{lo}:{hi}]", M=hi - lo)
        assert dispatch_of(h, "fwd", dt)[0] == dispatch_of(h, "bwd", dt)[0] == "generic"
        hinp = dinp._replace(x=dinp.x[lo:hi], dy=dinp.dy[lo:hi], res=None if dinp.res is None else dinp.res[lo:hi])
        gen = {**_forward(hip, h, dt, hinp), **_backward(hip, h, dt, hinp, mean[lo:hi], rstd[lo:hi])}
        bg = {**_cpu(bound_fwd(h, hinp, dt)), **_cpu(bound_bwd(h, hinp, dt, mean[lo:hi], rstd[lo:hi]))}
        for k in ("y", "mean", "rstd", "dx"):
            a, b = fast[k][lo:hi].double().cpu(), gen[k].double().cpu()
            bad = (a - b).abs() > bf[k][lo:hi] + bg[k]
            assert torch.isfinite(a).all() and torch.isfinite(b).all() and not bad.any(), \
                f"{name} rows {lo}:{hi} {k}: {int(bad.sum())} elements differ by more than the two bounds"


def _raw_bwd(hip, c, dt, t, **over):
    """the C entry point itself (hip.layernorm_bwd refuses most bad arguments before it); -> (rc, the outputs)"""
    f32 = torch.float32
    M, N = c.M, c.N
    inp = inputs_to(make_inputs(c, dt), DEV)
    x, dy, gamma = _Buf((M, N), t, inp.x), _Buf((M, N), t, inp.dy), _Buf((N,), f32, inp.gamma)
    mean, rstd = saved_stats(c, inp, dt)
    outs = {"dx": _Buf((M, N), t), "dgamma": _Buf((N,), f32), "dbeta": _Buf((N,), f32)}
    need = 2 * ln_bwd_parts(M) * N
    ws = torch.full((need,), NAN, dtype=f32, device=DEV)
    add = torch.zeros(-(-M // 5), N, dtype=t, device=DEV)
    a = dict(dgamma=outs["dgamma"].view.data_ptr(), dbeta=outs["dbeta"].view.data_ptr(), ws_bytes=4 * need, add=None, ld_add=0,
             seg=0, N=N)
    a.update(over)
    if a["add"]:
        a["add"] = add.data_ptr()
    rc = hip.lib().ib_layernorm_bwd(dy.view.data_ptr(), x.view.data_ptr(), None, 0, gamma.view.data_ptr(), mean.data_ptr(),
                                    rstd.data_ptr(), outs["dx"].view.data_ptr(), None, a["dgamma"], a["dbeta"], 0, ws.data_ptr(),
                                    a["ws_bytes"], a["add"], a["ld_add"], a["seg"], M, a["N"], hip.dtype_code(t), hip.stream_ptr())
    torch.cuda.synchronize()
    untouched = all(torch.isnan(b.view).all() and b.intact() for b in outs.values()) and bool(torch.isnan(ws).all())
    return rc, untouched


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_layernorm_refusals(hip, dt):
    t, f32 = DT[dt], torch.float32
    c = BY_NAME["flags_40_none"]
    assert _raw_bwd(hip, c, dt, t)[0] == 0                            # the arguments below differ from these in one thing each
    for what, over, code in (("dgamma without dbeta", dict(dbeta=None), IB_E_ARG), ("dbeta without dgamma", dict(dgamma=None), IB_E_ARG),
                             ("ld_add < N", dict(add=True, ld_add=c.N - 1, seg=5), IB_E_ARG),
                             ("seg = 0 with add_div", dict(add=True, ld_add=c.N, seg=0), IB_E_ARG),
                             ("seg < 0 with add_div", dict(add=True, ld_add=c.N, seg=-5), IB_E_ARG),
                             # include/ib_hip.h gives a short workspace its own code, IB_E_WORKSPACE: refused all the same
                             ("short workspace", dict(ws_bytes=4 * 2 * ln_bwd_parts(c.M) * c.N - 1), IB_E_WORKSPACE)):
        rc, untouched = _raw_bwd(hip, c, dt, t, **over)
        assert rc == code and untouched, f"{what}: code {rc}, outputs untouched: {untouched}"
    # the forward's two
    M, N = c.M, c.N
    x, y, mean, rstd = _Buf((M, N), t, torch.ones(M, N)), _Buf((M, N), t), _Buf((M,), f32), _Buf((M,), f32)
    gb = torch.ones(N, device=DEV)
    add = torch.zeros(3, N, dtype=t, device=DEV)
    for ld_add, seg in ((N - 1, 5), (N, 0)):
        rc = hip.lib().ib_layernorm_fwd(x.view.data_ptr(), None, 0, gb.data_ptr(), gb.data_ptr(), y.view.data_ptr(),
                                        mean.view.data_ptr(), rstd.view.data_ptr(), add.data_ptr(), ld_add, seg, M, N, EPS,
                                        hip.dtype_code(t), hip.stream_ptr())
        torch.cuda.synchronize()
        assert rc == IB_E_ARG and all(torch.isnan(b.view).all() and b.intact() for b in (y, mean, rstd))
    # N = 2049: IB_E_UNSUPPORTED from both directions, nothing written
    M, N = 5, 2049
    x, y, dx = _Buf((M, N), t, torch.ones(M, N)), _Buf((M, N), t), _Buf((M, N), t)
    mean, rstd, dg, db = _Buf((M,), f32), _Buf((M,), f32), _Buf((N,), f32), _Buf((N,), f32)
    gb = torch.ones(N, device=DEV)
    ws = torch.full((2 * N + WS_TAIL,), NAN, device=DEV)
    with pytest.raises(hip.HipError, match=rf"code {IB_E_UNSUPPORTED}\)"):
        hip.layernorm_fwd(x.view, gb, gb, y.view, mean.view, rstd.view)
    with pytest.raises(hip.HipError, match=rf"code {IB_E_UNSUPPORTED}\)"):
        hip.layernorm_bwd(x.view, x.view, gb, torch.zeros(M, device=DEV), torch.ones(M, device=DEV), dx.view, dg.view, db.view, ws)
    torch.cuda.synchronize()
    assert all(torch.isnan(b.view).all() and b.intact() for b in (y, dx, mean, rstd, dg, db)) and torch.isnan(ws).all()


# ---- 2. ib_segment_colsum ----------------------------------------------------------------------------------------------
COLSUM_RPS = (1, 31, 32, 33, 63, 64, 65, 4 * 16 + 1)
COLSUM_N = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257)


def _segments(M, seg, mode):
    if mode == 0:
        return [list(range(s * seg, min((s + 1) * seg, M))) for s in range(-(-M // seg))]
    return [list(range(s, M, seg)) for s in range(min(seg, M))]


def _colsum_once(hip, dt, mode, rps, N, layout, accumulate, gen):
    t = DT[dt]
    if mode == 0:
        seg = rps
        M = 2 * seg + (seg + 1) // 2                                 # a ragged last segment (seg > 1)
    else:
        seg, M = 3, 3 * rps - 1                                      # segment 2 is one row short
    segs = _segments(M, seg, mode)
    assert max(len(s) for s in segs) == rps and (rps == 1 or min(len(s) for s in segs) < rps)
    x64 = torch.randn(M, N, generator=gen, dtype=torch.float64).to(t)
    ldx = {"plain": N, "pitched": N + 4 - N % 4 if N % 4 else N + 4, "odd_ldx": N + (1 if N % 2 == 0 else 2), "misaligned": N + 4}[layout]
    buf = torch.full((M * ldx + 16,), NAN, dtype=t, device=DEV)
    lo = 8 + (1 if layout == "misaligned" else 0)
    xv = buf[lo:lo + M * ldx].view(M, ldx)[:, :N]
    xv.copy_(x64)
    ldo = N + 3
    out = torch.full((len(segs) + 2, ldo), SENT, device=DEV)
    ov = out[1:-1, :N]
    old = torch.randn(len(segs), N, generator=gen)
    ov.copy_(old if accumulate else torch.full_like(old, NAN))
    lp = torch.full((len(segs) + 2, N + 5), SENT, dtype=torch.bfloat16, device=DEV)
    hip.segment_colsum(xv, ov, seg, mode=mode, accumulate=accumulate, out_bf16=lp[1:-1, :N])
    torch.cuda.synchronize()
    X = x64.double()
    ref = torch.stack([X[s].sum(0) for s in segs])
    mag = torch.stack([X[s].abs().sum(0) for s in segs])
    n = torch.tensor([colsum_adds(len(s), rps) for s in segs], dtype=torch.float64)[:, None]
    bnd = n * U32 * mag
    if accumulate:
        ref = old.double() + ref
        bnd = bnd + U32 * ref.abs()
    tag = f"colsum {dt} mode {mode} rps {rps} N {N} {layout} acc {accumulate}"
    msg, worst = violations(tag, ov, ref, S * bnd)
    assert msg is None, msg
    o2 = out.clone()
    o2[1:-1, :N] = SENT
    assert (o2 == SENT).all(), f"{tag}: wrote outside out[:, :N]"
    assert torch.equal(lp[1:-1, :N], ov.to(torch.bfloat16)), f"{tag}: out_bf16 is not the RNE of out"
    l2 = lp.clone()
    l2[1:-1, :N] = SENT
    assert (l2 == SENT).all(), f"{tag}: wrote outside out_bf16[:, :N]"
    return worst


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_segment_colsum(hip, dt, mode):
    assert [colsum_rl(r) for r in (32, 33)] == [4, 16]
    gen = torch.Generator().manual_seed(11 + mode)
    worst = 0.0
    for rps in COLSUM_RPS:
        for N in COLSUM_N:
            worst = max(worst, _colsum_once(hip, dt, mode, rps, N, "plain", False, gen))
            if N in (4, 64, 257) or rps in (33, 65):
                for layout in ("pitched", "odd_ldx", "misaligned"):
                    worst = max(worst, _colsum_once(hip, dt, mode, rps, N, layout, layout == "odd_ldx", gen))
            if N in (5, 256):
                worst = max(worst, _colsum_once(hip, dt, mode, rps, N, "plain", True, gen))
    print(f"kernel error / bound  segment_colsum {dt} mode {mode}  {worst:.3f}")


def test_segment_colsum_segment_limit(hip):
    """the segment index is the grid's y: 65535 segments are taken (N = 1), 65536 refused with nothing written"""
    x = torch.randn(65536, 1, device=DEV)
    out = torch.full((65536, 1), NAN, device=DEV)
    hip.segment_colsum(x[:65535], out[:65535], 1)
    torch.cuda.synchronize()
    assert torch.equal(out[:65535], x[:65535]) and torch.isnan(out[65535]).all()
    out.fill_(NAN)
    with pytest.raises(hip.HipError, match=rf"code {IB_E_UNSUPPORTED}\)"):
        hip.segment_colsum(x, out, 1)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ---- 3. ib_cast2d / ib_cast --------------------------------------------------------------------------------------------
def _special_f32():
    bits = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001,
            0x00000001, 0x80000001, 0x007FFFFF, 0x00012345,            # fp32 subnormals
            0x00010000, 0x80010000, 0x00008000, 0x00008001, 0x00007FFF,  # the smallest bf16 subnormal, half of it (a tie), +-1 ulp
            0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,              # exact ties: down to even, up to even
            0x3F808001, 0x3F807FFF,                                      # one ulp either side of a tie
            0x7F7F7FFF, 0x7F7F8000, 0xFF7F7FFF, 0xFF7F8000,              # the last below bf16 overflow, the first at it
            0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F0000, 0x00800000]              # FLT_MAX, the largest bf16, the smallest normal
    return torch.tensor([b - (1 << 32) if b >= 1 << 31 else b for b in bits], dtype=torch.int32).view(torch.float32)


def _same_bits(got, want, tag):
    got, want = got.cpu(), want.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), f"{tag}: NaN must stay NaN, and only NaN"
    iv = torch.int32 if got.dtype == torch.float32 else torch.int16
    g, w = got.contiguous().view(iv), want.contiguous().view(iv)
    bad = (g != w) & ~nan
    assert not bad.any(), f"{tag}: {int(bad.sum())} elements differ in their bits, first at {tuple(bad.nonzero()[0].tolist())}"


@pytest.mark.parametrize("dst_dt", ["fp32", "bf16"])
@pytest.mark.parametrize("src_dt", ["fp32", "bf16"])
def test_cast2d_bit_exact(hip, src_dt, dst_dt):
    ts, td = DT[src_dt], DT[dst_dt]
    gen = torch.Generator().manual_seed(5)
    sp = _special_f32()
    for rows, cols in ((1, 1), (3, 5), (64, 64), (65, 63)):
        vals = torch.randn(rows * cols, generator=gen) * torch.exp(8 * torch.randn(rows * cols, generator=gen))
        k = min(len(sp), rows * cols)
        vals[:k] = sp[:k]
        if (rows, cols) == (1, 1):
            vals[0] = sp[15]                                         # a tie
        src_cpu = vals.to(ts).view(rows, cols)                       # (fp32 -> bf16 on the CPU first for a bf16 source)
        want = src_cpu.to(td)
        for lds, ldd in ((cols, cols), (cols + 3, cols + 5)):
            src = torch.full((rows, lds), SENT, dtype=ts, device=DEV)
            src[:, :cols] = src_cpu
            dst = torch.full((rows + 2, ldd), SENT, dtype=td, device=DEV)
            hip.cast2d(src[:, :cols], dst[1:-1, :cols])
            torch.cuda.synchronize()
            _same_bits(dst[1:-1, :cols], want, f"cast2d {src_dt}->{dst_dt} {rows}x{cols} pitch {lds}/{ldd}")
            d2 = dst.clone()
            d2[1:-1, :cols] = SENT
            assert (d2 == SENT).all(), "cast2d wrote into the padding"
        flat = torch.full((rows * cols + 2 * G,), SENT, dtype=td, device=DEV)
        hip.cast(src_cpu.reshape(-1).to(DEV), flat[G:-G])
        torch.cuda.synchronize()
        _same_bits(flat[G:-G], want.reshape(-1), f"cast {src_dt}->{dst_dt} n = {rows * cols}")
        assert (flat[:G] == SENT).all() and (flat[-G:] == SENT).all()


# ---- 4. ib_concat_keys -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_concat_keys_bit_exact(hip, dt):
    t = DT[dt]
    gen = torch.Generator().manual_seed(3)
    for rows in (1, 5):
        for widths in ((5,), (1,), (1, 7), (7, 1), tuple(1 + k % 4 for k in range(16))):
            keys = [torch.randn(rows, w, generator=gen) for w in widths]
            total = sum(widths)
            out = _Buf((rows, total), t)
            hip.concat_keys([k.to(DEV) for k in keys], out.view)
            torch.cuda.synchronize()
            assert out.intact()
            _same_bits(out.view, torch.cat(keys, 1).to(t), f"concat {dt} rows {rows} widths {widths}")
            off = 0
            for k, w in zip(keys, widths):                           # the boundary columns between keys, explicitly
                assert torch.equal(out.view[:, off].cpu(), k[:, 0].to(t)) and torch.equal(out.view[:, off + w - 1].cpu(), k[:, -1].to(t))
                off += w
    keys = [torch.randn(2, 1, device=DEV) for _ in range(17)]
    out = _Buf((2, 17), t)
    with pytest.raises(hip.HipError, match=rf"code {IB_E_ARG}\)"):
        hip.concat_keys(keys, out.view)
    torch.cuda.synchronize()
    assert torch.isnan(out.view).all() and out.intact()
