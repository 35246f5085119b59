"""The frozen-weight layer kernels on the GPU: csrc/linln_panel.hip (ib_linear_ln_panel_fwd, ib_linear_panel_fwd,
ib_ffn_infer_fwd), the INFER form of csrc/ffn_chain.hip (ib_ffn_chain_fwd_infer) and ib_linear_ln_fwd of csrc/gemm.hip.

Every case of tests/frozen_cases.py: integer inputs, so that every GEMM and every bf16 value kept before a LayerNorm is exact;
GEMM outputs and the fp32 slabs left in the workspaces are compared bit for bit, LayerNorm outputs elementwise against the
bound derived there (tests/test_frozen_bounds_cpu.py shows that the bound admits a correct kernel and rejects the issue's
thirteen one-line bugs).  Each case asserts the path the launcher took (ib_debug_last_path) and the workgroup and workspace
numbers of the C query functions against the restated geometry that names the case's kernel instantiation.
Memory hygiene: every tensor is a view inside a larger buffer, G guard elements on each side, pitched where the entry point
takes a pitch; inputs carry NaN in the guards and in the pitch padding, outputs start as NaN with the sentinel SENT around them
(guards and padding), which must survive bit for bit; workspaces are NaN-filled and must still be NaN beyond what the launch
is to write.  Refusals hand over valid buffers and rely on the return code: nothing written, no path recorded.
The chain's training form (ib_ffn_chain_fwd with the attention epilogue and tail) runs on the same inputs where the table says
so: its saved s1, x1, f1, s2 are the exact values; its y, qkv, mean, rstd, mean1, rstd1 are held to the same staged bounds
as the INFER form's.  The two forms' y are NOT required to agree bit for bit: the compiler contracts the one-pass variance
E[v^2] - mean^2 of ff_ln_rows_fwd as fma(-mean, mean, E2) for one row of a pair and as fma(sq, 1 / N, -fl(mean^2)) for the
other, and which row gets which differs between the instantiations (both contractions are inside the bound's u mean^2 + u var
terms).  The count of elements whose bits differ is printed.
The largest error / bound of each case is printed (pytest -rP) and asserted only to be <= 1."""
import ctypes

import pytest
import torch

from tests.frozen_cases import (BF, BY_NAME, CASES, D, EPS, F32, IB_BF16, IB_E_UNSUPPORTED, IB_F32, IB_OK, PATH_NONE, REFUSED,
                                case_id, check, expected_path, ffn_coop_geometry, ffn_geometry, ffn_infer_workspace,
                                linear_ln_plan, linear_panel_workgroups, linln_panel_workgroups, ln_adds,
                                ln_reference, make_inputs, reference, violations, weights)

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 1536.0                          # exact in bf16 and fp32
G = 8                                  # guard elements: 16 bytes of bf16, 32 of fp32, so an aligned view stays aligned
NAN = float("nan")
WS_TAIL = 64                           # floats handed over beyond what the launcher asks for


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from inferbiomechanics_amd import hip as h
    h.lib()
    return h


class _Buf:
    """rows [M, N] of pitch ld (default N) -- or a vector [N] -- as a view inside a 1-D buffer with G guard elements on each
    side; fill: a tensor (an input: NaN in guards and padding) or None (an output: NaN inside, the sentinel around it)"""

    def __init__(self, shape, dtype, fill=None, ld=0):
        rows, n = (shape[0], shape[1]) if len(shape) == 2 else (1, shape[0])
        ld = ld or n
        assert ld >= n
        self.buf = torch.full((rows * ld + 2 * G,), NAN if fill is not None else SENT, dtype=dtype, device=DEV)
        body = self.buf[G:G + rows * ld].view(rows, ld)
        self.view = body[:, :n] if len(shape) == 2 else body[0, :n]
        if fill is not None:
            self.view.copy_(fill.to(dtype))
        else:
            self.view.fill_(NAN)
        self.mask = torch.zeros_like(self.buf, dtype=torch.bool)
        self.mask[G:G + rows * ld].view(rows, ld)[:, :n] = True
        assert self.view.data_ptr() % 16 == 0

    def intact(self):
        return bool((self.buf[~self.mask] == SENT).all())

    def untouched(self):
        return self.intact() and bool(torch.isnan(self.view).all())


def _ws(need_floats):
    ws = torch.full((need_floats + WS_TAIL,), NAN, dtype=F32, device=DEV)
    assert ws.data_ptr() % 16 == 0
    return ws


_PACKED = {}


def _packed(hip, c):
    """the packed images of a case's weights (packed once per weight set): linln_panel / linear_panel weights go through the
    W1 slot of ib_ffn_chain_pack, whose chunk k is the image of rows 512 k ... of the matrix"""
    key = (c.fam, c.N, c.K, c.ffn)
    if key not in _PACKED:
        W = weights(*key)
        if c.fam in ("linln_panel", "linear_panel"):
            w1 = W["w"].to(BF).to(DEV)
            layer = (w1, torch.zeros(D, c.N, dtype=BF, device=DEV))
            ffn = c.N
        else:
            layer = (W["w1"].to(BF).to(DEV), W["w2"].to(BF).to(DEV))
            ffn = c.ffn
        packed = torch.zeros(hip.ffn_chain_packed_elems(D, ffn), dtype=BF, device=DEV)
        if c.fam == "chain":
            layer = layer + (packed, W["wo"].to(BF).to(DEV), W["wqkv"].to(BF).to(DEV))
        else:
            layer = layer + (packed,)
        hip.ffn_chain_pack([layer])
        torch.cuda.synchronize()
        _PACKED[key] = packed
    return _PACKED[key]


def _vec(t):
    return _Buf((t.numel(),), F32, t)


def _path(hip):
    return hip.lib().ib_debug_last_path()


# ---- the launches: -> the outputs as frozen_cases.check takes them --------------------------------------------------------
def _run_linln_panel(hip, c):
    inp, W = make_inputs(c), weights(c.fam, c.N, c.K, c.ffn)
    M = c.M
    rows = ctypes.c_int32(0)
    nwg, P = linln_panel_workgroups(M)
    assert hip.lib().ib_linear_ln_panel_workgroups(M, D, D, ctypes.byref(rows)) == nwg and rows.value == P
    x = _Buf((M, D), BF, inp["x"], c.ldx)
    res = _Buf((M, D), BF, inp["res"], c.ldres) if c.res else None
    bias = _vec(W["bias"]) if c.bias else None
    gamma, beta = _vec(W["gamma"]), _vec(W["beta"])
    y = _Buf((M, D), BF, None, c.ldy)
    _path(hip)
    assert hip.linear_ln_panel_fwd(x.view, _packed(hip, c)[:D * D], bias.view if bias else None, res.view if res else None,
                                   gamma.view, beta.view, y.view, eps=EPS)
    assert _path(hip) == expected_path(c)
    torch.cuda.synchronize()
    assert y.intact(), f"{c.name}: wrote outside y"
    return {"y": y.view}


def _run_linear_panel(hip, c):
    inp, W = make_inputs(c), weights(c.fam, c.N, c.K, c.ffn)
    M = c.M
    assert hip.lib().ib_linear_panel_workgroups(M, c.N, D) == linear_panel_workgroups(M, c.N, D) > 0
    x = _Buf((M, D), BF, inp["x"], c.ldx)
    bias = _vec(W["bias"]) if c.bias else None
    y = _Buf((M, c.N), BF, None, c.ldy)
    _path(hip)
    assert hip.linear_panel_fwd(x.view, _packed(hip, c)[:c.N * D], bias.view if bias else None, y.view)
    assert _path(hip) == expected_path(c)
    torch.cuda.synchronize()
    assert y.intact(), f"{c.name}: wrote outside y (sentinel columns or guards)"
    return {"y": y.view}


def _run_ffn_infer(hip, c):
    inp, W = make_inputs(c), weights(c.fam, c.N, c.K, c.ffn)
    M = c.M
    panels, P, nc, sb = ffn_coop_geometry(M, D, c.ffn)
    rows, pn = ctypes.c_int32(0), ctypes.c_int32(0)
    assert hip.lib().ib_ffn_infer_workgroups(M, D, c.ffn, ctypes.byref(rows), ctypes.byref(pn)) == panels * nc * sb
    assert (rows.value, pn.value) == (P, panels)
    need = ffn_infer_workspace(M, D, c.ffn)
    assert hip.lib().ib_ffn_infer_workspace(M, D, c.ffn) == need == nc * sb * M * D * 4
    x1 = _Buf((M, D), BF, inp["x1"])
    b1, b2, gamma, beta = _vec(W["b1"]), _vec(W["b2"]), _vec(W["gamma"]), _vec(W["beta"])
    y = _Buf((M, D), BF)
    ws = _ws(need // 4)
    _path(hip)
    hip.ffn_infer_fwd(x1.view, _packed(hip, c), b1.view, b2.view, gamma.view, beta.view, y.view, ws, eps=EPS)
    assert _path(hip) == expected_path(c)
    torch.cuda.synchronize()
    assert y.intact(), f"{c.name}: wrote outside y"
    assert torch.isnan(ws[need // 4:]).all(), f"{c.name}: wrote past the {nc * sb} slabs of the workspace"
    return {"slabs": ws[:need // 4].view(nc * sb, M, D), "y": y.view}


def _run_chain(hip, c):
    inp, W = make_inputs(c), weights(c.fam, c.N, c.K, c.ffn)
    M = c.M
    nwg, P, nc = ffn_geometry(M, D, c.ffn)
    rows = ctypes.c_int32(0)
    assert hip.lib().ib_ffn_chain_workgroups(M, D, c.ffn, ctypes.byref(rows)) == nwg and rows.value == P
    x, attn = _Buf((M, D), BF, inp["x"]), _Buf((M, D), BF, inp["attn"])
    v = {k: _vec(W[k]) for k in ("b1", "b2", "gamma", "beta", "bo", "gamma1", "beta1", "bqkv")}
    y = _Buf((M, D), BF)
    qkv = _Buf((M, 3 * D), BF) if c.tail else None
    packed = _packed(hip, c)
    _path(hip)
    assert hip.ffn_chain_fwd_infer(x.view, packed, v["b1"].view, v["b2"].view, v["gamma"].view, v["beta"].view, y.view, attn.view,
                                   v["bo"].view, v["gamma1"].view, v["beta1"].view,
                                   qkv_next=(packed, v["bqkv"].view, qkv.view) if c.tail else None, eps=EPS)
    assert _path(hip) == expected_path(c)
    torch.cuda.synchronize()
    assert y.intact() and (qkv is None or qkv.intact()), f"{c.name}: wrote outside y / qkv"
    out = {"y": y.view}
    if c.tail:
        out["qkv"] = qkv.view
    return out, (x, attn, v, packed)


def _run_chain_training(hip, c, held):
    """ib_ffn_chain_fwd with the attention epilogue (and the tail) on the buffers of _run_chain -> every output it stores"""
    x, attn, v, packed = held
    M = c.M
    o = {"f1": _Buf((M, c.ffn), BF), "s2": _Buf((M, D), BF), "y": _Buf((M, D), BF), "mean": _Buf((M,), F32), "rstd": _Buf((M,), F32),
         "s1": _Buf((M, D), BF), "x1": _Buf((M, D), BF), "mean1": _Buf((M,), F32), "rstd1": _Buf((M,), F32)}
    if c.tail:
        o["qkv"] = _Buf((M, 3 * D), BF)
    mask = torch.zeros(hip.ffn_chain_mask_bytes(M, D, c.ffn), dtype=torch.uint8, device=DEV)
    hip.ffn_chain_fwd(x.view, packed, v["b1"].view, v["b2"].view, v["gamma"].view, v["beta"].view, o["f1"].view, o["s2"].view,
                      o["y"].view, o["mean"].view, o["rstd"].view, mask, eps=EPS,
                      attn_out=(attn.view, v["bo"].view, v["gamma1"].view, v["beta1"].view, o["s1"].view, o["x1"].view,
                                o["mean1"].view, o["rstd1"].view),
                      qkv_next=(packed, v["bqkv"].view, o["qkv"].view) if c.tail else None)
    torch.cuda.synchronize()
    for k, b in o.items():
        assert b.intact(), f"{c.name}: the training form wrote outside {k}"
    return {k: b.view for k, b in o.items()}


def _run_linear_ln(hip, c):
    inp, W = make_inputs(c), weights(c.fam, c.N, c.K, c.ffn)
    M, N, K = c.M, c.N, c.K
    prod, used, asked = linear_ln_plan(M, N, K)
    need = int(hip.lib().ib_linear_ln_fwd_workspace(M, N, K))
    assert need == asked * M * N * 4
    x, w = _Buf((M, K), BF, inp["x"], c.ldx), _Buf((N, K), BF, W["w"])
    res = _Buf((M, N), BF, inp["res"], c.ldres) if c.res else None
    bias = _vec(W["bias"]) if c.bias else None
    gamma, beta = _vec(W["gamma"]), _vec(W["beta"])
    y = _Buf((M, N), BF, None, c.ldy)
    a_out, mean, rstd = (_Buf((M, N), BF), _Buf((M,), F32), _Buf((M,), F32)) if c.saved else (None, None, None)
    ws = _ws(need // 4)
    ptr = lambda b: b.view.data_ptr() if b is not None else None
    _path(hip)
    rc = hip.lib().ib_linear_ln_fwd(ptr(x), c.ldx or K, ptr(w), K, ptr(bias), ptr(res), c.ldres if c.res else 0, ptr(gamma),
                                    ptr(beta), ptr(y), c.ldy, ptr(a_out), ptr(mean), ptr(rstd), ws.data_ptr(), need, M, N, K, EPS,
                                    IB_BF16, hip.stream_ptr())
    assert rc == IB_OK and _path(hip) == expected_path(c)
    torch.cuda.synchronize()
    for name, b in (("y", y), ("a_out", a_out), ("mean", mean), ("rstd", rstd)):
        assert b is None or b.intact(), f"{c.name}: wrote outside {name}"
    slabs = ws[:asked * M * N].view(asked, M * N)
    written = ~torch.isnan(slabs).all(1)
    assert torch.isnan(ws[used * M * N:]).all(), f"{c.name}: wrote past the {used} slabs of the {prod} producer"
    assert torch.isfinite(slabs[:used]).all(), f"{c.name}: a slab element was left unwritten"
    out = {"slab_sum": slabs[:used].sum(0).view(M, N), "nslab": int(written.sum()), "y": y.view}
    if c.saved:
        out.update(a_out=a_out.view, mean=mean.view, rstd=rstd.view)
    return out


def _run(hip, c):
    if c.fam == "chain":
        return _run_chain(hip, c)[0]
    return {"linln_panel": _run_linln_panel, "linear_panel": _run_linear_panel, "ffn_infer": _run_ffn_infer,
            "linear_ln": _run_linear_ln}[c.fam](hip, c)


def _same_bits(a, b):
    iv = torch.int32 if a.dtype == F32 else torch.int16
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(iv), b.contiguous().view(iv))


# ---- every case ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_case(hip, c):
    if c.fam == "chain":
        got, held = _run_chain(hip, c)
    else:
        got = _run(hip, c)
    msgs, worst = check(c, got, DEV)
    print(f"kernel error / bound  {c.name:36s} {worst:.3f}  {c.kernel}")
    assert not msgs, "\n".join(msgs)
    assert worst <= 1.0
    if c.fam == "chain" and c.cross:
        ref, W = reference(c), weights(c.fam, c.N, c.K, c.ffn)
        tr = _run_chain_training(hip, c, held)
        for k, want in (("s1", ref["s1"]), ("x1", ref["x1"]), ("f1", ref["h"]), ("s2", ref["v"])):
            assert torch.equal(tr[k].float().cpu(), want), f"{c.name}: the training form's {k} is not the exact value"
        msgs, worst = check(c, tr, DEV)                                # y (and qkv from ITS y): the staged bounds
        for v, g, b, mk, rk in ((ref["s1"], W["gamma1"], W["beta1"], "mean1", "rstd1"),
                                (ref["v"], W["gamma"], W["beta"], "mean", "rstd")):
            lref, lbnd = ln_reference(v.to(DEV), g, b, *ln_adds(c))
            for k, gk in (("mean", mk), ("rstd", rk)):
                msg, r = violations(f"{c.name} training form {gk}", tr[gk], lref[k].cpu(), lbnd[k].cpu())
                worst = max(worst, r)
                msgs += [msg] if msg else []
        differ = int((tr["y"].view(torch.int16) != got["y"].view(torch.int16)).sum())
        differ_q = int((tr["qkv"].view(torch.int16) != got["qkv"].view(torch.int16)).sum()) if c.tail else 0
        print(f"training form error / bound  {c.name:28s} {worst:.3f}  elements whose bits differ from the INFER form: "
              f"y {differ}, qkv {differ_q}")
        assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("name", ["linln_panel_4100", "linear_panel_417_chunks3", "ffn_infer_321_ffn2048", "ffn_infer_4097_ffn2048",
                                  "chain_8193_ffn2048_tail", "linear_ln_639_N512_K512", "linear_ln_641_N256_K1024"])
def test_two_launches_give_identical_bits(hip, name):
    c = BY_NAME[name]
    a, b = _run(hip, c), _run(hip, c)
    for k in a:
        assert a[k] == b[k] if isinstance(a[k], int) else _same_bits(a[k], b[k]), f"{name}: {k} differs between two launches"


# ---- refusals: IB_E_UNSUPPORTED, nothing written, no path recorded -----------------------------------------------------------
def _refused(hip, what, rc, outs, ws=None):
    torch.cuda.synchronize()
    assert rc == IB_E_UNSUPPORTED, f"{what}: code {rc}"
    assert _path(hip) == PATH_NONE, f"{what}: a launch path was recorded"
    assert all(b.untouched() for b in outs), f"{what}: an output was written"
    assert ws is None or torch.isnan(ws).all(), f"{what}: the workspace was written"


def test_linln_panel_and_linear_panel_refusals(hip):
    lib, s = hip.lib(), hip.stream_ptr()
    M = 8193
    x, y = _Buf((M, D), BF, torch.ones(M, D)), _Buf((M, 3 * D), BF)
    gb = _vec(torch.ones(9 * D))
    img = torch.zeros(9 * D * D, dtype=BF, device=DEV)
    _path(hip)
    rc = lib.ib_linear_ln_panel_fwd(x.view.data_ptr(), D, img.data_ptr(), gb.view.data_ptr(), None, 0, gb.view.data_ptr(),
                                    gb.view.data_ptr(), y.view.data_ptr(), 3 * D, M, D, D, EPS, s)
    _refused(hip, "linln_panel M = 8193", rc, [y])
    rc = lib.ib_linear_panel_fwd(x.view.data_ptr(), D, img.data_ptr(), gb.view.data_ptr(), y.view.data_ptr(), 3 * D, M, 3 * D, D, s)
    _refused(hip, "linear_panel M = 8193", rc, [y])
    y9 = _Buf((64, 9 * D), BF)
    rc = lib.ib_linear_panel_fwd(x.view.data_ptr(), D, img.data_ptr(), gb.view.data_ptr(), y9.view.data_ptr(), 9 * D, 64, 9 * D, D, s)
    _refused(hip, "linear_panel chunks = 9", rc, [y9])
    assert [w for w, _ in REFUSED["linln_panel"] + REFUSED["linear_panel"]] == ["M = 8193", "M = 8193", "chunks = 9"]


def test_ffn_infer_and_chain_refusals(hip):
    lib, s = hip.lib(), hip.stream_ptr()
    packed = torch.zeros((4 * 9 + 8) * D * D, dtype=BF, device=DEV)     # room for nine chunks
    vec = _vec(torch.ones(9 * D))
    p = vec.view.data_ptr()
    for what, a in REFUSED["ffn_infer"]:
        M, d, ffn = a["M"], a["d"], a["ffn"]
        x1, y = _Buf((M, D), BF, torch.ones(M, D)), _Buf((M, D), BF)
        ws = _ws(max(ffn // D, 4) * M * D)
        _path(hip)
        rc = lib.ib_ffn_infer_fwd(x1.view.data_ptr(), packed.data_ptr(), p, p, p, p, y.view.data_ptr(), ws.data_ptr(),
                                  ws.numel() * 4, M, d, ffn, EPS, s)
        _refused(hip, "ffn_infer " + what, rc, [y], ws)
        del ws
    for what, a in REFUSED["chain"]:
        M, d, ffn = a["M"], a["d"], a["ffn"]
        x, attn, y, qkv = _Buf((M, D), BF, torch.ones(M, D)), _Buf((M, D), BF, torch.ones(M, D)), _Buf((M, D), BF), _Buf((M, 3 * D), BF)
        _path(hip)
        rc = lib.ib_ffn_chain_fwd_infer(x.view.data_ptr(), packed.data_ptr(), p, p, p, p, y.view.data_ptr(), attn.view.data_ptr(),
                                        p, p, p, packed.data_ptr(), p, qkv.view.data_ptr(), M, d, ffn, EPS, s)
        _refused(hip, "chain " + what, rc, [y, qkv])


@pytest.mark.parametrize("what", [w for w, _ in REFUSED["linear_ln"]])
def test_linear_ln_refusals(hip, what):
    """N = 192 is a multiple of 64 below 1024 without a slab_ln_kernel instantiation: refused before the GEMM is launched"""
    a = dict(REFUSED["linear_ln"])[what]
    M, N, K = 64, a["N"], a["K"]
    t = F32 if a["dtype"] == IB_F32 else BF
    x, w = _Buf((M, K), t, torch.ones(M, K)), _Buf((N, K), t, torch.ones(N, K))
    res = _Buf((M, N), t, torch.ones(M, N))
    vec = _vec(torch.ones(N))
    y, a_out, mean, rstd = _Buf((M, N), t), _Buf((M, N), t), _Buf((M,), F32), _Buf((M,), F32)
    ws = _ws(16 * M * N)
    p = lambda b: b.view.data_ptr()
    _path(hip)
    rc = hip.lib().ib_linear_ln_fwd(p(x), K, p(w), K, p(vec), p(res), N, p(vec), p(vec), p(y), N, p(a_out), p(mean), p(rstd),
                                    ws.data_ptr(), ws.numel() * 4, M, N, K, EPS, a["dtype"], hip.stream_ptr())
    _refused(hip, "linear_ln " + what, rc, [y, a_out, mean, rstd], ws)
