"""The standalone attention kernels (ib_attention_fwd[_drop] / ib_attention_bwd[_drop]) at every dispatch and tile edge, each
output held ELEMENTWISE to the bound derived in tests/attention_cases.py (float64 reference on the stored inputs; u, u_P,
e_s, eps, eps_b, eta and the two second-order terms are defined and justified there, and tests/test_attention_bounds_cpu.py
shows that the bound admits a correct implementation and rejects six one-line bugs).

Every case of attention_cases.CASES names the path each direction must take (hip.PATH_NAMES: attn_valu, attn_mfma,
attn_mfma_2p, read from ib_debug_last_path() right after the call; "-" = refused).  A case that lands on another path fails:
re-derive the case from the C predicate.  The backward runs twice: on the reference lse rounded to fp32 (the backward alone)
and on the lse the kernel's forward wrote (as training does).

Memory hygiene: out, lse and dqkv are slices of larger buffers, prefilled with NaN (an element left unwritten fails) between
sentinel guards that must survive bit for bit; qkv and dout sit between NaN guards, so a read outside [B, T, .] poisons a
result.  Slices are 16-byte aligned except in the cases that are misaligned on purpose (2-byte-odd offset).

Deviations from a literal reading of the plan, each forced by the dispatch itself:
  * fp32 (T = 152, dh = 128) is the largest dh = 128 shape of the FORWARD; the backward's budget ends at T = 144, so the table
    holds (152, 128) with a refused backward and adds (144, 128) for both directions;
  * `qsplit is only a partition`: at T = 256 no (B, H) reaches qsplit = 1 on the one-pass kernel (B H > 128 is two-pass
    there), so T = 256 compares qsplit = 4 against qsplit = 2, and T = 128 compares qsplit = 2 against qsplit = 1."""
import pytest
import torch

from tests.attention_cases import (BY_NAME, CASES, DROP, DT, REFUSALS, case_inputs, dispatch, evaluate, group_of, make_inputs,
                                   ref_lse, up_of, violations)

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 1536.0                          # exact in bf16 and fp32
GUARD = 64                             # guard elements on each side: 128 / 256 bytes, so the slice stays 16-byte aligned
REDERIVE = "landed on another path: re-derive the case from the C predicate"
RATIOS = {}                            # (path, output) -> largest error / bound seen (reported, never asserted)


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from inferbiomechanics_amd import hip as h
    h.lib()
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    return h


class _Slot:
    """a contiguous tensor of `shape` inside a larger allocation: GUARD elements of `guard` before and after it (`off` more
    before it, to misalign the slice by `off` elements); the slice itself starts as `fill` (a tensor, or a number)"""

    def __init__(self, shape, dtype, guard, fill, off=0):
        n = 1
        for s in shape:
            n *= s
        self.lo = GUARD + off
        self.guard = guard
        self.buf = torch.full((self.lo + n + GUARD,), guard, dtype=dtype, device=DEV)
        self.view = self.buf[self.lo:self.lo + n].view(shape)
        if isinstance(fill, torch.Tensor):
            self.view.copy_(fill.to(dtype))
        else:
            self.view.fill_(fill)
        assert self.view.is_contiguous() and (self.view.data_ptr() % 16 == 0) == (off == 0)

    def guards_intact(self):
        g = torch.full_like(self.buf, self.guard)
        n = self.view.numel()
        return torch.equal(self.buf[:self.lo], g[:self.lo]) and torch.equal(self.buf[self.lo + n:], g[self.lo + n:])


def _src(t, off=0):
    return _Slot(tuple(t.shape), t.dtype, float("nan"), t, off)


def _dst(shape, dtype, off=0, fill=float("nan")):
    return _Slot(shape, dtype, SENT, fill, off)


def _call(hip, fn):
    """run fn -> (the HipError it raised or None, the path the dispatch stamped on this thread)"""
    lib = hip.lib()
    lib.ib_debug_last_path()                                   # read-and-clear
    err = None
    try:
        fn()
    except hip.HipError as e:
        err = e
    path = hip.PATH_NAMES[int(lib.ib_debug_last_path())]
    torch.cuda.synchronize()
    return err, path


def _note(path, what, ratio):
    RATIOS[(path, what)] = max(RATIOS.get((path, what), 0.0), ratio)


def _split_ratios(path, got, ref, bound, H, dh):
    d = H * dh
    for i, part in enumerate(("dQ", "dK", "dV")):
        s = slice(i * d, (i + 1) * d)
        g = got[..., s].detach().cpu().double()
        if torch.isfinite(g).all():
            _note(path, part, float(((g - ref[..., s]).abs() / bound[..., s]).max()))


def run_case(hip, c):
    x = case_inputs(c)
    B, T, H, dh = c.B, c.T, c.H, c.dh
    d, dt = H * dh, DT[c.dt]
    mis = c.opt.get("misalign")
    drop = DROP if c.opt.get("drop") else None
    qkv, dout = _src(x.qkv, 1 if mis == "qkv" else 0), _src(x.dout)
    out, lse = _dst((B, T, d), dt), _dst((B, H, T), torch.float32)
    err, pf = _call(hip, lambda: hip.attention_fwd(qkv.view, out.view, lse.view, H, drop=drop))
    assert err is None, (c.name, err)
    assert pf == c.fwd, f"{c.name}: forward {REDERIVE} ({pf}, expected {c.fwd})"
    mask = hip.attention_drop_mask(B, T, H, drop, DEV).cpu() if drop else None
    lse_ref32 = ref_lse(x).float()
    lse_k = lse.view.detach().cpu().clone()
    runs = []
    for given in ((lse_ref32, lse_k) if c.bwd != "-" else ()):
        dq = _dst((B, T, 3 * d), dt, 1 if mis == "dqkv" else 0)
        lin = _src(given)
        err, pb = _call(hip, lambda: hip.attention_bwd(qkv.view, out.view, dout.view, lin.view, dq.view, H, drop=drop))
        assert err is None, (c.name, err)
        assert pb == c.bwd, f"{c.name}: backward {REDERIVE} ({pb}, expected {c.bwd})"
        runs.append(dq)
    if c.bwd == "-":                                                # the backward refuses this shape and writes nothing
        dq = _dst((B, T, 3 * d), dt, fill=SENT)
        err, pb = _call(hip, lambda: hip.attention_bwd(qkv.view, out.view, dout.view, lse.view, dq.view, H, drop=drop))
        assert err is not None and pb == "-", (c.name, err, pb)
        assert torch.equal(dq.buf, torch.full_like(dq.buf, SENT)), "a refused backward wrote to dqkv"
    ref, bound = evaluate(x, c.dt, up_of(c.fwd), up_of(c.bwd), mask, [lse_ref32, lse_k.nan_to_num()][:len(runs)])
    msgs = []
    for what, got, r, b, path in [("O", out.view, ref["O"], bound["O"], pf), ("lse", lse.view, ref["lse"], bound["lse"], pf)] \
            + [("dqkv", dq.view, ref["dqkv"], bound["dqkv"][i], c.bwd) for i, dq in enumerate(runs)]:
        msg, ratio = violations(what, got, r, b, H, path)
        if msg:
            msgs.append(msg + (f" [backward on the {'reference' if got is runs[0].view else 'kernel'} lse]"
                               if what == "dqkv" else ""))
        if what == "dqkv":
            _split_ratios(path, got, r, b, H, dh)
        else:
            _note(path, what, ratio)
    for name, slot in [("qkv", qkv), ("dout", dout), ("out", out), ("lse", lse)] + [("dqkv", dq) for dq in runs]:
        if name in ("qkv", "dout"):                                 # NaN guards: untouched = still all NaN
            n = slot.view.numel()
            ok = bool(slot.buf[:slot.lo].isnan().all() and slot.buf[slot.lo + n:].isnan().all()) \
                and torch.equal(slot.view, (x.qkv if name == "qkv" else x.dout).to(DEV))
        else:
            ok = slot.guards_intact()
        if not ok:
            msgs.append(f"{name}: memory outside the tensor (or an input) was written")
    assert not msgs, c.name + "\n" + "\n".join(msgs)


def _cases(group):
    sel = [c for c in CASES if group_of(c) == group]
    assert sel
    return pytest.mark.parametrize("c", sel, ids=[c.name for c in sel])


@_cases("mfma_one_pass")
def test_mfma_one_pass(hip, c):
    run_case(hip, c)


@_cases("mfma_two_pass")
def test_mfma_two_pass(hip, c):
    run_case(hip, c)


@_cases("bf16_valu")
def test_bf16_outside_the_mfma_domain(hip, c):
    run_case(hip, c)


@_cases("fp32_valu")
def test_fp32_valu(hip, c):
    run_case(hip, c)


@_cases("dropout")
def test_probability_dropout(hip, c):
    run_case(hip, c)


# ---- refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,B,T,H,dh,fwd,bwd", REFUSALS, ids=[f"{r[0]}_T{r[2]}_dh{r[4]}" for r in REFUSALS])
def test_refusals(hip, dt, B, T, H, dh, fwd, bwd):
    """a refused call raises HipError, leaves path "-" and the sentinel-filled outputs untouched.  fp32 (T = 256, dh = 73 .. 76)
    fits the forward's LDS budget and not the backward's: pinned as it is (attention section)."""
    x = make_inputs(dt, B, T, H, dh, "gauss", 7)
    d = H * dh
    qkv, dout = _src(x.qkv), _src(x.dout)
    out, lse = _dst((B, T, d), DT[dt], fill=SENT), _dst((B, H, T), torch.float32, fill=SENT)
    dq = _dst((B, T, 3 * d), DT[dt], fill=SENT)
    untouched = lambda s: torch.equal(s.buf, torch.full_like(s.buf, SENT))
    err, pf = _call(hip, lambda: hip.attention_fwd(qkv.view, out.view, lse.view, H))
    assert pf == fwd and (err is not None) == (fwd == "-"), (err, pf)
    if fwd == "-":
        assert untouched(out) and untouched(lse), "a refused forward wrote to its outputs"
        lse_in = _src(ref_lse(x).float())
        out_in = _src(torch.zeros(B, T, d, dtype=DT[dt]))
    else:
        assert out.guards_intact() and lse.guards_intact() and bool(torch.isfinite(out.view.float()).all())
        lse_in, out_in = lse, out
    err, pb = _call(hip, lambda: hip.attention_bwd(qkv.view, out_in.view, dout.view, lse_in.view, dq.view, H))
    assert pb == bwd == "-" and err is not None, (err, pb)
    assert untouched(dq), "a refused backward wrote to dqkv"
    for p in (DROP,):                                               # the _drop entry points refuse the same shapes
        err, pf2 = _call(hip, lambda: hip.attention_fwd(qkv.view, out.view, lse.view, H, drop=p))
        assert pf2 == fwd and (err is not None) == (fwd == "-")
        err, pb2 = _call(hip, lambda: hip.attention_bwd(qkv.view, out_in.view, dout.view, lse_in.view, dq.view, H, drop=p))
        assert pb2 == "-" and err is not None and untouched(dq)


# ---- properties ----------------------------------------------------------------------------------------------------------
def _fwd_bwd(hip, qkv, dout, H, expect=None):
    """plain run on device tensors -> (out, lse, dqkv); the backward consumes the forward's lse"""
    B, T, d3 = qkv.shape
    out = torch.full((B, T, d3 // 3), float("nan"), dtype=qkv.dtype, device=DEV)
    lse = torch.full((B, H, T), float("nan"), dtype=torch.float32, device=DEV)
    dqkv = torch.full((B, T, d3), float("nan"), dtype=qkv.dtype, device=DEV)
    err, pf = _call(hip, lambda: hip.attention_fwd(qkv, out, lse, H))
    assert err is None and (expect is None or pf == expect[0]), (err, pf, expect)
    err, pb = _call(hip, lambda: hip.attention_bwd(qkv, out, dout, lse, dqkv, H))
    assert err is None and (expect is None or pb == expect[1]), (err, pb, expect)
    return out, lse, dqkv


PROPERTY_CASES = ["mfma1p_bf16_b2h2_T65_dh64_gauss", "mfma2p_bf16_b32h8_T65_dh64_gauss", "valu_fp32_b2h3_T5_dh65_gauss"]


@pytest.mark.parametrize("name", PROPERTY_CASES)
def test_repeatable_and_equivariant(hip, name):
    """two runs are bit-identical, and permuting the windows / the heads of the inputs permutes every output bit for bit (a
    b / h indexing slip that random data and a max-norm tolerance hide)"""
    c = BY_NAME[name]
    x = case_inputs(c)
    B, T, H, dh = c.B, c.T, c.H, c.dh
    qkv, dout = x.qkv.to(DEV), x.dout.to(DEV)
    a = _fwd_bwd(hip, qkv, dout, H, (c.fwd, c.bwd))
    b = _fwd_bwd(hip, qkv, dout, H, (c.fwd, c.bwd))
    assert all(torch.equal(s, t) for s, t in zip(a, b)), "two runs differ"
    assert all(bool(torch.isfinite(s.float()).all()) for s in a)
    pw = torch.arange(B - 1, -1, -1, device=DEV)                     # the windows, then the heads, in reverse order
    w = _fwd_bwd(hip, qkv[pw].contiguous(), dout[pw].contiguous(), H, (c.fwd, c.bwd))
    assert all(torch.equal(s[pw], t) for s, t in zip(a, w)), "a window permutation does not permute the outputs"
    ph = torch.arange(H - 1, -1, -1, device=DEV)
    hp = lambda t, k: t.reshape(B, T, k, H, dh)[:, :, :, ph].reshape(B, T, k * H * dh).contiguous()
    h = _fwd_bwd(hip, hp(qkv, 3), hp(dout, 1), H, (c.fwd, c.bwd))
    assert torch.equal(hp(a[0], 1), h[0]) and torch.equal(a[1][:, ph], h[1]) and torch.equal(hp(a[2], 3), h[2]), \
        "a head permutation does not permute the outputs"


@pytest.mark.parametrize("T,H,few,many,qs", [(128, 2, 1, 65, (2, 1)), (256, 2, 1, 63, (4, 2))])
def test_qsplit_is_only_a_partition(hip, T, H, few, many, qs):
    """window 0 alone (its query blocks split over several workgroups) is bit-identical to window 0 inside a batch that
    splits less, both on the one-pass kernel"""
    assert dispatch("bf16", few, T, H, 64)["qsplit"] == qs[0] and dispatch("bf16", many, T, H, 64)["qsplit"] == qs[1]
    assert not dispatch("bf16", few, T, H, 64)["two_pass"] and not dispatch("bf16", many, T, H, 64)["two_pass"]
    x = make_inputs("bf16", many, T, H, 64, "gauss", 11)
    qkv, dout = x.qkv.to(DEV), x.dout.to(DEV)
    big = _fwd_bwd(hip, qkv, dout, H, ("attn_mfma", "attn_mfma"))
    one = _fwd_bwd(hip, qkv[:few].contiguous(), dout[:few].contiguous(), H, ("attn_mfma", "attn_mfma"))
    assert all(torch.equal(s[:few], t) for s, t in zip(big, one))


def test_one_pass_against_two_pass(hip, record_property):
    """T = 129 on both sides of the two-pass edge (127 windows one-pass, 128 two-pass): the shared windows agree within the
    bound.  Whether they are in fact bit-identical is recorded, not required: the two kernels sum the row in another order."""
    H, T = 1, 129
    x = make_inputs("bf16", 128, T, H, 64, "gauss", 13)
    qkv, dout = x.qkv.to(DEV), x.dout.to(DEV)
    two = _fwd_bwd(hip, qkv, dout, H, ("attn_mfma_2p", "attn_mfma"))
    one = _fwd_bwd(hip, qkv[:127].contiguous(), dout[:127].contiguous(), H, ("attn_mfma", "attn_mfma"))
    sub = type(x)(x.qkv[:127], x.dout[:127], H, 64)
    _, bound = evaluate(sub, "bf16", up_of("attn_mfma"), up_of("attn_mfma"))
    same = bool(torch.equal(one[0], two[0][:127]) and torch.equal(one[1], two[1][:127]))
    record_property("one_pass_equals_two_pass_bitwise", same)
    print(f"one-pass and two-pass forward bit-identical at T = 129: {same}")
    for what, i in (("O", 0), ("lse", 1)):
        diff = (one[i].cpu().double() - two[i][:127].cpu().double()).abs()
        assert bool((diff <= bound[what]).all()), (what, float((diff / bound[what]).max()))
