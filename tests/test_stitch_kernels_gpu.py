"""ib_stitch_ddim_step / ib_stitch_dpmpp_step on the GPU (csrc/stitch.hip).  -m gpu.

Shapes: windows of T = 8 frames every hop = 3 over a trial of F = 17 frames, so W = 4 windows and 1 .. 3 of them cover a
frame; N = 2 trials; (D, ld) = (12, 16) takes the 8-wide kernel, (5, 5) the element-wise one; fp32 and bf16; with and without
observations; DDIM and DPM-Solver++ rows with C = 0 and C != 0.

(a) With F = T (one window) the stitched entries equal ib_ddim_step / ib_ddim_cond_step / ib_dpmpp_step /
    ib_dpmpp_cond_step bit for bit, history included.  Where ld % 8 != 0 and the flat kernels still go 8-wide (T * ld = 40 is a
    multiple of 8 here, whatever ld is) they key their rounding by flat offset and the stitched kernel keys it by column, so
    two things are left out there and nowhere else: the free bf16 elements (fp32 has one 8-wide form, so it is compared), and
    the observed elements, which the flat 8-wide kernel rounds per position in the vector and the stitched kernel as a lone
    element (obs_pin1) -- (d) pins those exactly instead.  The same (5, 5) buffers moved off 16-byte alignment make the flat
    kernels element-wise too, and then everything is compared bit for bit, bf16 included.
(b) After a step from consistent copies all copies are bitwise equal, in x and in hist.
(c) Every output lies within a bound derived from the operation count, see bound().
(d) Observed elements equal the pinned expression exactly; pad columns stay 0.
(e) The argument refusals."""
import numpy as np
import pytest
import torch

from tests.exact_fp32 import pinned

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
T, HOP, F, N, S = 8, 3, 17, 2, 6
GEOM = [(12, 16), (5, 5)]
U32, UBF = 2.0 ** -24, 2.0 ** -8          # unit roundoffs 2^-p of round-to-nearest: fp32 p = 24 significand bits, bf16 p = 8


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from inferbiomechanics_amd import hip
    hip.lib()


@pytest.fixture(scope="module")
def tabs():
    from inferbiomechanics_amd.diffusion.schedule import DiffusionTables
    t = DiffusionTables(torch.device(DEV), num_sample_steps=10)
    t.set_sampler(S, 0.0, "dpmpp2m", "logsnr")
    c5 = t.dpmpp_coef.cpu()
    assert float(c5[0, 2]) == 0.0 == float(c5[-1, 2]) and bool((c5[1:-1, 2] != 0).all())
    return t


def layout(frames):
    from inferbiomechanics_amd.diffusion.schedule import stitch_layout
    start, cover, wn, _ = stitch_layout(frames, T, HOP, "ramp")
    gather = start.long()[:, None] + torch.arange(T)[None, :]
    return {"start": start, "cover": cover, "wn": wn, "gather": gather, "W": start.numel(), "F": frames,
            "dev": (start.to(DEV), cover.to(DEV), wn.to(DEV))}


def col_mask(D, ld):
    """[T, ld] uint8, the same columns in every frame: (12, 16) has an all-observed vector (columns 0 .. 7) and a mixed one
    (8 and 10 observed, pad columns free); (5, 5) observes columns 0 and 3"""
    m = torch.zeros(T, ld, dtype=torch.uint8)
    cols = list(range(8)) + [8, 10] if ld == 16 else [0, 3]
    m[:, cols] = 3
    return m


def checker_mask(D, ld):
    m = torch.zeros(T, ld, dtype=torch.uint8)
    m[:, :D] = ((torch.arange(T).reshape(-1, 1) + torch.arange(D).reshape(1, -1)) % 2).to(torch.uint8) * 5
    return m


def guarded(shape, dt, shift=0):
    """zeros of `shape` `shift` elements into a flat buffer that ends in 64 sentinels no kernel may touch"""
    n = int(np.prod(shape))
    flat = torch.full((shift + n + 64,), 7.0, dtype=dt, device=DEV)
    v = flat[shift:shift + n].view(shape)
    v.zero_()
    return flat, v


def sentinels_ok(flat):
    return bool((flat[-64:] == 7.0).all())


def operands(lay, D, ld, dt, seed, shift=0):
    """consistent window-batch operands: x, hist, x0, z are gathered from trial tensors [N, F, ld] (pad columns 0), eps is
    drawn per window"""
    g = torch.Generator().manual_seed(seed)
    W = lay["W"]

    def trial(dtype, scale=1.0):
        t = torch.zeros(N, lay["F"], ld)
        t[:, :, :D] = scale * torch.randn(N, lay["F"], D, generator=g)
        return t.to(dtype)

    out = {}
    for name, dtype, scale in (("x", dt, 1.0), ("hist", torch.float32, 3.0), ("x0", dt, 1.0), ("z", dt, 1.0)):
        tr = trial(dtype, scale)
        flat, v = guarded((N, W, T, ld), dtype, shift)
        v.copy_(tr[:, lay["gather"]].to(DEV))
        out[name], out[name + "_flat"], out[name + "_trial"] = v, flat, tr
    e = torch.zeros(N, W, T, ld)
    e[..., :D] = torch.randn(N, W, T, D, generator=g)
    flat, v = guarded((N, W, T, ld), dt, shift)
    v.copy_(e.to(dt).to(DEV))
    out["eps"], out["eps_flat"] = v, flat
    return out


def run_stitch(hip, tabs, lay, op, solver, cond, mask, s, D, by_counter=True):
    """one stitched launch on clones of op -> (x, hist, t_out, x's flat buffer, hist's flat buffer)"""
    W = lay["W"]
    shift = op["x"].storage_offset()
    xf, x = guarded(op["x"].shape, op["x"].dtype, shift)
    hf, h = guarded(op["x"].shape, torch.float32, shift)
    x.copy_(op["x"])
    h.copy_(op["hist"])
    ctr = torch.tensor([s], dtype=torch.int32, device=DEV)
    t_out = torch.full((N * W,), -7, dtype=torch.int64, device=DEV)
    c = (op["x0"], op["z"], mask.to(DEV), tabs.obs_coef) if cond else (None, None, None, None)
    st, cv, wn = lay["dev"]
    kw = dict(step_dev=ctr, t_out=t_out) if by_counter else dict(step=s, t_out=t_out)
    if solver == "dpmpp":
        hip.stitch_dpmpp_step(x, op["eps"], h, c[0], c[1], c[2], tabs.dpmpp_coef, c[3], tabs.ddim_t, st, cv, wn, D=D, **kw)
    else:
        hip.stitch_ddim_step(x, op["eps"], c[0], c[1], c[2], tabs.ddim_coef, c[3], tabs.ddim_t, st, cv, wn, D=D, **kw)
    torch.cuda.synchronize()
    return x, h, t_out, xf, hf


def run_flat(hip, tabs, op, solver, cond, mask, s, D):
    """the existing entry point on the same buffers seen as [N, T, ld] (W = 1)"""
    shape3 = (N, T, op["x"].shape[-1])
    shift = op["x"].storage_offset()
    _, x = guarded(shape3, op["x"].dtype, shift)
    _, h = guarded(shape3, torch.float32, shift)
    x.copy_(op["x"].view(shape3))
    h.copy_(op["hist"].view(shape3))
    eps, x0, z = (op[k].view(shape3) for k in ("eps", "x0", "z"))
    if solver == "dpmpp" and cond:
        hip.dpmpp_cond_step(x, eps, h, x0, z, mask.to(DEV), tabs.dpmpp_coef, tabs.obs_coef, tabs.ddim_t, step=s, D=D)
    elif solver == "dpmpp":
        hip.dpmpp_step(x, eps, h, tabs.dpmpp_coef, tabs.ddim_t, step=s)
    elif cond:
        hip.ddim_cond_step(x, eps, x0, z, mask.to(DEV), tabs.ddim_coef, tabs.obs_coef, tabs.ddim_t, step=s, D=D)
    else:
        hip.ddim_step(x, eps, tabs.ddim_coef, tabs.ddim_t, step=s)
    torch.cuda.synchronize()
    return x, h


CASES = [(dt, D, ld, solver, cond) for dt in (torch.float32, BF) for D, ld in GEOM for solver in ("ddim", "dpmpp")
         for cond in (False, True)]


# ---------------------------------------------------------------------------------------------------------------------
# (a) one window: the existing kernels, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def left_out_of_one_window_comparison(dt, ld, shift):
    """What check (a) does NOT compare bit for bit, and the only place that says so: (free x, observed x and the history
    at observed elements).  Everything is compared unless the flat kernels run 8-wide over a row pitch that is no multiple
    of 8 -- ld % 8 != 0 with aligned buffers (shift == 0; T * ld = 40 is a multiple of 8 whatever ld is).  There they key
    their rounding by flat offset and the stitched kernel, element-wise, by column:
      free x      left out for bf16 only (ddim_mix<bf16, 8> alternates by position; fp32 has one 8-wide form, so it is compared)
      observed x  left out: the flat kernel rounds an observed element per position in its vector, the stitched kernel as a
                  lone element (obs_pin1); check (d) pins those values exactly instead
      history at observed elements  left out: unspecified there (include/ib_hip_stitch.h); the history of free elements
                  is always compared
    Nothing else may be added here: ld % 8 == 0 and the off-alignment runs compare every element."""
    by_offset = ld % 8 != 0 and shift == 0
    return by_offset and dt == BF, by_offset, by_offset


# shift = 1: the buffers start one element off 16-byte alignment (the element-wise comparison of ld % 8 != 0)
@pytest.mark.parametrize("dt,D,ld,solver,cond,shift", [c + (0,) for c in CASES] + [c + (1,) for c in CASES if c[2] % 8])
def test_one_window_equals_the_existing_kernels(tabs, dt, D, ld, solver, cond, shift):
    from inferbiomechanics_amd import hip
    lay = layout(T)
    assert lay["W"] == 1
    op = operands(lay, D, ld, dt, 100 + D + (dt == BF), shift)
    for mask in ((col_mask(D, ld), checker_mask(D, ld)) if cond else (None,)):
        for s in (0, 2, S - 1):                                        # C == 0, C != 0, the last row
            x, h, t_out, xf, hf = run_stitch(hip, tabs, lay, op, solver, cond, mask, s, D)
            fx, fh = run_flat(hip, tabs, op, solver, cond, mask, s, D)
            x3, h3 = x.view(N, T, ld), h.view(N, T, ld)
            free = torch.ones(T, ld, dtype=torch.bool) if mask is None else ~mask.bool()
            free, obs = free.to(DEV), ~free.to(DEV)
            skip_free, skip_obs, skip_obs_hist = left_out_of_one_window_comparison(dt, ld, shift)
            diff = int((x3[:, free] != fx[:, free]).sum())
            print(f"{dt} ld={ld} {solver} cond={cond} shift={shift} s={s}: {diff} free elements differ, "
                  f"{int((x3[:, obs] != fx[:, obs]).sum())} observed, {int((h3[:, free] != fh[:, free]).sum())} history")
            if not skip_free:
                assert torch.equal(x3[:, free], fx[:, free]), (s, "free elements")
            if not skip_obs:
                assert torch.equal(x3[:, obs], fx[:, obs]), (s, "observed elements")
            if solver == "dpmpp":
                assert torch.equal(h3[:, free], fh[:, free]), (s, "history")
                if not skip_obs_hist:
                    assert torch.equal(h3, fh), (s, "history at observed elements")
            assert sentinels_ok(xf) and sentinels_ok(hf)
            assert bool((t_out == (int(tabs.ddim_t[s + 1]) if s + 1 < S else 0)).all())


# ---------------------------------------------------------------------------------------------------------------------
# (b), (c), (d): overlapping windows
# ---------------------------------------------------------------------------------------------------------------------
def bound(count, mag, ref, dt):
    """|computed - float64 value| of one element.  fp32 roundings: the blend of `count` windows rounds `count` times (one
    product, count - 1 fused multiply-adds; none for one window), each by at most u times a partial sum that Sum |w_k e_k|
    bounds; the update rounds at most twice beyond that (its fused forms round one product and the result; the lone form
    rounds both products, whose magnitudes add up to at most `mag`, and the sum), and the history term C h is one more fused
    multiply-add.  Every rounded intermediate is at most mag = |cx y| + |ce| Sum |w_k e_k| + |C h| in magnitude, so the fp32
    error is at most gamma(count + 3) mag with gamma(n) = n u / (1 - n u), u = 2^-24.  Storing the state rounds once more, by
    u_state times the stored magnitude (at most |ref| plus the fp32 error)."""
    n = count + 3
    e32 = (n * U32 / (1 - n * U32)) * mag
    return e32 + (UBF if dt == BF else U32) * (ref.abs() + e32)


@pytest.mark.parametrize("dt,D,ld,solver,cond", CASES)
def test_overlapping_windows_invariant_bound_and_observed(tabs, dt, D, ld, solver, cond):
    from inferbiomechanics_amd import hip
    lay = layout(F)
    W = lay["W"]
    st, cv, wn = lay["start"].tolist(), lay["cover"].tolist(), lay["wn"]
    assert W == 4 and sorted({c for _, c in cv}) == [1, 2, 3]
    op = operands(lay, D, ld, dt, 200 + D + (dt == BF))
    mask = col_mask(D, ld) if cond else None
    obs_cols = mask[0].bool() if cond else torch.zeros(ld, dtype=torch.bool)
    vec = ld % 8 == 0
    Y, H, X0, Z = (op[k + "_trial"].double() for k in ("x", "hist", "x0", "z"))
    E = op["eps"].cpu().double()
    cnt = torch.tensor([c for _, c in cv], dtype=torch.float64)[None, :, None]
    # the windows' eps of every trial frame, slot k = k-th covering window (0 beyond the count)
    Ek = torch.zeros(8, N, F, ld, dtype=torch.float64)
    for f, (w0, c) in enumerate(cv):
        for k in range(c):
            Ek[k, :, f] = E[:, w0 + k, f - st[w0 + k]]
    Wk = wn.double().t()[:, None, :, None]                             # the fp32 weights the kernel reads
    eb, eb_abs = (Wk * Ek).sum(0), (Wk * Ek).abs().sum(0)
    coef2, coef5, oc = tabs.ddim_coef.cpu().double(), tabs.dpmpp_coef.cpu().double(), tabs.obs_coef.cpu().double()
    for s in (0, 2, S - 1):
        x, h, t_out, xf, hf = run_stitch(hip, tabs, lay, op, solver, cond, mask, s, D)
        x2, h2, _, _, _ = run_stitch(hip, tabs, lay, op, solver, cond, mask, s, D, by_counter=False)
        assert torch.equal(x, x2) and torch.equal(h, h2), "host step index and device step counter disagree"
        assert sentinels_ok(xf) and sentinels_ok(hf), "wrote past the state or the history"
        assert bool((t_out == (int(tabs.ddim_t[s + 1]) if s + 1 < S else 0)).all())
        xc, hc = x.cpu(), h.cpu()
        # (b) every copy holds the bits of the first copy
        first = torch.stack([xc[:, w0, f - st[w0]] for f, (w0, _) in enumerate(cv)], dim=1)          # [N, F, ld]
        first_h = torch.stack([hc[:, w0, f - st[w0]] for f, (w0, _) in enumerate(cv)], dim=1)
        assert torch.equal(xc, first[:, lay["gather"]]), (s, "copies of x differ")
        if solver == "dpmpp":
            free_c = ~obs_cols
            assert torch.equal(hc[..., free_c], first_h[:, lay["gather"]][..., free_c]), (s, "copies of hist differ")
            if vec:                                                    # a mixed vector writes hist at its observed elements too
                assert torch.equal(hc, first_h[:, lay["gather"]]), (s, "copies of hist differ at observed elements")
        # (c) free elements against float64
        if solver == "dpmpp":
            cx, ce, ch, hx, he = (float(v) for v in coef5[s])
        else:
            (cx, ce), ch, hx, he = (float(v) for v in coef2[s]), 0.0, 0.0, 0.0
        want = cx * Y + ce * eb + ch * H
        mag = (cx * Y).abs() + abs(ce) * eb_abs + (ch * H).abs()
        tol = bound(cnt, mag, want, dt)
        err = (first.double() - want).abs()
        fc = ~obs_cols
        worst = float((err[..., fc] / tol[..., fc].clamp_min(1e-300)).max())
        print(f"{dt} ld={ld} {solver} cond={cond} s={s}: state error at most {worst:.3f} of the bound "
              f"(max err {float(err[..., fc].max()):.3e})")
        assert bool((err[..., fc] <= tol[..., fc]).all()), (s, worst)
        if solver == "dpmpp":
            want_h = hx * Y + he * eb
            tol_h = bound(cnt, (hx * Y).abs() + abs(he) * eb_abs, want_h, torch.float32)
            err_h = (first_h.double() - want_h).abs()
            print(f"    history error at most {float((err_h[..., fc] / tol_h[..., fc].clamp_min(1e-300)).max()):.3f} of the bound")
            assert bool((err_h[..., fc] <= tol_h[..., fc]).all()), (s, "history")
        # (d) observed elements: the pinned expression, exactly; pad columns stay 0
        assert not xc[..., D:].any() and not hc[..., D:].any(), "pad columns must stay 0"
        if cond:
            ox, oz = tabs.obs_coef.cpu()[s + 1].tolist()
            x0t, zt = op["x0_trial"].float(), op["z_trial"].float()
            for c in torch.nonzero(obs_cols).flatten().tolist():
                exp = torch.tensor([[float(pinned(ox, x0t[n, f, c], oz, zt[n, f, c], c & 7, vec)) for f in range(F)]
                                    for n in range(N)], dtype=torch.float32).to(dt)
                assert torch.equal(first[:, :, c], exp), (s, c, "observed elements are not the pinned expression")
            if s == S - 1:
                assert torch.equal(first[..., obs_cols], op["x0_trial"][..., obs_cols]), "the last step lands on the observation"


# ---------------------------------------------------------------------------------------------------------------------
# (e) refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_refusals(tabs):
    from inferbiomechanics_amd import hip
    lay = layout(F)
    W, D, ld = lay["W"], 12, 16
    op = operands(lay, D, ld, torch.float32, 7)
    mask = col_mask(D, ld).to(DEV)
    st, cv, wn = lay["dev"]
    p = lambda t: None if t is None else t.data_ptr()
    base = dict(x=p(op["x"]), eps=p(op["eps"]), hist=p(op["hist"]), x0=p(op["x0"]), z=p(op["z"]), mask=p(mask),
                coef=None, obs_coef=p(tabs.obs_coef), timesteps=p(tabs.ddim_t), num_steps=S, step=0, step_dev=None,
                t_out=None, start=p(st), cover=p(cv), wn=p(wn), N=N, W=W, T=T, F=F, D=D, ld=ld, dtype=hip.F32, stream=0)

    def call(dpm, **over):
        a = dict(base, coef=p(tabs.dpmpp_coef if dpm else tabs.ddim_coef))
        a.update(over)                                                 # keeps the header's order of the keys
        if not dpm:
            a.pop("hist")
        fn = hip.lib().ib_stitch_dpmpp_step if dpm else hip.lib().ib_stitch_ddim_step
        return fn(*a.values())

    ARG, DTYPE, UNSUP = -1, -2, -5
    before = op["x"].clone()
    for dpm in (False, True):
        for name in ("x", "eps", "coef", "start", "cover", "wn"):
            assert call(dpm, **{name: None}) == ARG, name
        for name in ("x0", "z", "mask", "obs_coef"):                   # any mix of NULL and non-NULL
            assert call(dpm, **{name: None}) == ARG, name
            rest = {k: None for k in ("x0", "z", "mask", "obs_coef") if k != name}
            assert call(dpm, **rest) == ARG, name
        for name in ("N", "W", "T", "F", "D", "num_steps"):
            assert call(dpm, **{name: 0}) == ARG, name
        assert call(dpm, ld=D - 1) == ARG
        assert call(dpm, F=T - 1) == ARG
        assert call(dpm, t_out=p(torch.zeros(N * W, dtype=torch.int64, device=DEV)), timesteps=None) == ARG
        assert call(dpm, dtype=7) == DTYPE
        assert call(dpm, T=1 << 20, F=1 << 20, ld=1 << 11, D=1 << 11) == UNSUP
    assert call(True, hist=None) == ARG
    torch.cuda.synchronize()
    assert torch.equal(op["x"], before), "a refused call must launch nothing"
    with pytest.raises(hip.HipError, match="start"):                   # the binding owns the tables' validity
        bad = st.clone()
        bad[-1] += 1
        hip.stitch_ddim_step(op["x"], op["eps"], None, None, None, tabs.ddim_coef, None, tabs.ddim_t, bad, cv, wn, D=D)
    with pytest.raises(hip.HipError, match="wn"):
        hip.stitch_ddim_step(op["x"], op["eps"], None, None, None, tabs.ddim_coef, None, tabs.ddim_t, st, cv, wn[:, :4], D=D)
    with pytest.raises(hip.HipError, match="cover"):
        hip.stitch_ddim_step(op["x"], op["eps"], None, None, None, tabs.ddim_coef, None, tabs.ddim_t, st, cv.long(), wn, D=D)
    with pytest.raises(hip.HipError, match="device"):
        hip.stitch_ddim_step(op["x"], op["eps"], None, None, None, tabs.ddim_coef, None, tabs.ddim_t, st.cpu(), cv, wn, D=D)
