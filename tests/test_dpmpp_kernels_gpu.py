"""The DPM-Solver++(2M) update on the GPU: ib_dpmpp_step / ib_dpmpp_cond_step against a float64 evaluation of the fp32 table
values on the kernel's own inputs (state and fp32 history, every step of a table, element-wise / 8-wide / pitched, fp32 and
bf16, four masks), the bitwise relations to the DDIM entries (observed elements; rows with C == 0, whose history may hold
anything), the Gaussian closed-form problem of tests/test_dpmpp_plumbing_cpu.py through the real kernel, and a captured
step replayed against the eager loop.  -m gpu."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
ARITH = {torch.float32: 2e-6, BF: 8e-3}      # tests/test_eta_kernels_gpu.py: the state's bound, x max |want|
HIST = 2e-6                                  # the history is fp32 in both dtypes


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from inferbiomechanics_amd import hip
    hip.lib()


# the geometries of tests/test_eta_kernels_gpu.py::SHAPES, each in both dtypes
GEOM = [(3, 10, 177, 177),       # element-wise kernel (T * ld % 8 != 0)
        (4, 10, 177, 177),       # element-wise, with the rounding of ib_ddim_step's 8-wide kernel
        (3, 24, 44, 44),         # 8-wide, unpitched
        (3, 24, 44, 48),         # 8-wide, pitched
        (3, 10, 177, 192),       # 8-wide, pitched 177 -> 192
        (2, 10, 300, 320)]       # the benched row
SHAPES = [(dt,) + g for dt in (torch.float32, BF) for g in GEOM]
S6 = 6


def guarded(B, T, ld, D, dt, g, scale=1.0):
    """a [B, T, ld] view (pad columns 0) in front of 64 sentinel elements no kernel may touch"""
    flat = torch.full((B * T * ld + 64,), 7.0, dtype=dt)
    v = flat[:B * T * ld].view(B, T, ld)
    v.zero_()
    v[:, :, :D] = (scale * torch.randn(B, T, D, generator=g)).to(dt)
    flat = flat.to(DEV)
    return flat, flat[:B * T * ld].view(B, T, ld)


def view(flat, B, T, ld):
    return flat[:B * T * ld].view(B, T, ld)


def tables(S, spacing="logsnr"):
    from inferbiomechanics_amd.diffusion.schedule import DiffusionTables
    tabs = DiffusionTables(torch.device(DEV), num_sample_steps=10)
    tabs.set_sampler(S, 0.0, "dpmpp2m", spacing)
    return tabs


def masks(T, D, ld):
    free = torch.zeros(T, ld, dtype=torch.uint8)
    observed = free.clone()
    observed[:, :D] = 1
    label = observed.clone()
    label[:, D - 30:D] = 0
    checker = free.clone()
    checker[:, :D] = ((torch.arange(T).reshape(-1, 1) + torch.arange(D).reshape(1, -1)) % 2).to(torch.uint8) * 5
    return {"free": free, "observed": observed, "label": label, "checkerboard": checker}


def max_err(got, want, where=None):
    d = (got.cpu().double() - want).abs()
    if where is not None:
        d = d[:, where]
    return float(d.max()) if d.numel() else 0.0


@pytest.mark.parametrize("dt,B,T,D,ld", SHAPES)
def test_every_step_against_float64(dt, B, T, D, ld):
    from inferbiomechanics_amd import hip
    g = torch.Generator().manual_seed(13 * B + D + ld)
    tabs = tables(S6)
    c5 = tabs.dpmpp_coef.cpu().double()
    assert c5.shape == (S6, 5) and float(c5[0, 2]) == 0.0 == float(c5[-1, 2]) and bool((c5[1:-1, 2] != 0).all())
    xf, x = guarded(B, T, ld, D, dt, g)
    _, eps = guarded(B, T, ld, D, dt, g)
    hf, hist = guarded(B, T, ld, D, torch.float32, g, scale=3.0)
    X, E, H = x.cpu().double(), eps.cpu().double(), hist.cpu().double()
    n = B * T * ld
    for s in range(S6):
        ctr = torch.tensor([s], dtype=torch.int32, device=DEV)
        t_out = torch.full((B,), -7, dtype=torch.int64, device=DEV)
        xs_f, hs_f = xf.clone(), hf.clone()
        xs, hs = view(xs_f, B, T, ld), view(hs_f, B, T, ld)
        hip.dpmpp_step(xs, eps, hs, tabs.dpmpp_coef, tabs.ddim_t, step_dev=ctr, t_out=t_out)
        xh, hh = x.clone(), hist.clone()
        hip.dpmpp_step(xh, eps, hh, tabs.dpmpp_coef, tabs.ddim_t, step=s)
        torch.cuda.synchronize()
        A, Ec, C, hx, he = (float(v) for v in c5[s])
        want = A * X + Ec * E + C * H
        want_h = hx * X + he * E
        ex, eh = max_err(xs, want), max_err(hs, want_h)
        tol, tol_h = ARITH[dt] * float(want.abs().max()), HIST * float(want_h.abs().max())
        print(f"dpmpp_step {dt} B={B} D={D} ld={ld} s={s}: state err {ex:.3e} (tol {tol:.3e}), history err {eh:.3e} (tol {tol_h:.3e})")
        assert ex <= tol, (s, ex, tol)
        assert eh <= tol_h, (s, eh, tol_h)
        assert hs.dtype == torch.float32
        assert not xs[:, :, D:].any() and not hs[:, :, D:].any(), "pad columns must stay 0"
        assert bool((xs_f[n:] == 7.0).all()) and bool((hs_f[n:] == 7.0).all()), "wrote past the state or the history"
        assert torch.equal(xh, xs) and torch.equal(hh, hs), "host step index and device step counter disagree"
        assert int(t_out[0]) == (int(tabs.ddim_t[s + 1]) if s + 1 < S6 else 0) and int(ctr) == s
        assert bool((t_out == t_out[0]).all())


@pytest.mark.parametrize("dt,B,T,D,ld", SHAPES)
def test_every_masked_step_against_float64(dt, B, T, D, ld):
    from inferbiomechanics_amd import hip
    g = torch.Generator().manual_seed(29 * B + D + ld)
    tabs = tables(S6)
    c5, oc = tabs.dpmpp_coef.cpu().double(), tabs.obs_coef.cpu().double()
    _, x = guarded(B, T, ld, D, dt, g)
    _, eps = guarded(B, T, ld, D, dt, g)
    _, x0 = guarded(B, T, ld, D, dt, g)
    _, z = guarded(B, T, ld, D, dt, g)
    hf, hist = guarded(B, T, ld, D, torch.float32, g, scale=3.0)
    X, E, X0, Z, H = (t.cpu().double() for t in (x, eps, x0, z, hist))
    n = B * T * ld
    for name, m in masks(T, D, ld).items():
        mb, md = m.bool(), m.to(DEV)
        obs, free = mb.to(DEV), ~mb.to(DEV)
        for s in range(S6):
            ctr = torch.tensor([s], dtype=torch.int32, device=DEV)
            t_out = torch.full((B,), -7, dtype=torch.int64, device=DEV)
            xs, hs_f = x.clone(), hf.clone()
            hs = view(hs_f, B, T, ld)
            hip.dpmpp_cond_step(xs, eps, hs, x0, z, md, tabs.dpmpp_coef, tabs.obs_coef, tabs.ddim_t, step_dev=ctr,
                                t_out=t_out, D=D)
            xd = x.clone()                     # the DDIM entry's pinned value
            hip.ddim_cond_step(xd, eps, x0, z, md, tabs.ddim_coef, tabs.obs_coef, tabs.ddim_t, step=s, D=D)
            xu, hu = x.clone(), hist.clone()   # the unmasked entry
            hip.dpmpp_step(xu, eps, hu, tabs.dpmpp_coef, tabs.ddim_t, step=s)
            torch.cuda.synchronize()
            A, Ec, C, hx, he = (float(v) for v in c5[s])
            want = torch.where(mb, oc[s + 1, 0] * X0 + oc[s + 1, 1] * Z, A * X + Ec * E + C * H)
            want_h = hx * X + he * E
            ex, eh = max_err(xs, want), max_err(hs, want_h, ~mb)
            tol, tol_h = ARITH[dt] * float(want.abs().max()), HIST * float(want_h.abs().max())
            print(f"dpmpp_cond_step {dt} B={B} D={D} ld={ld} {name} s={s}: state err {ex:.3e} (tol {tol:.3e}), "
                  f"history err {eh:.3e} (tol {tol_h:.3e})")
            assert ex <= tol, (name, s, ex, tol)
            assert eh <= tol_h, (name, s, eh, tol_h)
            assert torch.equal(xs[:, obs], xd[:, obs]), (name, s, "observed elements differ from ib_ddim_cond_step")
            assert torch.equal(xs[:, free], xu[:, free]) and torch.equal(hs[:, free], hu[:, free]), \
                (name, s, "free elements differ from ib_dpmpp_step")
            assert not xs[:, :, D:].any() and not hs[:, :, D:].any(), "pad columns must stay 0"
            assert bool(torch.isfinite(hs).all()) and bool((hs_f[n:] == 7.0).all()), "wrote past the history"
            assert int(t_out[0]) == (int(tabs.ddim_t[s + 1]) if s + 1 < S6 else 0)
            if s == S6 - 1:
                assert torch.equal(xs[:, obs], x0[:, obs]), "the last step must land on the observation"


@pytest.mark.parametrize("dt,B,T,D,ld", SHAPES)
def test_rows_without_history_equal_the_ddim_entries_and_never_read_it(dt, B, T, D, ld):
    """the first and last row of a table (C == 0): the history holds NaN, the state is ib_ddim_step / ib_ddim_cond_step given
    (A, E) bit for bit"""
    from inferbiomechanics_amd import hip
    g = torch.Generator().manual_seed(7 * B + D + ld)
    for spacing, S in (("logsnr", S6), ("time", 10)):
        tabs = tables(S, spacing)
        assert torch.equal(tabs.dpmpp_coef[[0, S - 1], :2], tabs.ddim_coef[[0, S - 1]])
        _, x = guarded(B, T, ld, D, dt, g)
        _, eps = guarded(B, T, ld, D, dt, g)
        _, x0 = guarded(B, T, ld, D, dt, g)
        _, z = guarded(B, T, ld, D, dt, g)
        X, E = x.cpu().double(), eps.cpu().double()
        for s in (0, S - 1):
            assert float(tabs.dpmpp_coef[s, 2]) == 0.0
            a, b = x.clone(), x.clone()
            h = torch.full((B, T, ld), float("nan"), dtype=torch.float32, device=DEV)
            hip.ddim_step(a, eps, tabs.ddim_coef, tabs.ddim_t, step=s)
            hip.dpmpp_step(b, eps, h, tabs.dpmpp_coef, tabs.ddim_t, step=s)
            assert torch.equal(a, b) and bool(torch.isfinite(b).all()), ("ib_ddim_step", spacing, s)
            assert bool(torch.isfinite(h).all()), "every row writes the history"
            assert not h[:, :, D:].any(), "every row writes the history's pad columns (x = eps = 0 there)"
            for name, m in masks(T, D, ld).items():
                md = m.to(DEV)
                a, b = x.clone(), x.clone()
                h = torch.full((B, T, ld), float("nan"), dtype=torch.float32, device=DEV)
                hip.ddim_cond_step(a, eps, x0, z, md, tabs.ddim_coef, tabs.obs_coef, tabs.ddim_t, step=s, D=D)
                hip.dpmpp_cond_step(b, eps, h, x0, z, md, tabs.dpmpp_coef, tabs.obs_coef, tabs.ddim_t, step=s, D=D)
                assert torch.equal(a, b) and bool(torch.isfinite(b).all()), ("ib_ddim_cond_step", spacing, name, s)
                want_h = float(tabs.dpmpp_coef[s, 3]) * X + float(tabs.dpmpp_coef[s, 4]) * E
                assert max_err(h, want_h, ~m.bool()) <= HIST * float(want_h.abs().max())
                assert not h[:, :, D:].any(), "pad columns are free: the masked entry writes the history's too"


@pytest.mark.parametrize("dt", [torch.float32, BF])
def test_unaligned_history_takes_the_element_wise_form_with_the_8_wide_rounding(dt):
    """x and eps 16-byte aligned, hist offset by one float: the entries fall back to the element-wise kernel, which rounds
    the update as the 8-wide one (mix8).  Free elements and their history equal the aligned run bit for bit; observed
    elements (the element-wise pinned expression) are held to the float64 bound."""
    from inferbiomechanics_amd import hip
    B, T, D, ld = 3, 24, 44, 48
    n = B * T * ld
    g = torch.Generator().manual_seed(77)
    tabs = tables(S6)
    oc = tabs.obs_coef.cpu().double()
    _, x = guarded(B, T, ld, D, dt, g)
    _, eps = guarded(B, T, ld, D, dt, g)
    _, x0 = guarded(B, T, ld, D, dt, g)
    _, z = guarded(B, T, ld, D, dt, g)
    _, hist = guarded(B, T, ld, D, torch.float32, g, scale=3.0)
    m = masks(T, D, ld)["checkerboard"]
    mb, md = m.bool(), m.to(DEV)
    free = ~mb.to(DEV)
    for s in (0, 2, S6 - 1):
        big = torch.full((n + 65,), 7.0, dtype=torch.float32, device=DEV)
        off = big[1:n + 1].view(B, T, ld)
        assert off.data_ptr() % 16 == 4 and off.is_contiguous()
        off.copy_(hist)
        xa, ha, xo = x.clone(), hist.clone(), x.clone()
        hip.dpmpp_step(xa, eps, ha, tabs.dpmpp_coef, tabs.ddim_t, step=s)
        hip.dpmpp_step(xo, eps, off, tabs.dpmpp_coef, tabs.ddim_t, step=s)
        assert torch.equal(xa, xo) and torch.equal(ha, off), ("ib_dpmpp_step", s)
        assert float(big[0]) == 7.0 and bool((big[n + 1:] == 7.0).all()), "wrote outside the offset history"
        off.copy_(hist)
        xa, ha, xo = x.clone(), hist.clone(), x.clone()
        hip.dpmpp_cond_step(xa, eps, ha, x0, z, md, tabs.dpmpp_coef, tabs.obs_coef, tabs.ddim_t, step=s, D=D)
        hip.dpmpp_cond_step(xo, eps, off, x0, z, md, tabs.dpmpp_coef, tabs.obs_coef, tabs.ddim_t, step=s, D=D)
        assert torch.equal(xa[:, free], xo[:, free]) and torch.equal(ha[:, free], off[:, free]), ("ib_dpmpp_cond_step", s)
        want = oc[s + 1, 0] * x0.cpu().double() + oc[s + 1, 1] * z.cpu().double()
        assert max_err(xo, want, mb) <= ARITH[dt] * float(want.abs().max())
        assert float(big[0]) == 7.0 and bool((big[n + 1:] == 7.0).all()), "wrote outside the offset history"


# ---------------------------------------------------------------------------------------------------------------------
# the closed-form problem through the real kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sd", [0.3, 1.0, 2.0])
def test_closed_form_through_the_kernel(sd):
    """Data x0 ~ N(0, sd^2): eps*(x, t) = sigma_t x / (ab_t sd^2 + 1 - ab_t), exact end state x_T sqrt(sd^2 / (ab_t0 sd^2 + 1
    - ab_t0)).  S = 20 on the log-SNR grid in fp32, eps computed by torch on the device in float64 and cast.  The error
    against the closed form is within 1 % of the float64 loop's own error (1.45e-2; fp32 rounding is about 1e-6)."""
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion import schedule as sch
    S, N = 20, 1000
    tabs = tables(S)
    ab = sch.alphas_cumprod(N)
    ts = sch.sample_timesteps(N, S, "logsnr").tolist()
    c5 = sch.dpmpp_coefficients(N, S, "logsnr")
    gain = [float(torch.sqrt(1 - ab[t]) / (ab[t] * sd * sd + 1 - ab[t])) for t in ts]
    x_T = torch.randn(4, 64, 64, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    exact = x_T * float(torch.sqrt(sd * sd / (ab[ts[0]] * sd * sd + 1 - ab[ts[0]])))
    y, h = x_T.clone(), None
    for i in range(S):
        e = gain[i] * y
        new = c5[i, 0] * y + c5[i, 1] * e + (c5[i, 2] * h if float(c5[i, 2]) != 0.0 else 0.0)
        h, y = c5[i, 3] * y + c5[i, 4] * e, new
    rel = lambda a: float(torch.sqrt(((a - exact) ** 2).mean() / (exact ** 2).mean()))
    err64 = rel(y)
    x = x_T.to(torch.float32).to(DEV)
    hist = torch.full_like(x, float("nan"))
    ctr = torch.zeros(1, dtype=torch.int32, device=DEV)
    t_vec = torch.full((4,), ts[0], dtype=torch.int64, device=DEV)
    for i in range(S):
        assert int(t_vec[0]) == ts[i]
        eps = (x.double() * gain[i]).to(torch.float32)
        hip.dpmpp_step(x, eps, hist, tabs.dpmpp_coef, tabs.ddim_t, step_dev=ctr, t_out=t_vec)
        hip.counter_add(ctr, 1)
    err = rel(x.cpu().double())
    print(f"closed form sd={sd}: float64 loop {err64:.6e}, kernel loop (fp32) {err:.6e}, difference {abs(err - err64) / err64:.3e} of it")
    assert abs(err - err64) <= 0.01 * err64


# ---------------------------------------------------------------------------------------------------------------------
# a captured step replayed
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, BF])
@pytest.mark.parametrize("masked", [False, True])
def test_captured_step_replayed_equals_the_eager_loop(dt, masked):
    """one eager step, then one captured step (capturing runs nothing) replayed S - 1 times, as the samplers do"""
    from inferbiomechanics_amd import hip
    S, B, T, D, ld = 8, 3, 24, 44, 48
    tabs = tables(S)
    g = torch.Generator().manual_seed(41)
    _, x_start = guarded(B, T, ld, D, dt, g)
    _, eps = guarded(B, T, ld, D, dt, g, scale=0.5)
    _, x0 = guarded(B, T, ld, D, dt, g)
    _, z = guarded(B, T, ld, D, dt, g)
    md = masks(T, D, ld)["label"].to(DEV)

    def run(graph):
        x = x_start.clone()
        hist = torch.full((B, T, ld), 3.0, dtype=torch.float32, device=DEV)     # stale values: the first row does not read them
        ctr = torch.zeros(1, dtype=torch.int32, device=DEV)
        t_vec = torch.full((B,), int(tabs.ddim_t[0]), dtype=torch.int64, device=DEV)
        seen = []

        def step():
            if masked:
                hip.dpmpp_cond_step(x, eps, hist, x0, z, md, tabs.dpmpp_coef, tabs.obs_coef, tabs.ddim_t, step_dev=ctr,
                                    t_out=t_vec, D=D)
            else:
                hip.dpmpp_step(x, eps, hist, tabs.dpmpp_coef, tabs.ddim_t, step_dev=ctr, t_out=t_vec)
            hip.counter_add(ctr, 1)

        stream = hip.new_stream(torch.device(DEV))
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            step()
            if graph:
                gr = hip.Graph()
                gr.begin()
                step()
                gr.end()
                for _ in range(S - 1):
                    gr.launch()
            else:
                for _ in range(S - 1):
                    step()
                    seen.append(int(t_vec[0]))
        torch.cuda.current_stream().wait_stream(stream)
        torch.cuda.synchronize()
        return x, hist, ctr, t_vec, seen

    xe, he, ce, te, seen = run(False)
    xg, hg, cg, tg, _ = run(True)
    assert seen == tabs.ddim_t.tolist()[2:] + [0]
    assert int(ce) == int(cg) == S and torch.equal(te, tg)
    assert torch.equal(xe, xg) and bool(torch.isfinite(xg).all())
    assert torch.equal(he, hg)
