"""ib_sde_dpmpp_step on the GPU (csrc/sde.hip).  -m gpu.

Shapes are those of tests/test_stitch_noise_kernels_gpu.py: windows of T = 8 frames every hop = 3 over a trial of F = 17 frames
(W = 4 windows, 1 .. 3 of them cover a frame), N = 2 trials, fp32 and bf16, with and without observations, the geometries
(D, ld) = (12, 16) (8-wide, whole Philox blocks), (10, 16) (8-wide, blocks looked up per element) and (5, 5) (element-wise),
S = 10 steps on the log-SNR grid at eta = 0.7: row 0 has C = 0 and G != 0, row 5 C != 0 and G != 0, row 9 C = 0 = G.

(a) Against float64: normals, blend, update, history and stored-noise rule restated; the bound of that file,
    |G| GEN_TOL + ARITH[dt] max |want|, for x, for the stored noise (with q for G) and for the history at free elements.
(b) After a launch all copies of every element are bitwise equal in x, z and hist; pads stay 0, sentinels intact, the host
    step index and the device counter agree, t_out is the next timestep.
(c) Bit for bit: a table with G = 0 in every row is ib_stitch_dpmpp_step; a table with C = 0 in every row is
    ib_stitch_ddim_step_noise in x and z; with one window the same against the four per-window kernels, with the exclusions of
    left_out_of_one_window_comparison and nothing else.
(d) The draw depends on (seed, trial id, step) only.
(e) The C-ABI's refusals.
(f) Whole loops on Gaussian data follow the exact covariance recursion of (x, h) over the fp32 table."""
import pytest
import torch

from tests import sde_restatement as RS
from tests.test_eta_kernels_gpu import ARITH, GEN_TOL
from tests.test_stitch_kernels_gpu import (F, N, T, checker_mask, guarded, layout, left_out_of_one_window_comparison,
                                           operands, sentinels_ok)
from tests.test_stitch_noise_kernels_gpu import IDS, SEED, col_mask, first_copies, trial_normals

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
S = 10
ETA = 0.7
GEOM = [(12, 16), (10, 16), (5, 5)]
STEPS = (0, S // 2, S - 1)
CASES = [(dt, D, ld, cond) for dt in (torch.float32, BF) for D, ld in GEOM for cond in (False, True)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from inferbiomechanics_amd import hip
    hip.lib()


_TABS = {}


def tables(eta=ETA, steps=S, solver="dpmpp2m_sde", spacing="logsnr"):
    from inferbiomechanics_amd.diffusion.schedule import DiffusionTables
    key = (eta, steps, solver, spacing)
    if key not in _TABS:
        t = DiffusionTables(torch.device(DEV), num_sample_steps=10)
        t.set_sampler(steps, eta, solver, spacing)
        _TABS[key] = t
    return _TABS[key]


def run_sde(hip, tabs, lay, op, cond, mask, s, D, ids=IDS, seed=SEED, by_counter=True, coef=None, on=None):
    """one launch on clones of op -> (x, hist, z, t_out, and the three flat buffers)"""
    W = lay["W"]
    shift = op["x"].storage_offset()
    xf, x = guarded(op["x"].shape, op["x"].dtype, shift)
    zf, z = guarded(op["x"].shape, op["x"].dtype, shift)
    hf, h = guarded(op["x"].shape, torch.float32, shift)
    x.copy_(op["x"])
    z.copy_(op["z"])
    h.copy_(op["hist"])
    ctr = torch.tensor([s], dtype=torch.int32, device=DEV)
    t_out = torch.full((op["x"].shape[0] * W,), -7, dtype=torch.int64, device=DEV)
    coef = tabs.sde_coef if coef is None else coef
    on = tabs.sde_obs_noise_coef if on is None else on
    c = (op["x0"], z, mask.to(DEV), tabs.obs_coef, on) if cond else (None, None, None, None, None)
    st, cv, wn = lay["dev"]
    kw = dict(step_dev=ctr, t_out=t_out) if by_counter else dict(step=s, t_out=t_out)
    hip.sde_dpmpp_step(x, op["eps"], h, c[0], c[1], c[2], coef, c[3], c[4], tabs.ddim_t, st, cv, wn,
                       torch.tensor(ids, dtype=torch.int64, device=DEV), seed, D=D, **kw)
    torch.cuda.synchronize()
    return x, h, z, t_out, (xf, hf, zf)


# ---------------------------------------------------------------------------------------------------------------------
# (a) float64, (b) copies, and the host step index against the device counter
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,D,ld,cond", CASES)
def test_overlapping_windows_against_float64_and_copies(dt, D, ld, cond):
    from inferbiomechanics_amd import hip
    tabs = tables()
    lay = layout(F)
    W = lay["W"]
    st, cv, wn = lay["start"].tolist(), lay["cover"].tolist(), lay["wn"]
    assert W == 4 and sorted({c for _, c in cv}) == [1, 2, 3]
    op = operands(lay, D, ld, dt, 700 + D + (dt == BF))
    mask = col_mask(D, ld) if cond else None
    obs_cols = mask[0].bool() if cond else torch.zeros(ld, dtype=torch.bool)
    fc = ~obs_cols
    Y, H, X0, Z0 = (op[k + "_trial"].double() for k in ("x", "hist", "x0", "z"))
    E = op["eps"].cpu().double()
    Ek = torch.zeros(8, N, F, ld, dtype=torch.float64)
    for f, (w0, c) in enumerate(cv):
        for k in range(c):
            Ek[k, :, f] = E[:, w0 + k, f - st[w0 + k]]
    eb = (wn.double().t()[:, None, :, None] * Ek).sum(0)                # the fp32 weights the kernel reads
    c6, oc, on = (t.cpu().double() for t in (tabs.sde_coef, tabs.obs_coef, tabs.sde_obs_noise_coef))
    assert [float(c6[s, 2]) != 0 for s in STEPS] == [False, True, False], "rows with C = 0, C != 0 and the last"
    assert [float(c6[s, 5]) != 0 for s in STEPS] == [True, True, False], "rows with G != 0 and the last"
    for s in STEPS:
        x, h, z, t_out, flats = run_sde(hip, tabs, lay, op, cond, mask, s, D)
        x2, h2, z2, _, _ = run_sde(hip, tabs, lay, op, cond, mask, s, D, by_counter=False)
        assert torch.equal(x, x2) and torch.equal(z, z2) and torch.equal(h, h2), "host step index and device counter disagree"
        assert all(sentinels_ok(f) for f in flats), "wrote past the state, the history or the noise buffer"
        assert bool((t_out == (int(tabs.ddim_t[s + 1]) if s + 1 < S else 0)).all())
        xc, hc, zc = x.cpu(), h.cpu(), z.cpu()
        # (b) every copy holds the bits of the first copy
        first, first_h, first_z = first_copies(xc, lay), first_copies(hc, lay), first_copies(zc, lay)
        assert torch.equal(xc, first[:, lay["gather"]]), (s, "copies of x differ")
        assert torch.equal(hc, first_h[:, lay["gather"]]), (s, "copies of hist differ")
        assert torch.equal(zc, first_z[:, lay["gather"]]), (s, "copies of z differ")
        assert not xc[..., D:].any() and not zc[..., D:].any() and not hc[..., D:].any(), "pad columns must stay 0"
        assert torch.equal(zc[..., fc], op["z"].cpu()[..., fc]), "free elements must not touch z"
        # (a) float64
        A, Ec, C, hx, he, G = (float(v) for v in c6[s])
        r, q = float(on[s, 0]), float(on[s, 1])
        Zn = trial_normals(F, D, ld, SEED, s, IDS)
        want = A * Y + Ec * eb + C * H + G * Zn
        want_h = hx * Y + he * eb
        if cond:
            if G == 0.0:
                assert torch.equal(zc, op["z"].cpu()), "a G = 0 row leaves z untouched"
                e_new = Z0
            else:
                e_want = r * Z0 + q * Zn
                got_e = first_z.double()
                tol_e = abs(q) * GEN_TOL + ARITH[dt] * float(e_want.abs().max())
                err_e = float((got_e - e_want)[..., obs_cols].abs().max())
                print(f"    stored noise: max err {err_e:.3e} (tol {tol_e:.3e})")
                assert err_e <= tol_e, (s, err_e, tol_e)
                e_new = got_e                                          # the pinned value is formed from the STORED noise
            pin = oc[s + 1, 0] * X0 + oc[s + 1, 1] * e_new
            want = torch.where(obs_cols[None, None, :], pin, want)
        err = float((first.double() - want).abs().max())
        tol = abs(G) * GEN_TOL + ARITH[dt] * float(want.abs().max())
        err_h = float((first_h.double() - want_h)[..., fc].abs().max())
        tol_h = abs(G) * GEN_TOL + ARITH[dt] * float(want_h[..., fc].abs().max())
        print(f"sde {dt} D={D} ld={ld} cond={cond} s={s}: x max err {err:.3e} (tol {tol:.3e}), hist max err {err_h:.3e} "
              f"(tol {tol_h:.3e})")
        assert err <= tol, (s, err, tol)
        assert err_h <= tol_h, (s, err_h, tol_h)
        if cond and s == S - 1:
            assert torch.equal(first[..., obs_cols], op["x0_trial"][..., obs_cols]), "the last step lands on the observation"


# ---------------------------------------------------------------------------------------------------------------------
# (c) bit-for-bit equalities
# ---------------------------------------------------------------------------------------------------------------------
def g_zero_table():
    """(tables of 'dpmpp2m', their rows with a G = 0 column)"""
    tabs = tables(0.0, S, "dpmpp2m")
    six = torch.cat([tabs.dpmpp_coef, torch.zeros(S, 1, device=DEV)], dim=1).contiguous()
    assert bool((six[1:-1, 2] != 0).all()) and float(six[0, 2]) == 0.0 == float(six[-1, 2])
    return tabs, six


def c_zero_table():
    """(tables of the first-order eta loop, their fp32 (cx, ce, sigma) as rows (cx, ce, 0, hx, he, sigma)); the (r, q) of that
    loop go with it"""
    tabs = tables(ETA, S, "ddim")
    c3 = tabs.ddim_coef_eta
    six = torch.zeros(S, 6, device=DEV)
    six[:, 0], six[:, 1], six[:, 5] = c3[:, 0], c3[:, 1], c3[:, 2]
    six[:, 3], six[:, 4] = 1.5, -0.5                                    # any history: a C = 0 table never reads it
    assert float(c3[-1, 2]) == 0.0 and bool((c3[:-1, 2] != 0).all())
    return tabs, six.contiguous()


@pytest.mark.parametrize("dt,D,ld,cond", CASES)
def test_g_zero_table_is_the_stitched_dpmpp_update(dt, D, ld, cond):
    from inferbiomechanics_amd import hip
    tabs, six = g_zero_table()
    lay = layout(F)
    op = operands(lay, D, ld, dt, 800 + D + (dt == BF))
    mask = col_mask(D, ld) if cond else None
    st, cv, wn = lay["dev"]
    c = (op["x0"], op["z"], mask.to(DEV), tabs.obs_coef) if cond else (None, None, None, None)
    on = torch.full((S, 2), 0.25, device=DEV)                           # never read by a G = 0 row
    for s in range(S):
        x, h, z, _, flats = run_sde(hip, tabs, lay, op, cond, mask, s, D, coef=six, on=on)
        want, want_h = op["x"].clone(), op["hist"].clone()
        hip.stitch_dpmpp_step(want, op["eps"], want_h, c[0], c[1], c[2], tabs.dpmpp_coef, c[3], tabs.ddim_t, st, cv, wn,
                              step=s, D=D)
        torch.cuda.synchronize()
        assert torch.equal(x, want), (s, "x")
        assert torch.equal(h, want_h), (s, "hist")
        assert torch.equal(z, op["z"]), (s, "z must stay untouched")
        assert all(sentinels_ok(f) for f in flats)


@pytest.mark.parametrize("dt,D,ld,cond", CASES)
def test_c_zero_table_is_the_stitched_noise_update(dt, D, ld, cond):
    from inferbiomechanics_amd import hip
    tabs, six = c_zero_table()
    lay = layout(F)
    op = operands(lay, D, ld, dt, 900 + D + (dt == BF))
    mask = col_mask(D, ld) if cond else None
    st, cv, wn = lay["dev"]
    ids = torch.tensor(IDS, dtype=torch.int64, device=DEV)
    for s in range(S):
        x, _, z, _, flats = run_sde(hip, tabs, lay, op, cond, mask, s, D, coef=six, on=tabs.obs_noise_coef)
        want, want_z = op["x"].clone(), op["z"].clone()
        c = (op["x0"], want_z, mask.to(DEV), tabs.obs_coef, tabs.obs_noise_coef) if cond else (None, None, None, None, None)
        hip.stitch_ddim_step_noise(want, op["eps"], c[0], c[1], c[2], tabs.ddim_coef_eta, c[3], c[4], tabs.ddim_t, st, cv, wn,
                                   ids, SEED, step=s, D=D)
        torch.cuda.synchronize()
        assert torch.equal(x, want), (s, "x")
        assert torch.equal(z, want_z), (s, "z")
        assert all(sentinels_ok(f) for f in flats)


@pytest.mark.parametrize("dt,D,ld,cond,shift", [c + (0,) for c in CASES] + [c + (1,) for c in CASES if c[2] % 8])
def test_one_window_equals_the_per_window_kernels(dt, D, ld, cond, shift):
    from inferbiomechanics_amd import hip
    lay = layout(T)
    assert lay["W"] == 1
    op = operands(lay, D, ld, dt, 1000 + D + (dt == BF), shift)
    win = torch.tensor(IDS, dtype=torch.int64, device=DEV)
    shape3 = (N, T, ld)
    skip_free, skip_obs, skip_obs_hist = left_out_of_one_window_comparison(dt, ld, shift)
    dtabs, dsix = g_zero_table()
    ntabs, nsix = c_zero_table()
    for mask in ((col_mask(D, ld), checker_mask(D, ld)) if cond else (None,)):
        free = torch.ones(T, ld, dtype=torch.bool) if mask is None else ~mask.bool()
        free, obs = free.to(DEV), ~free.to(DEV)
        for s in (0, 2, S - 1):
            flat = {}
            for k, dtype in (("x", dt), ("z", dt), ("hist", torch.float32)):
                _, flat[k] = guarded(shape3, dtype, shift)
            eps, x0 = op["eps"].view(shape3), op["x0"].view(shape3)

            def reset():
                for k in flat:
                    flat[k].copy_(op[k].view(shape3))

            # G = 0: ib_dpmpp_step / ib_dpmpp_cond_step, history included
            x, h, z, t_out, flats = run_sde(hip, dtabs, lay, op, cond, mask, s, D, coef=dsix,
                                            on=torch.full((S, 2), 0.25, device=DEV))
            reset()
            if cond:
                hip.dpmpp_cond_step(flat["x"], eps, flat["hist"], x0, flat["z"], mask.to(DEV), dtabs.dpmpp_coef, dtabs.obs_coef,
                                    dtabs.ddim_t, step=s, D=D)
            else:
                hip.dpmpp_step(flat["x"], eps, flat["hist"], dtabs.dpmpp_coef, dtabs.ddim_t, step=s)
            torch.cuda.synchronize()
            x3, h3 = x.view(shape3), h.view(shape3)
            if not skip_free:
                assert torch.equal(x3[:, free], flat["x"][:, free]), (s, "dpmpp: free elements")
            if not skip_obs:
                assert torch.equal(x3[:, obs], flat["x"][:, obs]), (s, "dpmpp: observed elements")
            assert torch.equal(h3[:, free], flat["hist"][:, free]), (s, "dpmpp: history")
            if not skip_obs_hist:
                assert torch.equal(h3, flat["hist"]), (s, "dpmpp: history at observed elements")
            assert torch.equal(z, op["z"]) and all(sentinels_ok(f) for f in flats)
            assert bool((t_out == (int(dtabs.ddim_t[s + 1]) if s + 1 < S else 0)).all())
            # C = 0: ib_ddim_step_noise / ib_ddim_cond_step_noise with win_id = trial_id, x and z
            x, _, z, t_out, flats = run_sde(hip, ntabs, lay, op, cond, mask, s, D, coef=nsix, on=ntabs.obs_noise_coef)
            reset()
            if cond:
                hip.ddim_cond_step_noise(flat["x"], eps, x0, flat["z"], mask.to(DEV), ntabs.ddim_coef_eta, ntabs.obs_coef,
                                         ntabs.obs_noise_coef, ntabs.ddim_t, win, SEED, step=s, D=D)
            else:
                hip.ddim_step_noise(flat["x"], eps, ntabs.ddim_coef_eta, ntabs.ddim_t, win, SEED, step=s, D=D)
            torch.cuda.synchronize()
            x3, z3 = x.view(shape3), z.view(shape3)
            if not skip_free:
                assert torch.equal(x3[:, free], flat["x"][:, free]), (s, "noise: free elements")
            # observed elements in every geometry, as tests/test_stitch_noise_kernels_gpu.py check (d) argues: a sigma != 0
            # row pins fmaf(ox, x0, oz b') at either width, the one sigma = 0 row is the last, whose obs_coef row is (1, 0)
            if float(ntabs.ddim_coef_eta[s, 2]) == 0.0:
                assert s == S - 1 and ntabs.obs_coef[s + 1].tolist() == [1.0, 0.0]
            assert torch.equal(x3[:, obs], flat["x"][:, obs]), (s, "noise: observed elements")
            assert torch.equal(z3, flat["z"]), (s, "noise: stored noise")
            assert all(sentinels_ok(f) for f in flats)


# ---------------------------------------------------------------------------------------------------------------------
# (d) what the draw depends on
# ---------------------------------------------------------------------------------------------------------------------
def _sub(op, sel):
    out = {}
    for k in ("x", "x0", "z", "eps", "hist"):
        _, v = guarded((len(sel),) + tuple(op[k].shape[1:]), op[k].dtype)
        v.copy_(op[k][sel])
        out[k] = v
    return out


@pytest.mark.parametrize("dt,D,ld", [(torch.float32, 12, 16), (BF, 10, 16), (BF, 5, 5)])
@pytest.mark.parametrize("cond", [False, True])
def test_draw_depends_on_seed_trial_id_and_step_only(dt, D, ld, cond):
    from inferbiomechanics_amd import hip
    tabs = tables(1.0)
    lay = layout(F)
    op = operands(lay, D, ld, dt, 1100 + D)
    mask = col_mask(D, ld) if cond else None

    def run(sel, ids, s=3, seed=SEED):
        x, h, z, _, _ = run_sde(hip, tabs, lay, _sub(op, sel), cond, mask, s, D, ids=ids, seed=seed)
        return x, h, z

    bx, bh, bz = run([0], [42])
    for sel, ids, at in (([1, 0], [7, 42], 1), ([0, 1, 1], [42, 1, 2], 0), ([1, 1, 0, 1], [9, 8, 42, 7], 2)):
        x, h, z = run(sel, ids)
        assert torch.equal(x[at], bx[0]) and torch.equal(z[at], bz[0]) and torch.equal(h[at], bh[0]), \
            "the draw must not depend on N or the batch position"
    # another step reads another row of the table too; at eta = 1 its (r, q) and G differ as well: the draws must differ
    for what, (x, h, z) in (("trial id", run([0], [43])), ("step", run([0], [42], s=4)), ("seed", run([0], [42], seed=SEED + 1))):
        assert not torch.equal(x, bx), f"another {what}, the same draw"
        if cond:
            assert not torch.equal(z, bz), f"another {what}, the same stored noise"
        if what != "step":
            assert torch.equal(h, bh), "the history holds no noise of this step"


# ---------------------------------------------------------------------------------------------------------------------
# (e) refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_refusals():
    from inferbiomechanics_amd import hip
    tabs = tables()
    lay = layout(F)
    W, D, ld = lay["W"], 12, 16
    op = operands(lay, D, ld, torch.float32, 7)
    mask = col_mask(D, ld).to(DEV)
    st, cv, wn = lay["dev"]
    ids = torch.tensor(IDS, dtype=torch.int64, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()
    base = dict(x=p(op["x"]), eps=p(op["eps"]), hist=p(op["hist"]), x0=p(op["x0"]), z=p(op["z"]), mask=p(mask),
                coef=p(tabs.sde_coef), obs_coef=p(tabs.obs_coef), obs_noise_coef=p(tabs.sde_obs_noise_coef),
                timesteps=p(tabs.ddim_t), num_steps=S, step=0, step_dev=None, t_out=None, start=p(st), cover=p(cv), wn=p(wn),
                trial_id=p(ids), seed=3, N=N, W=W, T=T, F=F, D=D, ld=ld, dtype=hip.F32, stream=0)
    assert len(base) == 27

    def call(**over):
        a = dict(base)
        a.update(over)                                                 # keeps the header's order of the keys
        return hip.lib().ib_sde_dpmpp_step(*a.values())

    ARG, DTYPE, UNSUP = -1, -2, -5
    before = {k: op[k].clone() for k in ("x", "z", "hist")}
    for name in ("x", "eps", "hist", "coef", "start", "cover", "wn", "trial_id"):
        assert call(**{name: None}) == ARG, name
    five = ("x0", "z", "mask", "obs_coef", "obs_noise_coef")
    for name in five:                                                  # any mix of NULL and non-NULL
        assert call(**{name: None}) == ARG, name
        assert call(**{k: None for k in five if k != name}) == ARG, name
    for name in ("N", "W", "T", "F", "D", "num_steps"):
        assert call(**{name: 0}) == ARG, name
    assert call(ld=D - 1) == ARG
    assert call(F=T - 1) == ARG
    assert call(t_out=p(torch.zeros(N * W, dtype=torch.int64, device=DEV)), timesteps=None) == ARG
    assert call(dtype=7) == DTYPE
    assert call(T=1 << 20, F=1 << 20, ld=1 << 11, D=1 << 11) == UNSUP  # T * ld = 2^31
    assert call(T=8, F=1 << 20, ld=1 << 11, D=1 << 11) == UNSUP        # F * D = 2^31: the block index is one 32-bit word
    torch.cuda.synchronize()
    assert all(torch.equal(op[k], v) for k, v in before.items()), "a refused call must launch nothing"
    assert call() == 0
    assert call(**{k: None for k in five}) == 0                        # the unconditional loop
    torch.cuda.synchronize()
    assert not torch.equal(op["x"], before["x"])
    go = lambda **kw: hip.sde_dpmpp_step(op["x"], op["eps"], kw.get("hist", op["hist"]), None, None, None,
                                         kw.get("coef", tabs.sde_coef), None, kw.get("on"), tabs.ddim_t, st, cv, wn,
                                         kw.get("ids", ids), 3, D=D)
    with pytest.raises(hip.HipError, match="coef"):
        go(coef=tables(0.0, S, "dpmpp2m").dpmpp_coef)                  # [S, 5]
    with pytest.raises(hip.HipError, match="hist"):
        go(hist=op["hist"].to(BF))
    with pytest.raises(hip.HipError, match="trial_ids"):
        go(ids=torch.zeros(N * W, dtype=torch.int64, device=DEV))
    with pytest.raises(hip.HipError, match="trial_ids"):
        go(ids=ids.cpu())
    with pytest.raises(hip.HipError, match="together"):
        go(on=tabs.sde_obs_noise_coef)


# ---------------------------------------------------------------------------------------------------------------------
# (f) whole loops over Gaussian data
# ---------------------------------------------------------------------------------------------------------------------
LOOP_S = 20


def _expected_variance(tabs, s2):
    """the float64 covariance recursion of (x, h) over the fp32 table the kernel reads, and the analytic gains"""
    from inferbiomechanics_amd.diffusion import schedule as sch
    ab = RS.alpha_bars()
    ts = sch.sample_timesteps(1000, LOOP_S, "logsnr").tolist()
    assert ts == tabs.ddim_t.tolist()
    ks = RS.gains(ab, ts, s2)
    return RS.final_variance(tabs.sde_coef.cpu().double().tolist(), ks), ks


@pytest.mark.parametrize("eta", [0.5, 1.0])
@pytest.mark.parametrize("s2", [0.25, 4.0])
def test_flat_loop_variance_follows_the_exact_recursion(eta, s2):
    """The bound and reasoning of tests/test_stitch_noise_kernels_gpu.py::test_loop_variance_follows_the_exact_recursion, for
    the flat form (W = 1, every window a trial of its own): x0 ~ N(0, s2) has the analytic optimal denoiser eps = k x,
    elementwise, so every element stays a zero-mean Gaussian and (x, h) follows the linear recursion
    x' = (A + E k) x + C h + G z', h' = (hx + he k) x exactly -- if z' is one fresh unit normal per element and step and the
    history is the previous step's.  M = 2^22 independent elements: relative standard error of the sample variance
    sqrt(2 / M), bound 5 of them (3.5e-3).  A missing, mis-scaled or repeated noise term or a wrong history moves the variance
    by percents (G^2 sums to most of the final variance; C h carries the second-order correction, 5 .. 9 % here)."""
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion.schedule import stitch_layout
    B, Tt, D = 128, 32, 1024
    M = B * Tt * D
    assert M == 1 << 22
    tabs = tables(eta, LOOP_S)
    v, ks = _expected_variance(tabs, s2)
    st, cv, wn = (t.to(DEV) for t in stitch_layout(Tt, Tt, Tt)[:3])
    x = torch.randn(B, 1, Tt, D, generator=torch.Generator(device=DEV).manual_seed(int(10 * eta + s2)), device=DEV)
    hist = torch.full_like(x, 1e3)                                      # the first row has C = 0: it must not be read
    ids = torch.arange(500, 500 + B, dtype=torch.int64, device=DEV)
    ctr = torch.zeros(1, dtype=torch.int32, device=DEV)
    for s in range(LOOP_S):
        eps = x * ks[s]                                                # the test's own denoiser
        hip.sde_dpmpp_step(x, eps, hist, None, None, None, tabs.sde_coef, None, None, tabs.ddim_t, st, cv, wn, ids, 77,
                           step_dev=ctr)
        hip.counter_add(ctr, 1)
    got = x.double()
    var = float((got ** 2).mean())
    rel = var / v - 1
    print(f"flat eta={eta} s2={s2}: expected variance {v:.6f} ({v / s2:.5f} s2), sample {var:.6f}, rel {rel:+.3e} "
          f"(bound {5 * (2 / M) ** 0.5:.3e})")
    assert abs(rel) <= 5 * (2 / M) ** 0.5
    assert abs(float(got.mean())) <= 5 * (v / M) ** 0.5


def test_stitched_loop_variance_and_independence():
    """one stitched loop at the shapes and by the criteria of check (g) of tests/test_stitch_noise_kernels_gpu.py: M = 2^20
    trial elements, variance within 5 sqrt(2 / M) of the recursion, sample correlation of consecutive frames and of
    consecutive trials within 5 / sqrt(n) (n = 2^20 - 2^14 pairs each)"""
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion.schedule import stitch_layout
    eta, s2 = 1.0, 0.25
    Nn, Tt, hop, Ff, D = 64, 32, 16, 64, 256
    M = Nn * Ff * D
    assert M == 1 << 20
    n_frames, n_trials = (Ff - 1) * Nn * D, (Nn - 1) * Ff * D
    tabs = tables(eta, LOOP_S)
    v, ks = _expected_variance(tabs, s2)
    start, cover, wn, _ = stitch_layout(Ff, Tt, hop, "ramp")
    assert start.numel() == 3 and sorted(set(cover[:, 1].tolist())) == [1, 2]
    gather = (start.long()[:, None] + torch.arange(Tt)[None, :]).to(DEV)
    trial = torch.randn(Nn, Ff, D, generator=torch.Generator(device=DEV).manual_seed(41), device=DEV)
    x = trial[:, gather].contiguous()                                  # [N, W, T, D], consistent copies
    hist = torch.zeros_like(x)
    st, cv, wd = start.to(DEV), cover.to(DEV), wn.to(DEV)
    ids = torch.arange(1000, 1000 + Nn, dtype=torch.int64, device=DEV)
    ctr = torch.zeros(1, dtype=torch.int32, device=DEV)
    for s in range(LOOP_S):
        eps = x * ks[s]
        hip.sde_dpmpp_step(x, eps, hist, None, None, None, tabs.sde_coef, None, None, tabs.ddim_t, st, cv, wd, ids, 77,
                           step_dev=ctr)
        hip.counter_add(ctr, 1)
    w0 = cover[:, 0].long()
    t0 = torch.arange(Ff) - start.long()[w0]
    out = x[:, w0.to(DEV), t0.to(DEV)]                                 # [N, F, D] from the first copies
    assert torch.equal(x, out[:, gather]), "the copies of x came apart"
    assert torch.equal(hist, hist[:, w0.to(DEV), t0.to(DEV)][:, gather]), "the copies of hist came apart"
    got = out.double()
    var = float((got ** 2).mean())
    rel = var / v - 1
    corr = lambda a, b: float((a * b).mean() / ((a ** 2).mean() * (b ** 2).mean()).sqrt())
    cf, ct = corr(got[:, :-1], got[:, 1:]), corr(got[:-1], got[1:])
    print(f"stitched: expected variance {v:.6f}, sample {var:.6f}, rel {rel:+.3e} (bound {5 * (2 / M) ** 0.5:.3e}); correlation "
          f"of consecutive frames {cf:+.3e}, of consecutive trials {ct:+.3e} (bound {5 / n_frames ** 0.5:.3e})")
    assert abs(rel) <= 5 * (2 / M) ** 0.5
    assert abs(float(got.mean())) <= 5 * (v / M) ** 0.5
    assert abs(cf) <= 5 / n_frames ** 0.5
    assert abs(ct) <= 5 / n_trials ** 0.5
