"""ib_stitch_ddim_step_noise on the GPU (csrc/stitch_noise.hip).  -m gpu.

Shapes are those of tests/test_stitch_kernels_gpu.py: windows of T = 8 frames every hop = 3 over a trial of F = 17 frames
(W = 4 windows, 1 .. 3 of them cover a frame), N = 2 trials, fp32 and bf16, with and without observations.  Geometries
(D, ld): (12, 16) is 8-wide with whole Philox blocks, the second block of the second vector in the pad; (10, 16) is 8-wide
with D % 4 != 0, blocks looked up per element; (5, 5) is element-wise.  Trial ids {5, 2^32 - 1}, steps 0, S / 2, S - 1.

(a) Against float64: the normals from oracle.ref_cpu.draw_words with float64 Box-Muller indexed by (f D + d) over the TRIAL
    (ref_normals of tests/test_eta_kernels_gpu.py), the blend, the update and the stored-noise rule restated; that file's bound.
(b) After a launch all copies of every element are bitwise equal in x and in z; pads stay 0, sentinels intact, free elements
    leave z untouched.
(c) sigma = 0 rows equal ib_stitch_ddim_step bit for bit and leave z untouched.
(d) One window (F = T): ib_ddim_step_noise / ib_ddim_cond_step_noise with win_id = trial_id, bit for bit; what
    tests/test_stitch_kernels_gpu.py check (a) leaves out of the free elements is left out here, and nothing else.
(e) The draw depends on (seed, trial id, step) only.
(f) The argument refusals.
(g) A whole loop over Gaussian data follows the exact variance recursion and stays uncorrelated across frames and trials."""
import pytest
import torch

from oracle import ref_cpu as R
from tests.test_eta_kernels_gpu import ARITH, GEN_TOL, ref_normals
from tests.test_stitch_kernels_gpu import (F, N, T, checker_mask, guarded, layout, left_out_of_one_window_comparison,
                                           operands, sentinels_ok)

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
S = 10
GEOM = [(12, 16), (10, 16), (5, 5)]
IDS = [5, 2 ** 32 - 1]
SEED = 0x1234_5678_9ABC_DEF0
STEPS = (0, S // 2, S - 1)
CASES = [(dt, D, ld, cond) for dt in (torch.float32, BF) for D, ld in GEOM for cond in (False, True)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from inferbiomechanics_amd import hip
    hip.lib()


_TABS = {}


def tables(eta, steps=S):
    from inferbiomechanics_amd.diffusion.schedule import DiffusionTables
    if (eta, steps) not in _TABS:
        t = DiffusionTables(torch.device(DEV), num_sample_steps=steps)
        t.set_sampler(steps, eta)
        _TABS[(eta, steps)] = t
    return _TABS[(eta, steps)]


def col_mask(D, ld):
    """[T, ld] uint8, the same logical columns in every frame (pad columns are free): ld = 16 has an all-observed vector
    (columns 0 .. 7) and a mixed one (8 and, where it is a logical column, 10 observed); (5, 5) observes columns 0 and 3"""
    m = torch.zeros(T, ld, dtype=torch.uint8)
    m[:, [c for c in (list(range(8)) + [8, 10] if ld == 16 else [0, 3]) if c < D]] = 3
    return m


def run_noise(hip, tabs, lay, op, cond, mask, s, D, ids=IDS, seed=SEED, by_counter=True, coef=None, on=None):
    """one launch on clones of op -> (x, z, t_out, x's flat buffer, z's flat buffer)"""
    W = lay["W"]
    shift = op["x"].storage_offset()
    xf, x = guarded(op["x"].shape, op["x"].dtype, shift)
    zf, z = guarded(op["x"].shape, op["x"].dtype, shift)
    x.copy_(op["x"])
    z.copy_(op["z"])
    ctr = torch.tensor([s], dtype=torch.int32, device=DEV)
    t_out = torch.full((op["x"].shape[0] * W,), -7, dtype=torch.int64, device=DEV)
    coef = tabs.ddim_coef_eta if coef is None else coef
    on = tabs.obs_noise_coef if on is None else on
    c = (op["x0"], z, mask.to(DEV), tabs.obs_coef, on) if cond else (None, None, None, None, None)
    st, cv, wn = lay["dev"]
    kw = dict(step_dev=ctr, t_out=t_out) if by_counter else dict(step=s, t_out=t_out)
    hip.stitch_ddim_step_noise(x, op["eps"], c[0], c[1], c[2], coef, c[3], c[4], tabs.ddim_t, st, cv, wn,
                               torch.tensor(ids, dtype=torch.int64, device=DEV), seed, D=D, **kw)
    torch.cuda.synchronize()
    return x, z, t_out, xf, zf


def first_copies(t, lay):
    """[N, W, T, ld] -> [N, F, ld]: every trial frame from its first covering window"""
    st, cv = lay["start"].tolist(), lay["cover"].tolist()
    return torch.stack([t[:, w0, f - st[w0]] for f, (w0, _) in enumerate(cv)], dim=1)


def trial_normals(frames, D, ld, seed, s, ids):
    Z = torch.zeros(len(ids), frames, ld, dtype=torch.float64)
    for n, i in enumerate(ids):
        Z[n, :, :D] = ref_normals(frames, D, seed, s, int(i))
    return Z


# ---------------------------------------------------------------------------------------------------------------------
# (a) float64, (b) copies, and the host step index against the device counter
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,D,ld,cond", CASES)
def test_overlapping_windows_against_float64_and_copies(dt, D, ld, cond):
    from inferbiomechanics_amd import hip
    tabs = tables(0.7)
    lay = layout(F)
    W = lay["W"]
    st, cv, wn = lay["start"].tolist(), lay["cover"].tolist(), lay["wn"]
    assert W == 4 and sorted({c for _, c in cv}) == [1, 2, 3]
    op = operands(lay, D, ld, dt, 300 + D + (dt == BF))
    mask = col_mask(D, ld) if cond else None
    obs_cols = mask[0].bool() if cond else torch.zeros(ld, dtype=torch.bool)
    fc = ~obs_cols
    Y, X0, Z0 = (op[k + "_trial"].double() for k in ("x", "x0", "z"))
    E = op["eps"].cpu().double()
    Ek = torch.zeros(8, N, F, ld, dtype=torch.float64)
    for f, (w0, c) in enumerate(cv):
        for k in range(c):
            Ek[k, :, f] = E[:, w0 + k, f - st[w0 + k]]
    eb = (wn.double().t()[:, None, :, None] * Ek).sum(0)                # the fp32 weights the kernel reads
    c3, oc, on = (t.cpu().double() for t in (tabs.ddim_coef_eta, tabs.obs_coef, tabs.obs_noise_coef))
    for s in STEPS:
        x, z, t_out, xf, zf = run_noise(hip, tabs, lay, op, cond, mask, s, D)
        x2, z2, _, _, _ = run_noise(hip, tabs, lay, op, cond, mask, s, D, by_counter=False)
        assert torch.equal(x, x2) and torch.equal(z, z2), "host step index and device step counter disagree"
        assert sentinels_ok(xf) and sentinels_ok(zf), "wrote past the state or the noise buffer"
        assert bool((t_out == (int(tabs.ddim_t[s + 1]) if s + 1 < S else 0)).all())
        xc, zc = x.cpu(), z.cpu()
        # (b) every copy holds the bits of the first copy, in x and in z
        first, first_z = first_copies(xc, lay), first_copies(zc, lay)
        assert torch.equal(xc, first[:, lay["gather"]]), (s, "copies of x differ")
        assert torch.equal(zc, first_z[:, lay["gather"]]), (s, "copies of z differ")
        assert not xc[..., D:].any() and not zc[..., D:].any(), "pad columns must stay 0"
        assert torch.equal(zc[..., fc], op["z"].cpu()[..., fc]), "free elements must not touch z"
        # (a) float64
        sg, r, q = float(c3[s, 2]), float(on[s, 0]), float(on[s, 1])
        assert (sg == 0.0) == (s == S - 1)
        Zn = trial_normals(F, D, ld, SEED, s, IDS)
        want = c3[s, 0] * Y + c3[s, 1] * eb + sg * Zn
        if cond:
            if sg == 0.0:
                assert torch.equal(zc, op["z"].cpu()), "a sigma = 0 row leaves z untouched"
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
        tol = abs(sg) * GEN_TOL + ARITH[dt] * float(want.abs().max())
        print(f"stitch_noise {dt} D={D} ld={ld} cond={cond} s={s}: max err {err:.3e} (tol {tol:.3e})")
        assert err <= tol, (s, err, tol)
        if cond and s == S - 1:
            assert torch.equal(first[..., obs_cols], op["x0_trial"][..., obs_cols]), "the last step lands on the observation"


# ---------------------------------------------------------------------------------------------------------------------
# (c) sigma = 0 rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,D,ld,cond", CASES)
def test_sigma_zero_rows_equal_the_deterministic_stitched_update(dt, D, ld, cond):
    """every row of an eta = 0 table and the last row of an eta = 1 table"""
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion import schedule as sch
    tabs = tables(1.0)
    zero3 = sch.ddim_coefficients_eta(1000, S, 0.0).to(torch.float32).to(DEV).contiguous()
    one0 = sch.observation_noise_coefficients(1000, S, 0.0).to(torch.float32).to(DEV).contiguous()
    assert torch.equal(zero3[:, :2], tabs.ddim_coef) and not zero3[:, 2].any()
    assert float(tabs.ddim_coef_eta[S - 1, 2]) == 0.0 and bool((tabs.ddim_coef_eta[:S - 1, 2] != 0).all())
    lay = layout(F)
    op = operands(lay, D, ld, dt, 400 + D + (dt == BF))
    mask = col_mask(D, ld) if cond else None
    st, cv, wn = lay["dev"]
    c = (op["x0"], op["z"], mask.to(DEV), tabs.obs_coef) if cond else (None, None, None, None)
    for coef, on, steps in ((zero3, one0, range(S)), (tabs.ddim_coef_eta, tabs.obs_noise_coef, (S - 1,))):
        for s in steps:
            x, z, _, xf, zf = run_noise(hip, tabs, lay, op, cond, mask, s, D, coef=coef, on=on)
            want = op["x"].clone()
            hip.stitch_ddim_step(want, op["eps"], c[0], c[1], c[2], tabs.ddim_coef, c[3], tabs.ddim_t, st, cv, wn, step=s, D=D)
            assert torch.equal(x, want), (s, "ib_stitch_ddim_step")
            assert torch.equal(z, op["z"]), (s, "z must stay untouched")
            assert sentinels_ok(xf) and sentinels_ok(zf)


# ---------------------------------------------------------------------------------------------------------------------
# (d) one window: the per-window stochastic kernels with win_id = trial_id
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,D,ld,cond,shift", [c + (0,) for c in CASES] + [c + (1,) for c in CASES if c[2] % 8])
def test_one_window_equals_the_per_window_kernels(dt, D, ld, cond, shift):
    from inferbiomechanics_amd import hip
    tabs = tables(0.7)
    lay = layout(T)
    assert lay["W"] == 1
    op = operands(lay, D, ld, dt, 500 + D + (dt == BF), shift)
    win = torch.tensor(IDS, dtype=torch.int64, device=DEV)
    shape3 = (N, T, ld)
    for mask in ((col_mask(D, ld), checker_mask(D, ld)) if cond else (None,)):
        for s in STEPS:
            x, z, t_out, xf, zf = run_noise(hip, tabs, lay, op, cond, mask, s, D)
            _, fx = guarded(shape3, dt, shift)
            _, fz = guarded(shape3, dt, shift)
            fx.copy_(op["x"].view(shape3))
            fz.copy_(op["z"].view(shape3))
            eps, x0 = op["eps"].view(shape3), op["x0"].view(shape3)
            if cond:
                hip.ddim_cond_step_noise(fx, eps, x0, fz, mask.to(DEV), tabs.ddim_coef_eta, tabs.obs_coef, tabs.obs_noise_coef,
                                         tabs.ddim_t, win, SEED, step=s, D=D)
            else:
                hip.ddim_step_noise(fx, eps, tabs.ddim_coef_eta, tabs.ddim_t, win, SEED, step=s, D=D)
            torch.cuda.synchronize()
            x3, z3 = x.view(shape3), z.view(shape3)
            free = torch.ones(T, ld, dtype=torch.bool) if mask is None else ~mask.bool()
            free, obs = free.to(DEV), ~free.to(DEV)
            skip_free, _, _ = left_out_of_one_window_comparison(dt, ld, shift)
            print(f"{dt} D={D} ld={ld} cond={cond} shift={shift} s={s}: {int((x3[:, free] != fx[:, free]).sum())} free elements "
                  f"differ, {int((x3[:, obs] != fx[:, obs]).sum())} observed, {int((z3 != fz).sum())} stored noises")
            if not skip_free:
                assert torch.equal(x3[:, free], fx[:, free]), (s, "free elements")
            # observed elements in every geometry: a sigma != 0 row pins fmaf(ox, x0, oz b') at either width, and the one
            # sigma = 0 row here is the last, whose obs_coef row is (1, 0): every form of ox x0 + oz b returns x0 exactly
            if float(tabs.ddim_coef_eta[s, 2]) == 0.0:
                assert s == S - 1 and tabs.obs_coef[s + 1].tolist() == [1.0, 0.0]
            assert torch.equal(x3[:, obs], fx[:, obs]), (s, "observed elements")
            assert torch.equal(z3, fz), (s, "stored noise")
            assert sentinels_ok(xf) and sentinels_ok(zf)
            assert bool((t_out == (int(tabs.ddim_t[s + 1]) if s + 1 < S else 0)).all())


# ---------------------------------------------------------------------------------------------------------------------
# (e) what the draw depends on
# ---------------------------------------------------------------------------------------------------------------------
def _sub(op, sel):
    """the operands of the trials `sel` of op, in that order"""
    out = {}
    for k in ("x", "x0", "z", "eps"):
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
    op = operands(lay, D, ld, dt, 600 + D)
    mask = col_mask(D, ld) if cond else None

    def run(sel, ids, s=3, seed=SEED):
        x, z, _, _, _ = run_noise(hip, tabs, lay, _sub(op, sel), cond, mask, s, D, ids=ids, seed=seed)
        return x, z

    bx, bz = run([0], [42])
    for sel, ids, at in (([1, 0], [7, 42], 1), ([0, 1, 1], [42, 1, 2], 0), ([1, 1, 0, 1], [9, 8, 42, 7], 2)):
        x, z = run(sel, ids)
        assert torch.equal(x[at], bx[0]) and torch.equal(z[at], bz[0]), "the draw must not depend on N or the batch position"
    for what, (x, z) in (("trial id", run([0], [43])), ("step", run([0], [42], s=4)), ("seed", run([0], [42], seed=SEED + 1))):
        assert not torch.equal(x, bx), f"another {what}, the same draw"
        if cond:
            assert not torch.equal(z, bz), f"another {what}, the same stored noise"


@pytest.mark.parametrize("cond", [False, True])
def test_fp32_pitched_and_unpitched_runs_agree(cond):
    from inferbiomechanics_amd import hip
    tabs = tables(0.7)
    lay = layout(F)
    D = 12
    outs = []
    for ld in (12, 16):
        op = operands(lay, D, ld, torch.float32, 77)                   # the same generator stream: the same logical values
        mask = col_mask(D, 16)[:, :ld].contiguous() if cond else None
        x, z, _, _, _ = run_noise(hip, tabs, lay, op, cond, mask, 2, D)
        outs.append((x[..., :D].clone(), z[..., :D].clone(), op["x"][..., :D].clone()))
    assert torch.equal(outs[0][2], outs[1][2]), "the test's own operands differ between the pitches"
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert not torch.equal(outs[0][0], outs[0][2])


# ---------------------------------------------------------------------------------------------------------------------
# (f) refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_refusals():
    from inferbiomechanics_amd import hip
    tabs = tables(0.7)
    lay = layout(F)
    W, D, ld = lay["W"], 12, 16
    op = operands(lay, D, ld, torch.float32, 7)
    mask = col_mask(D, ld).to(DEV)
    st, cv, wn = lay["dev"]
    ids = torch.tensor(IDS, dtype=torch.int64, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()
    base = dict(x=p(op["x"]), eps=p(op["eps"]), x0=p(op["x0"]), z=p(op["z"]), mask=p(mask), coef=p(tabs.ddim_coef_eta),
                obs_coef=p(tabs.obs_coef), obs_noise_coef=p(tabs.obs_noise_coef), timesteps=p(tabs.ddim_t), num_steps=S, step=0,
                step_dev=None, t_out=None, start=p(st), cover=p(cv), wn=p(wn), trial_id=p(ids), seed=3, N=N, W=W, T=T, F=F, D=D,
                ld=ld, dtype=hip.F32, stream=0)

    def call(**over):
        a = dict(base)
        a.update(over)                                                 # keeps the header's order of the keys
        return hip.lib().ib_stitch_ddim_step_noise(*a.values())

    ARG, DTYPE, UNSUP = -1, -2, -5
    before, before_z = op["x"].clone(), op["z"].clone()
    for name in ("x", "eps", "coef", "start", "cover", "wn", "trial_id"):
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
    assert torch.equal(op["x"], before) and torch.equal(op["z"], before_z), "a refused call must launch nothing"
    assert call() == 0
    torch.cuda.synchronize()
    assert not torch.equal(op["x"], before)
    go = lambda **kw: hip.stitch_ddim_step_noise(op["x"], op["eps"], None, None, None, kw.get("coef", tabs.ddim_coef_eta), None,
                                                 kw.get("on"), tabs.ddim_t, st, cv, wn, kw.get("ids", ids), 3, D=D)
    with pytest.raises(hip.HipError):
        go(coef=tabs.ddim_coef)                                        # [S, 2]
    with pytest.raises(hip.HipError, match="trial_ids"):
        go(ids=torch.zeros(N * W, dtype=torch.int64, device=DEV))
    with pytest.raises(hip.HipError, match="trial_ids"):
        go(ids=ids.cpu())
    with pytest.raises(hip.HipError, match="together"):
        go(on=tabs.obs_noise_coef)


# ---------------------------------------------------------------------------------------------------------------------
# (g) a whole loop over Gaussian data
# ---------------------------------------------------------------------------------------------------------------------
def _levels(steps):
    ab = R.alphas_cumprod(R.linear_beta_schedule(1000))
    return [float(ab[t]) for t in R.ddim_timesteps(1000, steps).tolist()]


@pytest.mark.parametrize("eta", [0.5, 1.0])
@pytest.mark.parametrize("s2", [0.25, 4.0])
def test_loop_variance_follows_the_exact_recursion(eta, s2):
    """As tests/test_eta_kernels_gpu.py: x0 ~ N(0, s2) has the analytic optimal denoiser eps = gain x, elementwise, so every
    copy of a trial element gets the same prediction, their blend (a convex combination) is that prediction, and every trial
    element stays a zero-mean Gaussian with v' = (c_x + c_eps gain)^2 v + sigma^2 from v = 1 -- if the step noise is one
    fresh unit normal per TRIAL element and step.  The M = 2^20 trial elements: relative standard error of the sample
    variance sqrt(2 / M), bound 5 of them.  Independent elements: the sample correlation of n pairs has standard error
    1 / sqrt(n), bound 5 of them; n = (F - 1) N D = 2^20 - 2^14 pairs of consecutive frames (a noise keyed by in-window
    frame, or shared between the windows' first frames, correlates them across the boundaries at f = 16, 32), and
    n = (N - 1) F D = 2^20 - 2^14 pairs of consecutive trials (a noise that ignores the trial id correlates them fully)."""
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion import schedule as sch
    from inferbiomechanics_amd.diffusion.schedule import stitch_layout
    Nn, Tt, hop, Ff, D, steps = 64, 32, 16, 64, 256, 100
    M = Nn * Ff * D
    assert M == 1 << 20
    n_frames, n_trials = (Ff - 1) * Nn * D, (Nn - 1) * Ff * D
    assert n_frames == n_trials == (1 << 20) - (1 << 14)
    tabs = tables(eta, steps)
    c64 = sch.ddim_coefficients_eta(1000, steps, eta)
    lv = _levels(steps)
    v, gains = 1.0, []
    for s in range(steps):
        k = (1 - lv[s]) ** 0.5 / (lv[s] * s2 + 1 - lv[s])
        gains.append(k)
        v = (float(c64[s, 0]) + float(c64[s, 1]) * k) ** 2 * v + float(c64[s, 2]) ** 2
    start, cover, wn, _ = stitch_layout(Ff, Tt, hop, "ramp")
    W = start.numel()
    assert W == 3 and sorted(set(cover[:, 1].tolist())) == [1, 2]
    gather = (start.long()[:, None] + torch.arange(Tt)[None, :]).to(DEV)
    trial = torch.randn(Nn, Ff, D, generator=torch.Generator(device=DEV).manual_seed(int(10 * eta + s2)), device=DEV)
    x = trial[:, gather].contiguous()                                  # [N, W, T, D], consistent copies
    st, cv, wd = start.to(DEV), cover.to(DEV), wn.to(DEV)
    ids = torch.arange(1000, 1000 + Nn, dtype=torch.int64, device=DEV)
    ctr = torch.zeros(1, dtype=torch.int32, device=DEV)
    for s in range(steps):
        eps = x * gains[s]                                             # the test's own denoiser, on the window batch
        hip.stitch_ddim_step_noise(x, eps, None, None, None, tabs.ddim_coef_eta, None, None, tabs.ddim_t, st, cv, wd, ids, 77,
                                   step_dev=ctr)
        hip.counter_add(ctr, 1)
    w0 = cover[:, 0].long()
    t0 = torch.arange(Ff) - start.long()[w0]
    out = x[:, w0.to(DEV), t0.to(DEV)]                                 # [N, F, D] from the first copies
    assert torch.equal(x, out[:, gather]), "the copies came apart"
    got = out.double()
    var = float((got ** 2).mean())
    rel = var / v - 1
    corr = lambda a, b: float((a * b).mean() / ((a ** 2).mean() * (b ** 2).mean()).sqrt())
    cf, ct = corr(got[:, :-1], got[:, 1:]), corr(got[:-1], got[1:])
    print(f"eta={eta} s2={s2}: expected variance {v:.6f}, sample {var:.6f}, rel {rel:+.3e} (bound {5 * (2 / M) ** 0.5:.3e}); "
          f"correlation of consecutive frames {cf:+.3e}, of consecutive trials {ct:+.3e} (bound {5 / n_frames ** 0.5:.3e})")
    assert abs(rel) <= 5 * (2 / M) ** 0.5
    assert abs(float(got.mean())) <= 5 * (v / M) ** 0.5
    assert abs(cf) <= 5 / n_frames ** 0.5
    assert abs(ct) <= 5 / n_trials ** 0.5
