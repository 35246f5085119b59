"""ib_resample_renoise on the GPU (csrc/resample.hip).  -m gpu.

Shapes are those of tests/test_stitch_noise_kernels_gpu.py, whose harness is reused: windows of T = 8 frames every hop = 3 over
a trial of F = 17 frames (W = 4 windows, 1 .. 3 of them cover a frame), N = 2 trials, fp32 and bf16, with and without
observations.  Geometries (D, ld): (12, 16) is 8-wide with whole Philox blocks, (10, 16) 8-wide with blocks looked up per
element, (5, 5) element-wise.  Trial ids {5, 2^32 - 1}; a loop of S = 10 steps, jumps of back in {1, 3} from the positions
s in {back, S / 2, S}.

(a) Against float64 (tests/resample_restatement.py: the normals from oracle.ref_cpu.draw_words in domain 4): the error is at
    most |cz| GEN_TOL + ARITH max |want|, the bounds of tests/test_eta_kernels_gpu.py.
(b) All copies bitwise equal, pad columns 0, sentinels intact, z untouched, t_out == ddim_t[q].
(c) The observed elements after a jump to q >= 1 equal, bit for bit, those ib_stitch_ddim_step writes at step q - 1.
(d) Host step and device counter agree; the draw depends on (seed, trial id, visit) only: sub-batches, the row pitch, one
    window against the first copies of the stitched layout.
(e) The refusals, and a launch whose position lies outside back .. S leaves x and t_out untouched."""
import pytest
import torch

from tests import resample_restatement as RR
from tests.test_eta_kernels_gpu import ARITH, GEN_TOL
from tests.test_stitch_kernels_gpu import F, N, T, guarded, layout, operands, sentinels_ok
from tests.test_stitch_noise_kernels_gpu import col_mask, first_copies

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
S = 10
GEOM = [(12, 16), (10, 16), (5, 5)]
IDS = [5, 2 ** 32 - 1]
SEED = 0x1234_5678_9ABC_DEF0
BACKS = (1, 3)
CASES = [(dt, D, ld, cond) for dt in (torch.float32, BF) for D, ld in GEOM for cond in (False, True)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from inferbiomechanics_amd import hip
    hip.lib()


_TABS = {}


def tables(back):
    from inferbiomechanics_amd.diffusion.schedule import DiffusionTables
    if back not in _TABS:
        t = DiffusionTables(torch.device(DEV), num_sample_steps=S)
        t.set_resample(back)
        _TABS[back] = t
    return _TABS[back]


def run_jump(hip, tabs, lay, op, cond, mask, s, back, D, visit=3, ids=IDS, seed=SEED, by_counter=True, split=0):
    """one launch on clones of op -> (x, z, t_out, x's flat buffer, z's flat buffer).  by_counter: the position comes from the
    device counter (plus the host `split`), otherwise from the host alone"""
    W = lay["W"]
    shift = op["x"].storage_offset()
    xf, x = guarded(op["x"].shape, op["x"].dtype, shift)
    zf, z = guarded(op["x"].shape, op["x"].dtype, shift)
    x.copy_(op["x"])
    z.copy_(op["z"])
    ctr = torch.tensor([s - split], dtype=torch.int32, device=DEV)
    t_out = torch.full((op["x"].shape[0] * W,), -7, dtype=torch.int64, device=DEV)
    c = (op["x0"], z, mask.to(DEV), tabs.obs_coef) if cond else (None, None, None, None)
    st, cv, _ = lay["dev"]
    kw = dict(step=split, step_dev=ctr) if by_counter else dict(step=s)
    hip.resample_renoise(x, c[0], c[1], c[2], tabs.resample_coef, c[3], tabs.ddim_t, st, cv,
                         torch.tensor(ids, dtype=torch.int64, device=DEV), seed, back, visit, t_out, D=D, **kw)
    torch.cuda.synchronize()
    return x, z, t_out, xf, zf


# ---------------------------------------------------------------------------------------------------------------------
# (a), (b), (c) and the host step index against the device counter
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,D,ld,cond", CASES)
def test_overlapping_windows_against_float64_copies_and_the_pinned_bits(dt, D, ld, cond):
    from inferbiomechanics_amd import hip
    lay = layout(F)
    assert lay["W"] == 4
    op = operands(lay, D, ld, dt, 700 + D + (dt == BF))
    mask = col_mask(D, ld) if cond else None
    obs_cols = mask[0].bool() if cond else None
    X, X0, Z0 = (op[k + "_trial"] for k in ("x", "x0", "z"))
    st, cv, wn = lay["dev"]
    for back in BACKS:
        tabs = tables(back)
        rc, oc = tabs.resample_coef.cpu().double(), tabs.obs_coef.cpu().double()
        assert not rc[:back].any() and bool((rc[back:, 1] > 0).all())
        for s in (back, S // 2, S):
            q, visit = s - back, 3 + s
            x, z, t_out, xf, zf = run_jump(hip, tabs, lay, op, cond, mask, s, back, D, visit=visit)
            for kw in (dict(by_counter=False), dict(split=2)):
                x2, _, t2, _, _ = run_jump(hip, tabs, lay, op, cond, mask, s, back, D, visit=visit, **kw)
                assert torch.equal(x, x2) and torch.equal(t_out, t2), "host step index and device step counter disagree"
            # (b)
            assert sentinels_ok(xf) and sentinels_ok(zf), "wrote past the state or the noise buffer"
            assert bool((t_out == int(tabs.ddim_t[q])).all())
            xc = x.cpu()
            first = first_copies(xc, lay)
            assert torch.equal(xc, first[:, lay["gather"]]), (s, "copies of x differ")
            assert not xc[..., D:].any(), "pad columns must stay 0"
            assert torch.equal(z, op["z"]), "z is not written"
            # (a)
            Zn = RR.trial_jump_normals(F, D, ld, SEED, visit, IDS)
            want = RR.renoise(X, X0, Z0, obs_cols, rc[s], oc[q], Zn)
            err = float((first.double() - want).abs().max())
            tol = abs(float(rc[s, 1])) * GEN_TOL + ARITH[dt] * float(want.abs().max())
            print(f"renoise {dt} D={D} ld={ld} cond={cond} back={back} s={s}: max err {err:.3e} (tol {tol:.3e})")
            assert err <= tol, (s, err, tol)
            assert not torch.equal(xc, op["x"].cpu())
            # (c)
            if cond and q >= 1:
                stepped = op["x"].clone()
                hip.stitch_ddim_step(stepped, op["eps"], op["x0"], op["z"], mask.to(DEV), tabs.ddim_coef, tabs.obs_coef,
                                     tabs.ddim_t, st, cv, wn, step=q - 1, D=D)
                torch.cuda.synchronize()
                assert torch.equal(x[..., obs_cols.to(DEV)], stepped[..., obs_cols.to(DEV)]), \
                    (s, "the pinned value is not the one the update that arrived at position q wrote")


@pytest.mark.parametrize("dt,D,ld,cond", CASES)
def test_one_window_layout(dt, D, ld, cond):
    """W = 1 (F == T), as a per-window loop calls it: the same checks, and the draws are those of the first T frames of a
    stitched trial with the same id"""
    from inferbiomechanics_amd import hip
    lay1, layF = layout(T), layout(F)
    assert lay1["W"] == 1
    opF = operands(layF, D, ld, dt, 800 + D + (dt == BF))
    op1 = {}
    for k in ("x", "x0", "z"):                                         # the first T frames of the same trials
        _, v = guarded((N, 1, T, ld), dt)
        v.copy_(opF[k + "_trial"][:, None, :T].to(DEV))
        op1[k] = v
    mask = col_mask(D, ld) if cond else None
    tabs = tables(3)
    s = S // 2
    x1, z1, t1, xf, zf = run_jump(hip, tabs, lay1, op1, cond, mask, s, 3, D)
    xF, _, _, _, _ = run_jump(hip, tabs, layF, opF, cond, mask, s, 3, D)
    assert sentinels_ok(xf) and sentinels_ok(zf) and torch.equal(z1, op1["z"]) and bool((t1 == int(tabs.ddim_t[s - 3])).all())
    assert torch.equal(x1[:, 0].cpu(), first_copies(xF.cpu(), layF)[:, :T]), "the draw must not depend on the window layout"


# ---------------------------------------------------------------------------------------------------------------------
# (d) what the draw depends on
# ---------------------------------------------------------------------------------------------------------------------
def _sub(op, sel):
    out = {}
    for k in ("x", "x0", "z"):
        _, v = guarded((len(sel),) + tuple(op[k].shape[1:]), op[k].dtype)
        v.copy_(op[k][sel])
        out[k] = v
    return out


@pytest.mark.parametrize("dt,D,ld", [(torch.float32, 12, 16), (BF, 10, 16), (BF, 5, 5)])
@pytest.mark.parametrize("cond", [False, True])
def test_draw_depends_on_seed_trial_id_and_visit_only(dt, D, ld, cond):
    from inferbiomechanics_amd import hip
    tabs = tables(3)
    lay = layout(F)
    op = operands(lay, D, ld, dt, 900 + D)
    mask = col_mask(D, ld) if cond else None

    def run(sel, ids, visit=3, seed=SEED, s=5):
        return run_jump(hip, tabs, lay, _sub(op, sel), cond, mask, s, 3, D, visit=visit, ids=ids, seed=seed)[0]

    base = run([0], [42])
    for sel, ids, at in (([1, 0], [7, 42], 1), ([0, 1, 1], [42, 1, 2], 0), ([1, 1, 0, 1], [9, 8, 42, 7], 2)):
        assert torch.equal(run(sel, ids)[at], base[0]), "the draw must not depend on N or the batch position"
    for what, x in (("trial id", run([0], [43])), ("visit", run([0], [42], visit=4)), ("seed", run([0], [42], seed=SEED + 1))):
        assert not torch.equal(x, base), f"another {what}, the same draw"
    free = torch.ones(ld, dtype=torch.bool) if mask is None else ~mask[0].bool()
    free[D:] = False
    a, b = run([0], [42], s=5), run([0], [42], s=6)                    # the position picks the row, not the draw
    rc = tabs.resample_coef.cpu().double()
    za = (a.double().cpu() - rc[5, 0] * op["x"][:1].double().cpu()) / rc[5, 1]
    zb = (b.double().cpu() - rc[6, 0] * op["x"][:1].double().cpu()) / rc[6, 1]
    assert float((za - zb)[..., free].abs().max()) <= (0.1 if dt == BF else 1e-4), "the normal is keyed by the visit, not the step"


@pytest.mark.parametrize("cond", [False, True])
def test_fp32_pitched_and_unpitched_runs_agree(cond):
    from inferbiomechanics_amd import hip
    tabs = tables(1)
    lay = layout(F)
    D = 12
    outs = []
    for ld in (12, 16):
        op = operands(lay, D, ld, torch.float32, 77)                   # the same generator stream: the same logical values
        mask = col_mask(D, 16)[:, :ld].contiguous() if cond else None
        x, _, _, _, _ = run_jump(hip, tabs, lay, op, cond, mask, 4, 1, D)
        outs.append((x[..., :D].clone(), op["x"][..., :D].clone()))
    assert torch.equal(outs[0][1], outs[1][1]), "the test's own operands differ between the pitches"
    free = torch.ones(D, dtype=torch.bool) if not cond else ~col_mask(D, 16)[0, :D].bool()
    # free elements have one rounding form at either width; an observed element is pinned in the form of its width
    assert torch.equal(outs[0][0][..., free.to(DEV)], outs[1][0][..., free.to(DEV)])
    assert not torch.equal(outs[0][0], outs[0][1])


# ---------------------------------------------------------------------------------------------------------------------
# (e) refusals, and positions the host cannot refuse
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_refusals_and_positions_out_of_range():
    from inferbiomechanics_amd import hip
    tabs = tables(3)
    lay = layout(F)
    W, D, ld = lay["W"], 12, 16
    op = operands(lay, D, ld, torch.float32, 7)
    mask = col_mask(D, ld).to(DEV)
    st, cv, _ = lay["dev"]
    ids = torch.tensor(IDS, dtype=torch.int64, device=DEV)
    t_out = torch.full((N * W,), -7, dtype=torch.int64, device=DEV)
    ctr = torch.zeros(1, dtype=torch.int32, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()
    base = dict(x=p(op["x"]), x0=p(op["x0"]), z=p(op["z"]), mask=p(mask), coef=p(tabs.resample_coef), obs_coef=p(tabs.obs_coef),
                timesteps=p(tabs.ddim_t), num_steps=S, step=5, step_dev=None, back=3, visit=0, t_out=p(t_out), start=p(st),
                cover=p(cv), trial_id=p(ids), seed=3, N=N, W=W, T=T, F=F, D=D, ld=ld, dtype=hip.F32, stream=0)

    def call(**over):
        a = dict(base)
        a.update(over)                                                 # keeps the header's order of the keys
        return hip.lib().ib_resample_renoise(*a.values())

    ARG, DTYPE, UNSUP = -1, -2, -5
    before, before_z = op["x"].clone(), op["z"].clone()
    for name in ("x", "coef", "timesteps", "t_out", "start", "cover", "trial_id"):
        assert call(**{name: None}) == ARG, name
    four = ("x0", "z", "mask", "obs_coef")
    for name in four:                                                  # any mix of NULL and non-NULL
        assert call(**{name: None}) == ARG, name
        assert call(**{k: None for k in four if k != name}) == ARG, name
    for name in ("N", "W", "T", "F", "D", "num_steps"):
        assert call(**{name: 0}) == ARG, name
    for back in (0, -2):
        assert call(back=back) == ARG
    assert call(ld=D - 1) == ARG
    assert call(F=T - 1) == ARG
    assert call(dtype=7) == DTYPE
    assert call(T=1 << 20, F=1 << 20, ld=1 << 11, D=1 << 11) == UNSUP  # T * ld = 2^31
    assert call(T=8, F=1 << 20, ld=1 << 11, D=1 << 11) == UNSUP        # F * D = 2^31: the block index is one 32-bit word
    # positions outside back .. S: by the host index, by the counter, by their sum -- no row read, nothing written
    for step, c in ((2, None), (S + 1, None), (0, 2), (0, S + 1), (0, -1), (4, -2), (S, 1), (-(1 << 30), 0), (1 << 30, 0)):
        if c is not None:
            ctr.fill_(c)
        assert call(step=step, step_dev=None if c is None else p(ctr)) == 0, (step, c)
    torch.cuda.synchronize()
    assert torch.equal(op["x"], before) and torch.equal(op["z"], before_z), "a refused or out-of-range call must write nothing"
    assert bool((t_out == -7).all()), "an out-of-range position must leave t_out untouched"
    assert call() == 0
    torch.cuda.synchronize()
    assert not torch.equal(op["x"], before) and torch.equal(op["z"], before_z) and bool((t_out == int(tabs.ddim_t[2])).all())
    go = lambda **kw: hip.resample_renoise(op["x"], None, None, None, kw.get("coef", tabs.resample_coef), None, tabs.ddim_t, st, cv,
                                           kw.get("ids", ids), 3, kw.get("back", 3), kw.get("visit", 0), t_out, step=5, D=D)
    with pytest.raises(hip.HipError):
        go(coef=tabs.ddim_coef)                                        # [S, 2]
    with pytest.raises(hip.HipError, match="trial_ids"):
        go(ids=torch.zeros(N * W, dtype=torch.int64, device=DEV))
    with pytest.raises(hip.HipError, match="trial_ids"):
        go(ids=ids.cpu())
    with pytest.raises(hip.HipError, match="back"):
        go(back=0)
    with pytest.raises(hip.HipError, match="visit"):
        go(visit=1 << 32)
    with pytest.raises(hip.HipError, match="together"):
        hip.resample_renoise(op["x"], op["x0"], None, None, tabs.resample_coef, None, tabs.ddim_t, st, cv, ids, 3, 3, 0, t_out)
