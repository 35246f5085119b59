"""ib_vel_loss_partial and ib_vel_loss_finalize (include/ib_hip_velocity.h) on the GPU, held against the float64 restatement
velocity_loss.velocity_terms64 evaluated from the fp32 tables the kernel reads.

Shapes (D, C, pad) as in tests/test_prediction_kernels_gpu.py: the 4-wide and the element-wise kernel, a C that splits a
4-vector, the product's columns; fp32 and bf16; kinds eps, x0, v; n_levels 7 (empty bands), 50, 1000 with t at 0, n_levels - 1
and both sides of every band edge; T in {2, 3, FC, FC + 1, 2 FC + 1} with FC from the library's host query -- a window that is
all edges, one whole chunk, a chunk boundary with a last chunk of one frame, three chunks; B so that the launch spans several
workgroups and its units are no multiple of a workgroup's 256.

Tolerances are the project's constants, TIGHT and LOSS_RT of tests/test_loss_weight_kernels_gpu.py.  dpred is bounded per
element by TIGHT[dtype] * (|dm| + (|dp| + |dn|) * vscale * v), the magnitudes of the float64 parts and not their cancelling
sum, plus one ulp of the final rounding to the storage type.  Two things about that bound are settled here, in the inputs and
not in the bound:
  * It has no term for the rounding of q itself.  For eps and x0 q = pred - target is one fp32 subtraction, relative error
    2^-24, which |dm| covers.  For v the kernel forms the target in fp32, fmaf(a, eps, -(s * x0)), with an ABSOLUTE error of
    2^-24 (|s x0| + |target|) that no multiple of |q| covers where pred is close to the target.  That form is spelled, so the
    test restates it exactly (v_target32: a correctly rounded fp32 product, then the sum in float64 rounded to odd and then to
    fp32, which is the fma's single rounding) and hands the float64 restatement that target.
  * dp and dn inherit 2^-24 |q[f +- 1]| from the neighbours' q, which the bound covers through |dm| (|q[f +- 1]| <= |q[f]| +
    |dp or dn|) as long as 4 * 2^-24 * v * vscale <= TIGHT * w * gscale, i.e. v / w <= 83 (T - 1) / T for fp32.  The weight
    tables are random with v <= 3.2 w.
Every mean and band sum is within LOSS_RT relative, band counts are exact, conditioning columns are +0 by bit pattern, pad
columns keep a sentinel, the inputs are unchanged, a second launch gives identical bits.  -m gpu."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
LOSS_RT = 1e-5                                   # tests/test_loss_weight_kernels_gpu.py
TIGHT = {torch.float32: 2e-5, BF: 3e-2}
ULP = {torch.float32: 2.0 ** -23, BF: 2.0 ** -7}     # the spacing of the storage type relative to a value, at most
SENT = 7.0
NB = 8

SHAPES = [(44, 0, 0), (44, 14, 4), (43, 5, 0), (300, 270, 4)]       # (D, C, pad)
LEVELS = [7, 50, 1000]
KINDS = ["eps", "x0", "v"]
CHUNK_CASES = ["2", "3", "FC", "FC+1", "2FC+1"]


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from inferbiomechanics_amd import hip as h
    h.lib()
    assert h.loss_level_buckets() == NB == h.LOSS_LEVEL_BUCKETS
    assert h.vel_loss_frame_chunk() == h.VEL_FRAME_CHUNK >= 2
    return h


def frames(hip, case):
    FC = hip.vel_loss_frame_chunk()
    return {"2": 2, "3": 3, "FC": FC, "FC+1": FC + 1, "2FC+1": 2 * FC + 1}[case]


def windows(hip, D, T, wide):
    """B: at least 16 windows (levels_at_edges places 16 levels), the launch's units over several workgroups and no multiple
    of 256"""
    FC = hip.vel_loss_frame_chunk()
    per = -(-T // FC) * (D // 4 if wide else D)
    B = 19
    while hip.vel_loss_workspace_bytes(B * T, D, T) < 3 * 4 * (4 + 2 * NB) or (B * per) % 256 == 0:
        B += 1
    return B


def rnd(shape, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64).to(dtype)


def levels_at_edges(B, n_levels, seed):
    """B levels: 0, n_levels - 1, both sides of every band edge, the rest random"""
    edge = sorted({-(-k * n_levels // NB) for k in range(1, NB)})
    must = [0, n_levels - 1] + [e for e in edge if e < n_levels] + [e - 1 for e in edge if e - 1 >= 0]
    assert B >= len(must)
    g = torch.Generator().manual_seed(seed)
    rest = torch.randint(0, n_levels, (max(B - len(must), 0),), generator=g).tolist()
    t = (must + rest)[:B]
    perm = torch.randperm(B, generator=g).tolist()
    return torch.tensor([t[i] for i in perm], dtype=torch.int64)


_TABLES = {}


def tables(n_levels, kind):
    """fp32 on the device, made once per (n_levels, kind): random wtab in 1e-2 .. 1, vtab = wtab * 10^(-1.5 .. 0.5), random xtab
    in 1e-2 .. 1e2, the schedule's own utab, sqrt_ab, sqrt_1mab; and alpha_bar in float64"""
    key = (n_levels, kind)
    if key not in _TABLES:
        from inferbiomechanics_amd.diffusion.schedule import alphas_cumprod
        from inferbiomechanics_amd.prediction import eps_units
        g = torch.Generator().manual_seed(n_levels)
        r = lambda: torch.rand(n_levels, generator=g, dtype=torch.float64)
        w = 10.0 ** (-2.0 * r())
        v = w * 10.0 ** (2.0 * r() - 1.5)
        x = 10.0 ** (4.0 * r() - 2.0)
        ab = alphas_cumprod(n_levels)
        f = lambda a: a.to(torch.float32).to(DEV)
        _TABLES[key] = {"w": f(w), "v": f(v), "x": f(x), "u": torch.from_numpy(eps_units(ab, kind)).to(DEV),
                        "sa": f(torch.sqrt(ab)), "sb": f(torch.sqrt(1.0 - ab)), "ab": ab}
    return _TABLES[key]


def as_int(v):
    return v.contiguous().view(torch.int16 if v.dtype == BF else torch.int32)


def rel(a, e):
    return abs(a - e) / max(abs(e), 1e-30)


def v_target32(a32, s32, x0, eps):
    """the kernel's fp32 target of kind v, fmaf(a, eps, -(s * x0)) with s * x0 rounded first, bit for bit: numpy arrays, a32 /
    s32 fp32 per element, x0 / eps values that fp32 holds.  a * eps is exact in float64 (two 24-bit factors); the sum with -p
    is rounded to odd there (TwoSum gives the rounding error, an inexact even result moves to its odd neighbour on the side of
    the true value), after which the rounding to fp32 is the one rounding of the fused operation."""
    p = (s32.astype(np.float32) * x0.astype(np.float32)).astype(np.float64)
    prod = a32.astype(np.float64) * eps.astype(np.float64)
    s = prod - p
    bb = s - prod
    err = (prod - (s - bb)) + (-p - bb)
    even = (s.view(np.int64) & 1) == 0
    move = (err != 0) & even
    s = np.where(move, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def launch(hip, kind, pred, x0, eps, t, tb, T, C, dpred, vtab=None):
    rows, D = pred.shape
    ws = torch.zeros(hip.vel_loss_workspace_bytes(rows, D, T), dtype=torch.uint8, device=DEV)
    res = torch.zeros(hip.VEL_RESULT_LEN, dtype=torch.float32, device=DEV)
    hip.vel_loss_partial(pred, x0, eps, ws, t, tb["w"], tb["u"], tb["v"] if vtab is None else vtab, tb["x"], tb["sa"], tb["sb"],
                         T, kind, cond_cols=C, dpred=dpred)
    hip.vel_loss_finalize(ws, res, t, tb["w"].numel(), rows, D, C, T)
    return res, ws


def restate(kind, pred, x0, eps, t, tb, B, T, D, C, vtab=None):
    """velocity_terms64 on the device in float64 from the kernel's own tables; kind v: with the kernel's fp32 target"""
    from inferbiomechanics_amd.velocity_loss import velocity_terms64
    target = None
    if kind == "v":
        tc = t.cpu().numpy()
        a32 = np.repeat(tb["sa"].cpu().numpy()[tc], T)[:, None]
        s32 = np.repeat(tb["sb"].cpu().numpy()[tc], T)[:, None]
        target = torch.from_numpy(v_target32(a32, s32, x0.float().cpu().numpy(), eps.float().cpu().numpy())).view(B, T, D)
    return velocity_terms64(pred.double().reshape(B, T, D), x0.double().reshape(B, T, D), eps.double().reshape(B, T, D), t, tb["ab"],
                            kind, tb["w"], tb["u"], tb["v"] if vtab is None else vtab, tb["x"], cond_cols=C, target=target)


def check_dpred(dtype, got, e, what):
    """got [B, T, D] float64 of the device's dpred against the restatement e, per element"""
    bound = TIGHT[dtype] * (e["dm"].abs() + (e["dp"].abs() + e["dn"].abs()) * e["vscale"] * e["v"]) + ULP[dtype] * e["dpred"].abs()
    over = (got - e["dpred"]).abs() - bound
    worst = ((got - e["dpred"]).abs() / bound.clamp_min(1e-300)).max().item()
    print(what, "dpred worst error / bound", worst)
    assert over.max().item() <= 0.0, f"{what}: dpred beyond its per-element bound by {over.max().item()} (ratio {worst})"


def check_sums(hip, res, e, n_levels, t, what):
    r = res.cpu().double().tolist()
    counts = e["counts"].cpu().tolist()
    figures = {"total": (r[hip.VEL_R_TOTAL], float(e["loss"])), "mse": (r[hip.VEL_R_MSE], float(e["mse"])),
               "eps": (r[hip.VEL_R_EPS], float(e["eps_mse"])), "vel": (r[hip.VEL_R_VEL], float(e["vel"])),
               "x0": (r[hip.VEL_R_X0], float(e["x0_vel"]))}
    print(what, {k: rel(*v) for k, v in figures.items()}, "counts", counts)
    for k, (a, b) in figures.items():
        assert rel(a, b) <= LOSS_RT, (what, k, a, b)
    assert r[hip.VEL_R_COUNTS:hip.VEL_R_COUNTS + NB] == [float(c) for c in counts], "band counts are exact"
    assert counts == [int((t.cpu() * NB // n_levels == k).sum()) for k in range(NB)]
    for k in range(NB):
        for at, name in ((hip.VEL_R_BANDS, "bands"), (hip.VEL_R_X0_BANDS, "x0_bands")):
            if counts[k]:
                assert rel(r[at + k], float(e[name][k])) <= LOSS_RT, (what, name, k, r[at + k], float(e[name][k]))
            else:
                assert r[at + k] == 0.0, "an empty band must sum to 0"


def setup(dtype, D, pad, T, B, n_levels, seed=0, offset=0):
    rows, ld = B * T, D + pad
    store = torch.full((rows * ld + offset,), SENT, dtype=dtype, device=DEV)
    pfull = store[offset:].view(rows, ld)
    pfull[:, :D] = rnd((rows, D), 3 + seed, dtype).to(DEV)
    x0, eps = rnd((rows, D), 4 + seed, dtype).to(DEV), rnd((rows, D), 6 + seed, dtype).to(DEV)
    t = levels_at_edges(B, n_levels, 5 + seed).to(DEV)
    return rows, pfull, x0, eps, t


@pytest.mark.parametrize("dtype", [torch.float32, BF])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_levels", LEVELS)
@pytest.mark.parametrize("case", CHUNK_CASES)
@pytest.mark.parametrize("D,C,pad", SHAPES)
def test_against_float64(hip, dtype, kind, n_levels, case, D, C, pad):
    T = frames(hip, case)
    B = windows(hip, D, T, wide=D % 4 == 0)
    rows, pfull, x0, eps, t = setup(dtype, D, pad, T, B, n_levels, seed=n_levels + T)
    pred = pfull[:, :D]
    keep = [v.clone() for v in (pfull, x0, eps, t)]
    tb = tables(n_levels, kind)
    dfull = torch.full((rows, D + pad), SENT, dtype=dtype, device=DEV)
    res, ws = launch(hip, kind, pred, x0, eps, t, tb, T, C, dfull[:, :D])
    torch.cuda.synchronize()
    d1, r1, w1 = dfull.clone(), res.clone(), ws.clone()
    dfull[:, :C] = 5.0                                            # garbage: the next launch must clear it
    res2, ws2 = launch(hip, kind, pred, x0, eps, t, tb, T, C, dfull[:, :D])
    torch.cuda.synchronize()
    assert torch.equal(as_int(dfull), as_int(d1)) and torch.equal(ws2, w1), "a second launch must give the same bits"
    assert torch.equal(res2.view(torch.int32), r1.view(torch.int32))
    for now, was in zip((pfull, x0, eps, t), keep):
        assert torch.equal(now, was), "the inputs must be unchanged"
    what = f"{kind} {dtype} {(D, C, pad)} T={T} B={B} levels={n_levels}"
    e = restate(kind, pred, x0, eps, t, tb, B, T, D, C)
    check_dpred(dtype, dfull[:, :D].double().reshape(B, T, D), e, what)
    assert torch.equal(as_int(dfull[:, :C]), torch.zeros_like(as_int(dfull[:, :C]))), "conditioning columns must be +0"
    assert torch.equal(dfull[:, D:], torch.full((rows, pad), SENT, dtype=dtype, device=DEV)), "pad columns were touched"
    check_sums(hip, res, e, n_levels, t, what)
    # sums only: no dpred, the same workspace
    res3, ws3 = launch(hip, kind, pred, x0, eps, t, tb, T, C, None)
    torch.cuda.synchronize()
    assert torch.equal(ws3, w1) and torch.equal(res3.view(torch.int32), r1.view(torch.int32))


@pytest.mark.parametrize("dtype", [torch.float32, BF])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", ["2", "FC+1", "2FC+1"])
@pytest.mark.parametrize("D,C,pad", [(44, 14, 4), (43, 5, 0)])
def test_windows_are_isolated(hip, dtype, kind, case, D, C, pad):
    """pred, x0 and eps constant over each window's frames, so pred - target is -- bit for bit, the same operations on the
    same values -- and pred differing by 1e3 between neighbouring windows: every frame difference inside a window is exactly
    0, and a difference taken across a window boundary would be 1e3"""
    T, n_levels = frames(hip, case), 50
    B = windows(hip, D, T, wide=D % 4 == 0)
    rows = B * T
    per_window = lambda seed: rnd((B, 1, D), seed, dtype).expand(B, T, D).reshape(rows, D).contiguous().to(DEV)
    step = (1e3 * torch.arange(B, dtype=torch.float64)).view(B, 1, 1).expand(B, T, D).reshape(rows, D).to(DEV)
    pfull = torch.full((rows, D + pad), SENT, dtype=dtype, device=DEV)
    pfull[:, :D] = (per_window(31).double() + step).to(dtype)
    pred, x0, eps = pfull[:, :D], per_window(32), per_window(33)
    t = levels_at_edges(B, n_levels, 34).to(DEV)
    tb = tables(n_levels, kind)
    dfull = torch.full((rows, D + pad), SENT, dtype=dtype, device=DEV)
    res, ws = launch(hip, kind, pred, x0, eps, t, tb, T, C, dfull[:, :D])
    torch.cuda.synchronize()
    r = res.cpu().tolist()
    assert r[hip.VEL_R_VEL] == 0.0 and r[hip.VEL_R_X0] == 0.0, "a frame difference crossed a window boundary"
    assert r[hip.VEL_R_X0_BANDS:hip.VEL_R_X0_BANDS + NB] == [0.0] * NB
    parts = ws.view(torch.float32).view(-1, 4 + 2 * NB)
    assert torch.equal(parts[:, 2 + NB:], torch.zeros_like(parts[:, 2 + NB:])), "sv, sx and every sxb of every workgroup"
    assert r[hip.VEL_R_TOTAL] == r[hip.VEL_R_MSE] > 0.0
    e = restate(kind, pred, x0, eps, t, tb, B, T, D, C)
    assert float(e["vel"]) == 0.0 and float(e["dn"].abs().max()) == 0.0, "the restatement sees constant windows too"
    got = dfull[:, :D].double().reshape(B, T, D)
    bound = TIGHT[dtype] * e["dm"].abs() + ULP[dtype] * e["dm"].abs()
    assert ((got - e["dm"]).abs() <= bound).all(), "dpred must be the dm of the restatement"
    assert torch.equal(as_int(dfull[:, :C]), torch.zeros_like(as_int(dfull[:, :C])))
    assert torch.equal(dfull[:, D:], torch.full((rows, pad), SENT, dtype=dtype, device=DEV))


@pytest.mark.parametrize("dtype", [torch.float32, BF])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", ["2", "FC+1"])
@pytest.mark.parametrize("D,C,pad", SHAPES)
def test_zero_velocity_table_gives_the_prediction_entrys_gradient(hip, dtype, kind, case, D, C, pad):
    T, n_levels = frames(hip, case), 50
    B = windows(hip, D, T, wide=D % 4 == 0)
    rows, pfull, x0, eps, t = setup(dtype, D, pad, T, B, n_levels, seed=70)
    pred = pfull[:, :D]
    tb = tables(n_levels, kind)
    zeros = torch.zeros(n_levels, dtype=torch.float32, device=DEV)
    dfull = torch.full((rows, D + pad), SENT, dtype=dtype, device=DEV)
    dref = torch.full((rows, D + pad), SENT, dtype=dtype, device=DEV)
    res, _ = launch(hip, kind, pred, x0, eps, t, tb, T, C, dfull[:, :D], vtab=zeros)
    ws_ref = torch.zeros(hip.mse_loss_weighted_workspace_bytes(rows * D), dtype=torch.uint8, device=DEV)
    res_ref = torch.zeros(2 + 2 * NB, dtype=torch.float32, device=DEV)
    hip.mse_loss_pred_partial(pred, x0, eps, ws_ref, t, tb["w"], tb["u"], tb["sa"], tb["sb"], T, kind, cond_cols=C,
                              dpred=dref[:, :D])
    hip.mse_loss_weighted_finalize(ws_ref, res_ref, t, n_levels, rows * D, rows * (D - C))
    torch.cuda.synchronize()
    assert bool((dfull == dref).all()), "dpred must compare equal to ib_mse_loss_pred_partial's, pad included"
    r, rr = res.cpu().tolist(), res_ref.cpu().tolist()
    assert r[hip.VEL_R_VEL] == 0.0 and r[hip.VEL_R_TOTAL] == r[hip.VEL_R_MSE]
    assert rel(r[hip.VEL_R_MSE], rr[0]) <= LOSS_RT and rel(r[hip.VEL_R_EPS], rr[1]) <= LOSS_RT      # another order of the sums
    assert r[hip.VEL_R_COUNTS:hip.VEL_R_COUNTS + NB] == rr[2 + NB:2 + 2 * NB]
    assert r[hip.VEL_R_X0] > 0.0, "the x0-unit report does not depend on the weight of the term"


@pytest.mark.parametrize("dtype", [torch.float32, BF])
@pytest.mark.parametrize("kind", KINDS)
def test_element_wise_path_from_an_offset_base_pointer(hip, dtype, kind):
    """44 columns would take the 4-wide kernel; a base pointer one element off a 4-element boundary must not"""
    D, C, pad, n_levels = 44, 14, 4, 50
    T = frames(hip, "FC+1")
    B = windows(hip, D, T, wide=False)
    rows, pfull, x0, eps, t = setup(dtype, D, pad, T, B, n_levels, seed=90, offset=1)
    pred = pfull[:, :D]
    assert pred.data_ptr() % (4 * pred.element_size()) != 0
    tb = tables(n_levels, kind)
    dstore = torch.full((rows * (D + pad) + 1,), SENT, dtype=dtype, device=DEV)
    dfull = dstore[1:].view(rows, D + pad)
    res, _ = launch(hip, kind, pred, x0, eps, t, tb, T, C, dfull[:, :D])
    torch.cuda.synchronize()
    what = f"offset {kind} {dtype}"
    e = restate(kind, pred, x0, eps, t, tb, B, T, D, C)
    check_dpred(dtype, dfull[:, :D].double().reshape(B, T, D), e, what)
    check_sums(hip, res, e, n_levels, t, what)
    assert torch.equal(as_int(dfull[:, :C]), torch.zeros_like(as_int(dfull[:, :C])))
    assert torch.equal(dfull[:, D:], torch.full((rows, pad), SENT, dtype=dtype, device=DEV)) and float(dstore[0]) == SENT
    # the aligned launch on the same values: the 4-wide kernel computes the same elements, its sums in another order
    dal = torch.full((rows, D + pad), SENT, dtype=dtype, device=DEV)
    pal = pfull.clone()
    res_al, _ = launch(hip, kind, pal[:, :D], x0, eps, t, tb, T, C, dal[:, :D])
    torch.cuda.synchronize()
    assert torch.equal(as_int(dal), as_int(dfull)), "one spelled form at both widths: dpred bit for bit"
    assert rel(float(res_al[0]), float(res[0])) <= LOSS_RT


def test_bad_arguments_are_refused_without_a_launch(hip):
    D, T, B, n_levels = 44, 5, 23, 50
    rows, pfull, x0, eps, t = setup(torch.float32, D, 0, T, B, n_levels, seed=50)
    ones = torch.ones(n_levels, dtype=torch.float32, device=DEV)
    dpred = torch.full((rows, D), SENT, device=DEV)
    wsb = hip.vel_loss_workspace_bytes(rows, D, T)
    ws = torch.full((wsb // 4,), SENT, dtype=torch.float32, device=DEV)
    lib, s = hip.lib(), hip.stream_ptr()
    E_ARG = lib.ib_mse_loss_partial_cond(None, D, None, None, D, None, 0, rows, D, 0, 0, s)      # the library's IB_E_ARG
    o = ones.data_ptr()

    def partial(kind=2, rpw=T, C=0, vtab=o, bytes_=wsb, dtype=0, n=rows):
        return lib.ib_vel_loss_partial(pfull.data_ptr(), D, x0.data_ptr(), eps.data_ptr(), dpred.data_ptr(), D, t.data_ptr(), o,
                                       o, vtab, o, o, o, n_levels, rpw, ws.data_ptr(), bytes_, n, D, C, kind, dtype, s)
    assert partial(kind=3) == E_ARG and partial(rpw=1, n=B) == E_ARG and partial(rpw=T + 1) == E_ARG and partial(C=D) == E_ARG
    assert partial(vtab=None) == E_ARG
    assert partial(bytes_=wsb - 1) not in (0, E_ARG) and partial(dtype=5) not in (0, E_ARG)
    torch.cuda.synchronize()
    assert bool((dpred == SENT).all()) and bool((ws == SENT).all()), "a refused call must not launch"
    assert partial() == 0
    torch.cuda.synchronize()
    assert not bool((dpred == SENT).any())
