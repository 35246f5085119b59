"""ib_mse_loss_weighted_partial + ib_mse_loss_weighted_finalize (include/ib_hip_lossweight.h) on the GPU: the diffusion loss
weighted by each window's noise level, with the unweighted error overall and per band of noise level from the same pass.

With a table of ones the pair is the existing conditional pair: dpred bit for bit, the weighted mean bit for bit the unweighted
one, the unweighted mean within 1e-5 of the existing entry's loss.  With a random table (1e-4 .. 1) everything is held against
a float64 restatement written here: dpred per element within TIGHT[dtype] (tests/test_cond_train_kernels_gpu.py), the two means
and every band sum within 1e-5 relative, every band count exactly.  Conditioning columns of dpred are +0 by bit pattern, pad
columns keep a sentinel, a second launch gives the same bits, dpred = None the same result vector.  Shapes: 4-wide and
element-wise kernels, a C that splits a 4-vector, the product's columns, T = 1 / 5 / 12 (a wave and a workgroup span several
windows), rows * cols no multiple of 2048, one case above 1024 * 2048 elements (grid capped, every thread loops); n_levels 7
(empty bands), 50, 1000, with t on both sides of every band edge.  -m gpu."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
LOSS_RT = 1e-5                                   # tests/test_cond_train_kernels_gpu.py
TIGHT = {torch.float32: 2e-5, BF: 3e-2}
SENT = 7.0
NB = 8

SHAPES = [(44, 0, 0), (44, 14, 4), (44, 16, 4), (43, 5, 0), (300, 270, 4)]       # (D, C, pad)
# (T, B): rows * D is above 2048 (several workgroups) and no multiple of 2048 for any D above: B * T is odd or 4 * odd, D has
# at most two factors of 2
WINDOWS = [(1, 131), (5, 23), (12, 21)]
LEVELS = [7, 50, 1000]


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from inferbiomechanics_amd import hip as h
    h.lib()
    assert h.loss_level_buckets() == NB == h.LOSS_LEVEL_BUCKETS
    return h


def rnd(shape, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64).to(dtype)


def levels_at_edges(B, n_levels, seed):
    """B levels: 0, n_levels - 1, both sides of every band edge, the rest random"""
    edge = sorted({-(-k * n_levels // NB) for k in range(1, NB)})
    must = [0, n_levels - 1] + [e for e in edge if e < n_levels] + [e - 1 for e in edge if e - 1 >= 0]
    g = torch.Generator().manual_seed(seed)
    rest = torch.randint(0, n_levels, (max(B - len(must), 0),), generator=g).tolist()
    t = (must + rest)[:B]
    perm = torch.randperm(B, generator=g).tolist()
    return torch.tensor([t[i] for i in perm], dtype=torch.int64)


def random_table(n_levels, seed):
    g = torch.Generator().manual_seed(seed)
    return (10.0 ** (-4.0 * torch.rand(n_levels, generator=g, dtype=torch.float64))).to(torch.float32)     # 1e-4 .. 1


def weighted(hip, pred, target, t, wtab, T, C, dpred, accum=None, result=None):
    rows, D = pred.shape
    ws = torch.empty(hip.mse_loss_weighted_workspace_bytes(rows * D), dtype=torch.uint8, device=DEV)
    res = torch.zeros(2 + 2 * NB, dtype=torch.float32, device=DEV) if result is None else result
    hip.mse_loss_weighted_partial(pred, target, ws, t, wtab, T, cond_cols=C, dpred=dpred)
    hip.mse_loss_weighted_finalize(ws, res, t, wtab.numel(), rows * D, rows * (D - C), accum=accum)
    return res


def cond_loss(hip, pred, target, C, dpred):
    rows, D = pred.shape
    ws = torch.empty(hip.mse_loss_workspace_bytes(rows * D), dtype=torch.uint8, device=DEV)
    res = torch.zeros(1, dtype=torch.float32, device=DEV)
    hip.mse_loss_partial_cond(pred, target, ws, C, dpred=dpred)
    hip.mse_loss_finalize_cond(ws, res, rows * D, rows * (D - C))
    return res


def as_int(v):
    return v.contiguous().view(torch.int16 if v.dtype == BF else torch.int32)


def setup(dtype, D, C, pad, T, B, n_levels, seed=0):
    rows, ld = B * T, D + pad
    pfull = torch.full((rows, ld), SENT, dtype=dtype, device=DEV)
    pfull[:, :D] = rnd((rows, D), 3 + seed, dtype).to(DEV)
    target = rnd((rows, D), 4 + seed, dtype).to(DEV)
    t = levels_at_edges(B, n_levels, 5 + seed).to(DEV)
    return rows, pfull[:, :D], target, t


def rel(a, e):
    return abs(a - e) / max(abs(e), 1e-30)


@pytest.mark.parametrize("dtype", [torch.float32, BF])
@pytest.mark.parametrize("n_levels", LEVELS)
@pytest.mark.parametrize("T,B", WINDOWS)
@pytest.mark.parametrize("D,C,pad", SHAPES)
def test_ones_table_is_the_existing_pair(hip, dtype, D, C, pad, T, B, n_levels):
    rows, pred, target, t = setup(dtype, D, C, pad, T, B, n_levels)
    assert (rows * D) % 2048 != 0 and rows * D > 2048
    ones = torch.ones(n_levels, dtype=torch.float32, device=DEV)
    dfull = torch.full((rows, D + pad), SENT, dtype=dtype, device=DEV)
    dref = torch.full((rows, D + pad), SENT, dtype=dtype, device=DEV)
    res = weighted(hip, pred, target, t, ones, T, C, dfull[:, :D])
    ref = cond_loss(hip, pred, target, C, dref[:, :D])
    torch.cuda.synchronize()
    assert torch.equal(as_int(dfull), as_int(dref)), "dpred must be ib_mse_loss_partial_cond's bit for bit, pad included"
    if C == 0:
        dplain = torch.full((rows, D + pad), SENT, dtype=dtype, device=DEV)
        ws = torch.empty(hip.mse_loss_workspace_bytes(rows * D), dtype=torch.uint8, device=DEV)
        hip.mse_loss_partial(pred, target, ws, dpred=dplain[:, :D])
        torch.cuda.synchronize()
        assert torch.equal(as_int(dfull), as_int(dplain)), "dpred must be ib_mse_loss_partial's on the same 2-D view"
    r = res.cpu()
    assert as_int(r[0:1]).item() == as_int(r[1:2]).item(), "weighted mean != unweighted mean at w = 1"
    print("ones", dtype, (D, C, pad), (T, B), n_levels, "loss", float(r[1]), "existing", float(ref), "rel",
          rel(float(r[1]), float(ref)))
    assert rel(float(r[1]), float(ref)) <= LOSS_RT


@pytest.mark.parametrize("dtype", [torch.float32, BF])
@pytest.mark.parametrize("n_levels", LEVELS)
@pytest.mark.parametrize("T,B", WINDOWS)
@pytest.mark.parametrize("D,C,pad", SHAPES)
def test_random_table_against_float64(hip, dtype, D, C, pad, T, B, n_levels):
    check_random_table(hip, dtype, D, C, pad, T, B, n_levels)


def check_random_table(hip, dtype, D, C, pad, T, B, n_levels):
    rows, pred, target, t = setup(dtype, D, C, pad, T, B, n_levels, seed=10)
    wtab = random_table(n_levels, 6).to(DEV)
    dfull = torch.full((rows, D + pad), SENT, dtype=dtype, device=DEV)
    res = weighted(hip, pred, target, t, wtab, T, C, dfull[:, :D])
    torch.cuda.synchronize()
    # ---- the float64 restatement
    q = (pred.double() - target.double()).cpu()[:, C:]
    tc = t.cpu()
    w = wtab.cpu().double()[tc].repeat_interleave(T)[:, None]                     # per row
    band = (tc * NB // n_levels).repeat_interleave(T)
    n_mean = rows * (D - C)
    gscale = float(np.float32(2.0) / np.float32(n_mean))
    e_dpred = q * gscale * w
    e_w, e_u = float((w * q * q).sum() / n_mean), float((q * q).sum() / n_mean)
    e_bands = [float((q[band == k] ** 2).sum()) for k in range(NB)]
    e_counts = [int((tc * NB // n_levels == k).sum()) for k in range(NB)]
    # ---- dpred
    got = dfull[:, C:D].double().cpu()
    err, ref = (got - e_dpred).abs().max().item(), e_dpred.abs().max().item()
    r = res.cpu().double().tolist()
    worst_band = max(rel(r[2 + k], e_bands[k]) for k in range(NB) if e_counts[k])
    print("random", dtype, (D, C, pad), (T, B), n_levels, "dpred err/ref", err / ref, "weighted rel", rel(r[0], e_w),
          "unweighted rel", rel(r[1], e_u), "worst band rel", worst_band, "counts", e_counts)
    assert err <= TIGHT[dtype] * ref
    assert torch.equal(as_int(dfull[:, :C]), torch.zeros_like(as_int(dfull[:, :C]))), "conditioning columns must be +0"
    assert torch.equal(dfull[:, D:], torch.full((rows, pad), SENT, dtype=dtype, device=DEV)), "pad columns were touched"
    assert rel(r[0], e_w) <= LOSS_RT and rel(r[1], e_u) <= LOSS_RT
    assert [int(c) for c in r[2 + NB:2 + 2 * NB]] == e_counts and r[2 + NB:2 + 2 * NB] == [float(c) for c in e_counts]
    for k in range(NB):
        if e_counts[k]:
            assert rel(r[2 + k], e_bands[k]) <= LOSS_RT, (k, r[2 + k], e_bands[k])
        else:
            assert r[2 + k] == 0.0, "an empty band must sum to 0"
    assert rel(sum(r[2:2 + NB]), r[1] * n_mean) <= LOSS_RT, "the band sums must add up to the unweighted sum"
    if n_levels < NB:
        assert 0 in e_counts, "fewer levels than bands leaves empty bands"


@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_capped_grid_every_thread_loops(hip, dtype):
    """just above 1024 * 2048 elements: the grid is capped at 1024 workgroups and every thread takes a second trip"""
    D, C, pad, T, n_levels = 300, 270, 4, 12, 1000
    B = 584                                                       # 584 * 12 * 300 = 2 102 400 > 2 097 152
    rows, pred, target, t = setup(dtype, D, C, pad, T, B, n_levels, seed=20)
    assert rows * D > 1024 * 2048 and hip.mse_loss_weighted_workspace_bytes(rows * D) == 1024 * (2 + NB) * 4
    wtab = random_table(n_levels, 7).to(DEV)
    dfull = torch.full((rows, D + pad), SENT, dtype=dtype, device=DEV)
    res = weighted(hip, pred, target, t, wtab, T, C, dfull[:, :D])
    torch.cuda.synchronize()
    q = (pred.double() - target.double())[:, C:]
    w = wtab.double()[t].repeat_interleave(T)[:, None]
    band = (t * NB // n_levels).repeat_interleave(T)
    n_mean = rows * (D - C)
    e_dpred = q * float(np.float32(2.0) / np.float32(n_mean)) * w
    err, ref = (dfull[:, C:D].double() - e_dpred).abs().max().item(), e_dpred.abs().max().item()
    r = res.cpu().double().tolist()
    e_w, e_u = float((w * q * q).sum() / n_mean), float((q * q).sum() / n_mean)
    print("capped", dtype, "dpred err/ref", err / ref, "weighted rel", rel(r[0], e_w), "unweighted rel", rel(r[1], e_u))
    assert err <= TIGHT[dtype] * ref
    assert rel(r[0], e_w) <= LOSS_RT and rel(r[1], e_u) <= LOSS_RT
    for k in range(NB):
        e = float((q[band == k] ** 2).sum())
        assert rel(r[2 + k], e) <= LOSS_RT, (k, r[2 + k], e)
        assert r[2 + NB + k] == float((t * NB // n_levels == k).sum())
    assert torch.equal(as_int(dfull[:, :C]), torch.zeros_like(as_int(dfull[:, :C])))
    assert torch.equal(dfull[:, D:], torch.full((rows, pad), SENT, dtype=dtype, device=DEV))


@pytest.mark.parametrize("dtype", [torch.float32, BF])
@pytest.mark.parametrize("D,C,pad", [(44, 14, 4), (43, 5, 0)])
def test_relaunch_none_dpred_and_accum(hip, dtype, D, C, pad):
    T, B, n_levels = 5, 23, 50
    rows, pred, target, t = setup(dtype, D, C, pad, T, B, n_levels, seed=30)
    wtab = random_table(n_levels, 8).to(DEV)
    dfull = torch.full((rows, D + pad), SENT, dtype=dtype, device=DEV)
    first = weighted(hip, pred, target, t, wtab, T, C, dfull[:, :D]).clone()
    d1 = dfull.clone()
    dfull[:, :C] = 5.0                                            # garbage: the next launch must clear it
    accum = torch.zeros(2 + 2 * NB, dtype=torch.float64, device=DEV)
    second = weighted(hip, pred, target, t, wtab, T, C, dfull[:, :D], accum=accum).clone()
    none = weighted(hip, pred, target, t, wtab, T, C, None, accum=accum).clone()
    weighted(hip, pred, target, t, wtab, T, C, None, accum=accum)
    torch.cuda.synchronize()
    assert torch.equal(as_int(dfull), as_int(d1)), "a second launch into the same buffers must give the same bits"
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))
    assert torch.equal(first.view(torch.int32), none.view(torch.int32)), "dpred = None must give the same result vector"
    a, r = accum.cpu().tolist(), first.cpu().double().tolist()
    assert a[2 + NB:] == [3.0 * c for c in r[2 + NB:]] and sum(a[2 + NB:]) == 3.0 * B
    for j in range(2 + NB):
        assert rel(a[j], 3.0 * r[j]) <= 1e-6 if r[j] else a[j] == 0.0, (j, a[j], r[j])


def test_out_of_range_levels_are_clamped(hip):
    """a level outside [0, n_levels) reads the table's first / last entry and counts in the first / last band"""
    D, C, T, B, n_levels = 44, 0, 5, 23, 50
    rows, pred, target, t = setup(torch.float32, D, C, 0, T, B, n_levels, seed=40)
    wtab = random_table(n_levels, 9).to(DEV)
    bad = t.clone()
    bad[0], bad[1], bad[2] = -3, n_levels, 1 << 40
    clamped = bad.clamp(0, n_levels - 1)
    da, db = torch.empty(rows, D, device=DEV), torch.empty(rows, D, device=DEV)
    ra = weighted(hip, pred, target, bad, wtab, T, C, da)
    rb = weighted(hip, pred, target, clamped, wtab, T, C, db)
    torch.cuda.synchronize()
    assert torch.equal(ra, rb) and torch.equal(da, db)


def test_bad_arguments_are_refused_without_a_launch(hip):
    import ctypes
    D, T, B, n_levels = 44, 5, 23, 50
    rows, pred, target, t = setup(torch.float32, D, 0, 0, T, B, n_levels, seed=50)
    wtab = torch.ones(n_levels, dtype=torch.float32, device=DEV)
    dpred = torch.full((rows, D), SENT, device=DEV)
    wsb = hip.mse_loss_weighted_workspace_bytes(rows * D)
    ws = torch.full((wsb // 4,), SENT, dtype=torch.float32, device=DEV)
    res = torch.full((2 + 2 * NB,), SENT, dtype=torch.float32, device=DEV)
    lib, s = hip.lib(), hip.stream_ptr()
    E_ARG = lib.ib_mse_loss_partial_cond(None, D, None, None, D, None, 0, rows, D, 0, 0, s)      # the library's IB_E_ARG
    assert E_ARG < 0

    def partial(rows=rows, rpw=T, C=0, tab=wtab.data_ptr(), tt=t.data_ptr(), bytes_=wsb, levels=n_levels):
        return lib.ib_mse_loss_weighted_partial(pred.data_ptr(), D, target.data_ptr(), dpred.data_ptr(), D, tt, tab, levels,
                                                rpw, ws.data_ptr(), bytes_, rows, D, C, 0, s)
    assert partial(rpw=T + 1) == E_ARG                  # rows % rows_per_window != 0
    assert partial(C=D) == E_ARG and partial(C=D + 3) == E_ARG and partial(C=-1) == E_ARG
    assert partial(tab=None) == E_ARG and partial(tt=None) == E_ARG
    assert partial(levels=0) == E_ARG
    small = partial(bytes_=wsb - 4)
    assert small < 0 and small != E_ARG and b"workspace" in lib.ib_error_string(small).lower()
    assert lib.ib_mse_loss_weighted_finalize(ws.data_ptr(), wsb - 4, t.data_ptr(), B, n_levels, res.data_ptr(), None,
                                             rows * D, rows * D, s) == small
    assert lib.ib_mse_loss_weighted_finalize(ws.data_ptr(), wsb, None, B, n_levels, res.data_ptr(), None, rows * D,
                                             rows * D, s) == E_ARG
    torch.cuda.synchronize()
    for buf in (dpred, ws, res):
        assert torch.equal(buf, torch.full_like(buf, SENT)), "a refused call must launch nothing"
    # the binding refuses the same before the library is asked
    for kw in ({"rows_per_window": T + 1}, {"rows_per_window": T, "cond_cols": D}):
        with pytest.raises(hip.HipError):
            hip.mse_loss_weighted_partial(pred, target, ws, t, wtab, **kw)
    with pytest.raises(hip.HipError):
        hip.mse_loss_weighted_partial(pred, target, ws[:8], t, wtab, T)
    assert partial() == 0                               # and the good call goes through
    torch.cuda.synchronize()
