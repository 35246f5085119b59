"""The three entries of include/ib_hip_standardize.h on the GPU: the moments against a float64 two-pass reference within
the bound the one-pass shifted sums allow, bit-reproducible; the affine bit for bit against tests/standardize_restatement.py
at every dtype pair, width, geometry and sub-range, with everything outside the window untouched.

The moments' bound.  Each of the R <= 2^16 rows adds d and d*d to fp64 sums: a relative error of at most R 2^-53 < 1e-11
in S1 and S2 whatever the order of the adds (per lane, per workgroup, per slot).  var = S2/R - md^2 loses a factor
(1 + md^2/var) to cancellation, md = mean - shift; the inputs put row 0 (the shift) within 3 sigma of the mean, so the factor
is at most 10 and the error of sd at most 1e-10 sd, of md at most 1e-11 (|md| + sd).  The float64 reference is as good.
Both stay inside 1e-9 sd; the rounding of the result to fp32 adds half an ulp: the test allows one."""
import numpy as np
import pytest
import torch

from tests import standardize_restatement as SR

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
DEV = "cuda"


def column_params(D, gen):
    """per column (mean, spread): column 0 is offset (1e4 +- 1), column 1 constant, the rest of order 10^-2 .. 10"""
    mu = (torch.rand(D, generator=gen) * 4 - 2).double()
    sg = (10.0 ** (torch.rand(D, generator=gen) * 3 - 2)).double()
    mu[0], sg[0] = 1.0e4, 1.0
    if D > 1:
        mu[1], sg[1] = 0.7, 0.0
    return mu, sg


def make_table(n, T, D, pitch, dtype, seed, offset=0):
    """[n, pitch] of `dtype` on the device (its base `offset` elements into an allocation), NaN behind T * D, row 0 of
    window 0 within 3 sigma of the column means"""
    gen = torch.Generator().manual_seed(seed)
    mu, sg = column_params(D, gen)
    z = torch.randn(n, T, D, generator=gen, dtype=torch.float64)
    z[0, 0].clamp_(-2.5, 2.5)
    host = torch.full((n, pitch), float("nan"), dtype=torch.float64)
    host[:, :T * D] = (mu + sg * z).reshape(n, T * D)
    buf = torch.empty(offset + n * pitch, dtype=dtype, device=DEV)
    table = buf[offset:].view(n, pitch)
    table.copy_(host.to(torch.float32).to(dtype))
    return table


def run_moments(hip, table, T, D, G, chunks=None, min_std=1e-6):
    shift = table[0, :D].to(F32).contiguous()
    acc = hip.column_moments_acc(D, DEV, G)
    n = table.shape[0]
    for a, b in (chunks or [(0, n)]):
        hip.column_moments(table[a:b], T, D, shift, acc)
    mean, scale, inv = hip.column_moments_finalize(acc, n * T, shift, min_std)
    torch.cuda.synchronize()
    return acc, mean.cpu().numpy(), scale.cpu().numpy(), inv.cpu().numpy()


def check_moments(table, T, D, mean, scale, inv, min_std=1e-6):
    ref_mean, ref_sd = SR.moments_ref(SR.table_rows(table, T, D))
    assert np.isfinite(mean).all() and np.isfinite(scale).all() and np.isfinite(inv).all(), "the pad is not read"
    err_m = np.abs(mean.astype(np.float64) - ref_mean)
    bound_m = SR.ulp32(ref_mean) + 1e-9 * ref_sd
    assert (err_m <= bound_m).all(), (err_m / bound_m).max()
    live = ref_sd > 10 * min_std
    assert (scale[~live] == 1.0).all(), "a constant column keeps scale 1"
    err_s = np.abs(scale.astype(np.float64) - ref_sd)[live]
    bound_s = (SR.ulp32(ref_sd) + 1e-9 * ref_sd)[live]
    assert (err_s <= bound_s).all(), (err_s / bound_s).max()
    assert np.array_equal(SR.bits(inv), SR.bits(SR.inv_rule(scale))), "inv is the rule applied to the fp32 scale"
    return ref_mean, ref_sd


# (D, T, n, G): N T below G, and N T no multiple of G
SHAPES = [(1, 1, 5, 8), (1, 50, 37, 64), (7, 1, 1000, 64), (7, 50, 37, 1024), (300, 1, 3, 8), (300, 50, 41, 256)]


@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("D,T,n,G", SHAPES)
def test_moments_against_float64_and_reproducible(D, T, n, G, dtype):
    from inferbiomechanics_amd import hip
    per = T * D
    assert n * T < G or (n * T) % G != 0
    layouts = {"pitch8": ((per + 7) // 8 * 8 + 8, 0), "dense": (per, 0), "odd pitch": (per + 3, 0), "offset base": (per + 8, 1)}
    for name, (pitch, offset) in layouts.items():
        table = make_table(n, T, D, pitch, dtype, seed=D * 100 + T, offset=offset)
        acc, mean, scale, inv = run_moments(hip, table, T, D, G)
        ref_mean, _ = check_moments(table, T, D, mean, scale, inv)
        if D > 1:
            assert scale[1] == 1.0 and mean[1] == np.float32(ref_mean[1]), f"{name}: a constant column's mean is exact"
        acc2, mean2, scale2, inv2 = run_moments(hip, table, T, D, G)
        assert torch.equal(acc.view(torch.int64), acc2.view(torch.int64)), f"{name}: two runs, the same bits"
        assert np.array_equal(SR.bits(mean), SR.bits(mean2)) and np.array_equal(SR.bits(scale), SR.bits(scale2))


@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_moments_three_unequal_chunks_into_one_accumulator(dtype):
    from inferbiomechanics_amd import hip
    D, T, n = 300, 50, 41
    table = make_table(n, T, D, T * D + 8, dtype, seed=11)
    _, mean, scale, inv = run_moments(hip, table, T, D, 256, chunks=[(0, 5), (5, 6), (6, 41)])
    check_moments(table, T, D, mean, scale, inv)
    _, mean1, scale1, inv1 = run_moments(hip, table[:6], T, D, 256, chunks=[(0, 5), (5, 6)])
    check_moments(table[:6], T, D, mean1, scale1, inv1)


def test_moments_offset_column_and_min_std():
    """a column of mean 1e4 and spread 1 in fp32: E[x^2] - E[x]^2 without the shift would lose 8 digits; and min_std"""
    from inferbiomechanics_amd import hip
    table = make_table(64, 50, 7, 352, F32, seed=3)
    _, mean, scale, inv = run_moments(hip, table, 50, 7, 64)
    _, ref_sd = check_moments(table, 50, 7, mean, scale, inv)
    assert abs(mean[0] - 1.0e4) < 0.2 and abs(scale[0] - 1.0) < 0.1 and abs(ref_sd[0] - 1.0) < 0.1
    _, _, big, inv_big = run_moments(hip, table, 50, 7, 64, min_std=5.0)
    assert ((big == 1.0) | (big > 5.0)).all() and big[0] == 1.0 and inv_big[0] == 1.0


# ---------------------------------------------------------------------------------------------------------------------
# the affine
# ---------------------------------------------------------------------------------------------------------------------
SENTINEL = -123.0        # exact in bf16


def make_side(geometry, N, T, D, ld, dtype, gen, offset, fill):
    """a table [N, ld] (ld = pitch >= T D) or a state [N, T, ld] of `dtype`, its base `offset` elements into an allocation;
    `fill` None: SENTINEL everywhere, else random values of order `fill`"""
    shape = (N, ld) if geometry == "table" else (N, T, ld)
    numel = int(np.prod(shape))
    buf = torch.empty(offset + numel, dtype=dtype, device=DEV)
    t = buf[offset:].view(shape)
    if fill is None:
        t.fill_(SENTINEL)
    else:
        t.copy_((torch.randn(shape, generator=gen) * fill + 0.5 * fill).to(dtype))
    return t


def windowed(t, geometry, T, D):
    """the [N, T, D'] view of a side that holds the D feature columns first in every row"""
    return t[:, :T * D].reshape(t.shape[0], T, D) if geometry == "table" else t


def run_affine(geometry, sdt, ddt, mode, N, T, D, s_ld, d_ld, cols=None, inplace=False, a_none=False, offset=0, seed=0):
    from inferbiomechanics_amd import hip
    gen = torch.Generator().manual_seed(seed)
    a = torch.randn(D, generator=gen) * 3
    b = torch.rand(D, generator=gen) * 2 + 0.25
    src = make_side(geometry, N, T, D, s_ld, sdt, gen, offset, fill=4.0)
    dst = src if inplace else make_side(geometry, N, T, D, d_ld, ddt, gen, offset, fill=None)
    before_src = src.clone()
    sv, dv = windowed(src, geometry, T, D), windowed(dst, geometry, T, D)
    want = SR.affine_into(dv, sv, None if a_none else a.numpy(), b.numpy(), mode, cols)
    whole_before = SR.widen(dst).copy()
    hip.column_affine(src, dst, None if a_none else a.to(DEV), b.to(DEV), cols=cols, mode=mode,
                      window=T if geometry == "table" else None)
    torch.cuda.synchronize()
    got = SR.widen(windowed(dst, geometry, T, D))
    assert np.array_equal(SR.bits(got), SR.bits(want)), np.argwhere(SR.bits(got) != SR.bits(want))[:4]
    # what lies outside the [N, T, D] view: a table's pad behind T D (a state's pad columns are inside the view)
    whole_after = SR.widen(dst)
    if geometry == "table":
        assert np.array_equal(SR.bits(whole_after[:, T * D:]), SR.bits(whole_before[:, T * D:])), "the pad is not written"
    if not inplace:
        assert torch.equal(src.view(torch.int16 if sdt == BF else torch.int32),
                           before_src.view(torch.int16 if sdt == BF else torch.int32)), "src is only read"


# (src dtype, dst dtype, mode, in place, a is None)
PAIRS = [(F32, F32, 0, False, False), (F32, BF, 0, False, False), (BF, BF, 0, True, False), (BF, F32, 1, False, False),
         (BF, BF, 1, False, True), (F32, F32, 1, True, False)]
PAIR_IDS = ["f32-f32 m0", "f32-bf16 m0", "bf16 in place m0", "bf16-f32 m1", "bf16 m1 no a", "f32 in place m1"]


@pytest.mark.parametrize("sdt,ddt,mode,inplace,a_none", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("geometry", ["table", "state"])
def test_affine_bit_for_bit(geometry, sdt, ddt, mode, inplace, a_none):
    kw = dict(inplace=inplace, a_none=a_none)
    if geometry == "table":
        # vector: D, pitch multiples of 8; scalar: D = 37 (rows of a window not 16-byte aligned), odd pitch, an offset base
        run_affine("table", sdt, ddt, mode, 5, 6, 40, 248, 248, **kw)
        run_affine("table", sdt, ddt, mode, 5, 6, 37, 222 + 3, 222 + 3, seed=1, **kw)
        run_affine("table", sdt, ddt, mode, 5, 6, 40, 248, 248, offset=1, seed=2, **kw)
        run_affine("table", sdt, ddt, mode, 300, 50, 40, 2000, 2000, seed=3, **kw)          # more than one block, grid stride
        # whole dense rows are flat runs of 8 values whatever D is: one run per window with a tail of 4 (pitch % 8 == 0), one
        # run over a dense table whose vectors wrap from row to row, and rows too wide for the coefficients' LDS copy
        run_affine("table", sdt, ddt, mode, 5, 5, 12, 64, 64, seed=4, **kw)
        run_affine("table", sdt, ddt, mode, 700, 3, 300, 900, 900, seed=5, **kw)
        run_affine("table", sdt, ddt, mode, 3, 1, 2056, 2056, 2056, seed=6, **kw)
    else:
        run_affine("state", sdt, ddt, mode, 3, 6, 40, 48, 40 if not inplace else 48, **kw)  # ld > D: pad columns untouched
        run_affine("state", sdt, ddt, mode, 3, 6, 37, 37, 37, seed=1, **kw)                 # ld % 8 != 0
        run_affine("state", sdt, ddt, mode, 3, 6, 40, 48, 48, offset=1, seed=2, **kw)
        run_affine("state", sdt, ddt, mode, 2, 1, 40, 40, 40, seed=3, **kw)                 # T = 1
        run_affine("state", sdt, ddt, mode, 6, 73, 40, 48, 40 if not inplace else 48, seed=4, **kw)   # a trial: F = 73


@pytest.mark.parametrize("sdt,ddt,mode,inplace,a_none", PAIRS[1:4], ids=PAIR_IDS[1:4])
@pytest.mark.parametrize("cols", [(8, 16), (3, 9), (39, 1)], ids=["vector window", "scalar window", "last column"])
def test_affine_sub_range_leaves_the_rest(cols, sdt, ddt, mode, inplace, a_none):
    """c0 > 0, w < D: the columns outside the window, pad columns and pads keep the sentinel (or, in place, their values)"""
    for geometry, ld in (("table", 6 * 40 + 8), ("state", 48)):
        run_affine(geometry, sdt, ddt, mode, 4, 6, 40, ld, ld, cols=cols, inplace=inplace, a_none=a_none, seed=5)


def test_affine_refusals_launch_nothing():
    from inferbiomechanics_amd import hip
    x = torch.zeros(2, 3, 8, device=DEV)
    a, b = torch.zeros(8, device=DEV), torch.ones(8, device=DEV)
    for bad in (lambda: hip.column_affine(x, x.clone(), a, b[:7]), lambda: hip.column_affine(x, x[:1].clone(), a, b),
                lambda: hip.column_affine(x, x.clone(), a, b, cols=(4, 5)), lambda: hip.column_affine(x, x.clone(), None, b),
                lambda: hip.column_affine(x, x.clone(), a, b, mode=2), lambda: hip.column_affine(x.view(2, 24), x.clone(), a, b)):
        with pytest.raises(hip.HipError):
            bad()
