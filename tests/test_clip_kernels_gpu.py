"""The three kernels of csrc/clip.hip on the GPU against tests/clip_restatement.py.  Every comparison of eps is bit for bit
over the whole pitched buffer, pad columns included; ib_column_range is exact against amin / amax.  -m gpu.

ib_x0_clip_range: row widths that are and are not a multiple of the vector, pad columns, a mask that straddles a vector, a
ragged mask, an unbounded column inside a vector, the step from the device counter, a buffer off 16-byte alignment.
ib_x0_clip_dynamic: the edges of the radix select (counts around the workgroup size, ranks at both ends, equal keys,
duplicates astride the rank, keys that differ in their lowest byte only, -0), one scale per window, more windows than
workgroups."""
import numpy as np
import pytest
import torch

from tests import clip_restatement as CR

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
DTYPES = [torch.float32, BF]
INF = float("inf")


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from inferbiomechanics_amd import hip as h
    h.lib()
    return h


@pytest.fixture(scope="module")
def coef():
    """x0_coefficients of a 10-step loop, cast once: (host float32 numpy, device tensor)"""
    from inferbiomechanics_amd.diffusion.schedule import x0_coefficients
    c = x0_coefficients(1000, 10).to(torch.float32).contiguous()
    return c.numpy(), c.to(DEV)


def rnd(shape, seed, dtype, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).to(dtype)


def bits(v):
    return v.contiguous().view(torch.int16 if v.dtype == BF else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a.cpu()), bits(b.cpu()))


def dev32(v):
    return torch.as_tensor(np.asarray(v, dtype=np.float32)).to(DEV)


def bounds(D):
    """per-column bounds with column 1 unbounded (inside the first vector) and, from D = 12 on, column 9 with lo == hi"""
    c = np.arange(D)
    lo = (-0.3 - 0.1 * (c % 3)).astype(np.float32)
    hi = (0.4 + 0.05 * (c % 4)).astype(np.float32)
    lo[1], hi[1] = -INF, INF
    if D >= 12:
        lo[9] = hi[9] = np.float32(0.25)
    return lo, hi


def masks(kind, T, D, ld):
    if kind == "none":
        return None
    m = torch.zeros(T, ld, dtype=torch.uint8)
    if kind == "cols":
        m[:, :3] = 1                                                   # straddles a vector of 8
    else:
        g = torch.Generator().manual_seed(11)
        m[:, :D] = (torch.rand(T, D, generator=g) < 0.4).to(torch.uint8)
    return m


def pitched(B, T, D, ld, seed, dtype, scale=1.0):
    """[B, T, ld] with random feature columns and a sentinel in the pad"""
    v = torch.full((B, T, ld), 7.0, dtype=dtype)
    v[:, :, :D] = rnd((B, T, D), seed, dtype, scale)
    return v


# ---------------------------------------------------------------------------------------------------------------------
# ib_x0_clip_range
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["none", "cols", "ragged"])
@pytest.mark.parametrize("D,ld", [(5, 5), (12, 16), (16, 16), (30, 32)])
def test_range_is_the_restatement_and_leaves_the_rest(hip, coef, D, ld, kind, dtype):
    ch, cd = coef
    lo, hi = bounds(D)
    for B in (1, 3):
        for T in (1, 7):
            x, eps, mask = pitched(B, T, D, ld, 1, dtype), pitched(B, T, D, ld, 2, dtype), masks(kind, T, D, ld)
            want, changed = CR.clip_range(x, eps, mask, lo, hi, ch[8], D)
            got = eps.clone().to(DEV)
            hip.x0_clip_range(x.to(DEV), got, None if mask is None else mask.to(DEV), dev32(lo), dev32(hi), cd, step=8, D=D)
            torch.cuda.synchronize()
            assert same_bits(got, want), (B, T)
            # what the launch may not touch, against the copy taken before it: inside the bounds, observed, unbounded, pad
            keep = torch.from_numpy(~changed)
            assert torch.equal(bits(got.cpu())[keep], bits(eps)[keep])
            assert not changed[:, :, D:].any() and not changed[:, :, 1].any()
            if mask is not None:
                assert not changed[:, mask.numpy() != 0].any()
            if B * T * D >= 100:
                act = CR.active(mask, lo, hi, T, D, ld)[None].repeat(B, 0)
                assert changed.any() and (act & ~changed).any(), "both a clipped and an inside element are needed"


@pytest.mark.parametrize("dtype", DTYPES)
def test_range_reads_the_step_from_the_device_counter(hip, coef, dtype):
    ch, cd = coef
    B, T, D, ld = 3, 7, 12, 16
    lo, hi = bounds(D)
    x, eps = pitched(B, T, D, ld, 3, dtype), pitched(B, T, D, ld, 4, dtype)
    ctr = torch.tensor([6], dtype=torch.int32, device=DEV)
    got = eps.clone().to(DEV)
    hip.x0_clip_range(x.to(DEV), got, None, dev32(lo), dev32(hi), cd, step=2, step_dev=ctr, D=D)
    assert same_bits(got, CR.clip_range(x, eps, None, lo, hi, ch[6], D)[0]), "the counter's row, not `step`'s"
    assert not same_bits(got, CR.clip_range(x, eps, None, lo, hi, ch[2], D)[0])
    ctr.fill_(99)                                                      # past the table: clamped to its last row
    got = eps.clone().to(DEV)
    hip.x0_clip_range(x.to(DEV), got, None, dev32(lo), dev32(hi), cd, step_dev=ctr, D=D)
    assert same_bits(got, CR.clip_range(x, eps, None, lo, hi, ch[9], D)[0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_range_off_alignment_takes_the_scalar_path_to_the_same_bits(hip, coef, dtype):
    ch, cd = coef
    B, T, D, ld = 3, 7, 12, 16
    lo, hi = bounds(D)
    x, eps, mask = pitched(B, T, D, ld, 5, dtype), pitched(B, T, D, ld, 6, dtype), masks("cols", T, D, ld)
    want, _ = CR.clip_range(x, eps, mask, lo, hi, ch[1], D)
    n = B * T * ld

    def shifted(v):                                                    # the same values one element off the allocation's start
        buf = torch.zeros(n + 8, dtype=dtype, device=DEV)
        buf[1:n + 1] = v.reshape(-1).to(DEV)
        view = buf[1:n + 1].view(B, T, ld)
        assert view.data_ptr() % 16 != 0 and view.is_contiguous()
        return view

    got = shifted(eps)
    hip.x0_clip_range(shifted(x), got, mask.to(DEV), dev32(lo), dev32(hi), cd, step=1, D=D)
    assert same_bits(got, want)
    aligned = eps.clone().to(DEV)
    hip.x0_clip_range(x.to(DEV), aligned, mask.to(DEV), dev32(lo), dev32(hi), cd, step=1, D=D)
    assert same_bits(aligned, want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,ld", [(5, 5), (30, 32)])
def test_infinite_bounds_change_nothing(hip, coef, D, ld, dtype):
    from inferbiomechanics_amd.diffusion.schedule import clip_tables
    _, cd = coef
    B, T = 3, 7
    lo, hi = np.full(D, -INF, np.float32), np.full(D, INF, np.float32)
    m, h, ih, flags = clip_tables(lo, hi)
    assert not flags.any()
    x, eps = pitched(B, T, D, ld, 7, dtype, 5.0), pitched(B, T, D, ld, 8, dtype, 5.0)
    got = eps.clone().to(DEV)
    hip.x0_clip_range(x.to(DEV), got, None, dev32(lo), dev32(hi), cd, step=0, D=D)
    assert same_bits(got, eps)
    hip.x0_clip_dynamic(x.to(DEV), got, None, dev32(lo), dev32(hi), cd, dev32(m), dev32(h), dev32(ih), 1, step=0, D=D)
    assert same_bits(got, eps)


# ---------------------------------------------------------------------------------------------------------------------
# ib_x0_clip_dynamic
# ---------------------------------------------------------------------------------------------------------------------
def unit_tables(D, lo=-1.0, hi=1.0):
    from inferbiomechanics_amd.diffusion.schedule import clip_tables
    lo, hi = np.full(D, lo, np.float32), np.full(D, hi, np.float32)
    m, h, ih, _ = clip_tables(lo, hi)
    return lo, hi, m.numpy().astype(np.float32), h.numpy().astype(np.float32), ih.numpy().astype(np.float32)


def run_dynamic(hip, x, eps, mask, tabs, k, row, D):
    """launch over a one-row table `row` and compare with the restatement -> (got, changed, sw)"""
    lo, hi, m, h, ih = tabs
    want, changed, sw = CR.clip_dynamic(x, eps, mask, lo, hi, m, h, ih, k, row, D)
    got = eps.clone().to(DEV)
    hip.x0_clip_dynamic(x.to(DEV), got, None if mask is None else mask.to(DEV), dev32(lo), dev32(hi),
                        dev32(np.asarray(row, np.float32).reshape(1, 4)), dev32(m), dev32(h), dev32(ih), k, D=D)
    torch.cuda.synchronize()
    assert same_bits(got, want)
    keep = torch.from_numpy(~changed)
    assert torch.equal(bits(got.cpu())[keep], bits(eps)[keep])
    return got, changed, sw


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,D,ld", [(1, 1, 8), (1, 255, 256), (1, 256, 256), (1, 257, 264), (10, 300, 304)])
def test_dynamic_counts_around_the_workgroup_and_ranks_at_both_ends(hip, coef, T, D, ld, dtype):
    ch, _ = coef
    tabs, n = unit_tables(D, -1.0, 2.0), T * D
    x, eps = pitched(2, T, D, ld, 21, dtype, 3.0), pitched(2, T, D, ld, 22, dtype)
    seen = set()
    for k in sorted({1, (n + 1) // 2, n}):
        _, changed, sw = run_dynamic(hip, x, eps, None, tabs, k, ch[4], D)
        seen.update(bool(s > 1.0) for s in sw)
        if k == n:
            assert (sw > 1.0).all(), "the largest |u| of these inputs lies outside"
    if n > 1:
        assert seen == {True, False}, "k = 1 selects a |u| below 1 (sw == 1), k = n one above (sw > 1)"


@pytest.mark.parametrize("dtype", DTYPES)
def test_dynamic_masked_window_with_an_unbounded_column(hip, coef, dtype):
    ch, _ = coef
    T, D, ld = 7, 30, 32
    lo, hi = bounds(D)
    from inferbiomechanics_amd.diffusion.schedule import clip_rank, clip_tables
    m, h, ih, _ = clip_tables(lo, hi)
    tabs = (lo, hi) + tuple(v.numpy().astype(np.float32) for v in (m, h, ih))
    x, eps = pitched(3, T, D, ld, 23, dtype, 2.0), pitched(3, T, D, ld, 24, dtype)
    for kind in ("cols", "ragged"):
        mask = masks(kind, T, D, ld)
        n = int(CR.active(mask, lo, hi, T, D, ld).sum())
        _, changed, sw = run_dynamic(hip, x, eps, mask, tabs, clip_rank(0.9, n), ch[2], D)
        assert changed.any() and not changed[:, :, 1].any() and not changed[:, :, 9].any() and not changed[:, :, D:].any()
        assert not changed[:, mask.numpy() != 0].any()


ONE = (1.0, 0.0, 1.0, 1.0)                                             # x0 = x exactly; with (lo, hi) = (-1, 1), u = x


@pytest.mark.parametrize("dtype", DTYPES)
def test_dynamic_equal_keys_duplicates_centre_and_negative_zero(hip, dtype):
    T, D, ld = 2, 300, 304
    n, tabs = T * D, unit_tables(D)
    eps = pitched(1, T, D, ld, 25, dtype)
    # every |u| equal, signs mixed: q is that value at every rank
    x = torch.full((1, T, ld), 1.5, dtype=dtype)
    x[:, :, ::2] = -1.5
    for k in (1, n // 2, n):
        _, changed, sw = run_dynamic(hip, x, eps, None, tabs, k, ONE, D)
        assert sw[0] == np.float32(1.5) and changed[:, :, :D].all()
    # duplicates astride rank k: 200 values of 0.5, 200 of 2.5, 200 of 3.0 -> ranks 201 .. 400 are all 2.5
    x = torch.full((1, T, ld), 0.5, dtype=dtype)
    flat = x.view(-1)
    cols = torch.arange(T * ld).view(T, ld)[:, :D].reshape(-1)
    perm = cols[torch.randperm(n, generator=torch.Generator().manual_seed(3))]
    flat[perm[200:400]] = 2.5
    flat[perm[400:]] = -3.0
    for k, q in ((200, 1.0), (201, 2.5), (300, 2.5), (400, 2.5), (401, 3.0)):
        _, changed, sw = run_dynamic(hip, x, eps, None, tabs, k, ONE, D)
        assert sw[0] == np.float32(q), k
    # every x0 exactly at the centre, +0 and -0 mixed: q = 0, sw = 1, nothing is written
    x = torch.zeros((1, T, ld), dtype=dtype)
    x[:, :, 1::3] = -0.0
    assert bool(torch.signbit(x).any())
    for k in (1, n):
        got, changed, sw = run_dynamic(hip, x, eps, None, tabs, k, ONE, D)
        assert sw[0] == 1.0 and not changed.any() and same_bits(got, eps)
    # -0 among values on both sides of 1: it keys as 0, the smallest
    x = pitched(1, T, D, ld, 26, dtype, 2.0)
    x[:, 0, :7] = -0.0
    for k in (1, 7, 8, n - 1):
        _, _, sw = run_dynamic(hip, x, eps, None, tabs, k, ONE, D)
    assert sw[0] > 1.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_dynamic_keys_that_differ_in_the_lowest_byte_only(hip, dtype):
    """x = 2, e = j in 1 .. 255 (exact in bf16), sa = 2^-23: x0 = 2 - j ulp, so the keys 0x3FFFFFxx share their three high
    bytes and only the fourth pass separates them"""
    T, D, ld = 1, 255, 256
    tabs = unit_tables(D)
    row = (1.0, 2.0 ** -23, 1.0, 1.0)
    x = torch.full((1, T, ld), 2.0, dtype=dtype)
    eps = torch.zeros((1, T, ld), dtype=dtype)
    j = torch.randperm(255, generator=torch.Generator().manual_seed(5)) + 1
    eps[0, 0, :D] = j.to(dtype)
    x0 = CR.predicted_x0(row, CR.widen(x), CR.widen(eps))[0, 0, :D]
    keys = x0.view(np.uint32)
    assert len(set(keys.tolist())) == 255 and set((keys >> 8).tolist()) == {0x3FFFFF}
    for k in (1, 2, 100, 254, 255):
        _, changed, sw = run_dynamic(hip, x, eps, None, tabs, k, row, D)
        assert sw[0] == np.sort(x0)[k - 1] and sw[0] > 1.0 and changed[:, :, :D].any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_dynamic_every_window_gets_its_own_scale(hip, coef, dtype):
    ch, _ = coef
    T, D, ld = 7, 12, 16
    tabs = unit_tables(D)
    x, eps = pitched(3, T, D, ld, 27, dtype), pitched(3, T, D, ld, 28, dtype)
    x[0] *= 0.01
    eps[0] *= 0.01
    x[2] *= 100.0
    _, changed, sw = run_dynamic(hip, x, eps, None, tabs, 80, ch[5], D)
    assert sw[0] == 1.0 and sw[1] > 1.0 and sw[2] > 10.0 * sw[1]
    assert not changed[0].any() and changed[1].any() and changed[2].any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_dynamic_more_windows_than_workgroups(hip, coef, dtype):
    """600 windows of 5 elements: a workgroup takes a second window, whose histogram must start empty"""
    ch, _ = coef
    B, T, D, ld = 600, 1, 5, 8
    tabs = unit_tables(D)
    x, eps = pitched(B, T, D, ld, 29, dtype, 2.0), pitched(B, T, D, ld, 30, dtype)
    x[::3] *= 0.1
    eps[::3] *= 0.1
    for k in (1, 3, 5):
        _, changed, sw = run_dynamic(hip, x, eps, None, tabs, k, ch[8], D)
        if k == 3:
            assert (sw > 1.0).any() and (sw == 1.0).any() and len(set(sw.tolist())) > 100


# ---------------------------------------------------------------------------------------------------------------------
# ib_column_range
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,T,D", [(1, 1, 5), (3, 7, 5), (257, 2, 30), (40, 50, 300)])
def test_column_range_is_amin_amax_without_the_pad(hip, N, T, D, dtype):
    per = T * D
    pitch = (per + 7) // 8 * 8 + 8                                     # always some pad
    table = torch.full((N, pitch), 1.0e6, dtype=dtype)                 # the pad would be every column's maximum
    v = rnd((N * T, D), 31, dtype, 3.0)
    v[0, 0], v[-1, 0] = 0.0, -0.0                                      # +-0 in a column ...
    v[:, 1] = -v[:, 1].abs() - 1.0                                     # ... an all-negative one ...
    if D > 2:
        v[:, 2] = 0.0                                                  # ... and one of zeros of both signs
        v[::2, 2] = -0.0
    table[:, :per] = v.view(N, per)
    got = hip.column_range(table.to(DEV), T, D)
    torch.cuda.synchronize()
    want = CR.column_range(table, T, D)
    assert got.dtype == torch.float32 and tuple(got.shape) == (D, 2)
    assert torch.equal(got.cpu(), want)                                # exact; -0 == +0
    assert float(got.max()) < 1.0e6 and float(got[1, 1]) <= -1.0


# ---------------------------------------------------------------------------------------------------------------------
# refusals: nothing is launched
# ---------------------------------------------------------------------------------------------------------------------
def test_refusal_codes(hip):
    lib = hip.lib()
    E_ARG, E_DTYPE = -1, -2                                            # include/ib_hip.h
    z = torch.zeros(64, device=DEV)
    p, zb = z.data_ptr(), torch.zeros(64, dtype=torch.uint8, device=DEV).data_ptr()
    ok_range = [p, p, zb, p, p, p, 4, 0, None, 1, 2, 4, 8, 0, None]
    assert lib.ib_x0_clip_range(*ok_range) == 0
    for i, bad in ((0, None), (1, None), (3, None), (4, None), (5, None), (6, 0), (9, 0), (10, 0), (11, 0), (12, 3)):
        a = list(ok_range)
        a[i] = bad
        assert lib.ib_x0_clip_range(*a) == E_ARG, i
    a = list(ok_range)
    a[13] = 77
    assert lib.ib_x0_clip_range(*a) == E_DTYPE
    ok_dyn = [p, p, zb, p, p, p, 4, 0, None, p, p, p, 8, 1, 2, 4, 8, 0, None]
    assert lib.ib_x0_clip_dynamic(*ok_dyn) == 0
    for i, bad in ((0, None), (1, None), (9, None), (10, None), (11, None), (12, 0), (12, 9), (13, 0), (16, 3)):
        a = list(ok_dyn)
        a[i] = bad
        assert lib.ib_x0_clip_dynamic(*a) == E_ARG, i
    a = list(ok_dyn)
    a[17] = 77
    assert lib.ib_x0_clip_dynamic(*a) == E_DTYPE
    ok_col = [p, 2, 2, 4, 8, p, 1, p, 0, None]
    out = torch.zeros(8, device=DEV)
    ok_col[7] = out.data_ptr()
    part = torch.zeros(8, device=DEV)
    ok_col[5] = part.data_ptr()
    assert lib.ib_column_range(*ok_col) == 0
    for i, bad in ((0, None), (5, None), (7, None), (1, 0), (2, 0), (3, 0), (4, 7), (6, 0)):
        a = list(ok_col)
        a[i] = bad
        assert lib.ib_column_range(*a) == E_ARG, i
    a = list(ok_col)
    a[8] = 77
    assert lib.ib_column_range(*a) == E_DTYPE
    torch.cuda.synchronize()
