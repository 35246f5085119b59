"""Direct tests of the small entry points that were reached only through whole models or autograd functions:
ib_gather_rows_bwd (against ib_gather_rows), ib_sqdiff_mean / ib_sqdiff_mean_bwd, ib_scale_by_device_scalar and
ib_sum_partials.  Each against a float64 reference with a bound counted from the kernel's own roundings (u32 = 2^-24,
ub16 = 2^-8), or against an exact fp32 restatement on the CPU where the kernel's order is fixed.  -m gpu."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
U32, UB16 = 2.0 ** -24, 2.0 ** -8
SENT = 1536.0                          # exact in bf16 and fp32
DTYPES = [torch.float32, torch.bfloat16]


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from inferbiomechanics_amd import hip as h
    h.lib()
    return h


# ---- gather_rows_bwd ---------------------------------------------------------------------------------------------------
def _gather_idx(n, rows, g):
    """indices with repeats, values below 0 and at or above `rows`, and (rows >= 3) a middle row that is never hit"""
    idx = torch.randint(-2, rows + 2, (n,), generator=g)
    if n >= 2:
        idx[0], idx[-1] = -1, rows                                   # both out-of-range sides, whatever the draw
    if n >= 4:
        idx[1] = idx[2] = rows - 1                                   # a repeat
    if rows >= 3:
        idx[idx == rows // 2] = rows // 2 - 1
    return idx


@pytest.mark.parametrize("n,dim,rows", [(1, 1, 1), (7, 5, 3), (200, 36, 10), (50, 512, 50)])
def test_gather_rows_bwd(hip, n, dim, rows):
    g = torch.Generator().manual_seed(1000 * n + dim)
    idx = _gather_idx(n, rows, g) if n > 1 else torch.tensor([5])
    dout = torch.randn(n, dim, generator=g)
    cl = idx.clamp(0, rows - 1)
    hits = torch.bincount(cl, minlength=rows)
    if rows >= 3:
        assert hits[rows // 2] == 0 and hits.max() >= 2 and (idx < 0).any() and (idx >= rows).any()
    dtable = torch.full((rows, dim), float("nan"), device=DEV)
    hip.gather_rows_bwd(dout.to(DEV), idx.to(DEV), dtable)
    again = torch.full((rows, dim), -7.0, device=DEV)
    hip.gather_rows_bwd(dout.to(DEV), idx.to(DEV), again)
    got = dtable.cpu()
    assert torch.equal(got, again.cpu()), "depends on what dtable held before"
    # float64 reference; hits_r additions of fp32 terms, each rounding once on a partial sum within the absolute sum
    ref = torch.zeros(rows, dim, dtype=torch.float64).index_add_(0, cl, dout.double())
    mag = torch.zeros(rows, dim, dtype=torch.float64).index_add_(0, cl, dout.double().abs())
    bound = (hits.double()[:, None] + 1) * U32 * mag
    assert torch.isfinite(got).all() and ((got.double() - ref).abs() <= bound).all()
    # exactly the fp32 sum in position order
    seq = torch.zeros(rows, dim)
    for i in range(n):
        seq[cl[i]] += dout[i]
    assert torch.equal(got, seq)
    assert (got[hits == 0] == 0).all()
    # the forward clamps the same way: out[i] = table[clamp(idx[i])], so the two are adjoint on out-of-range indices too
    table = torch.randn(rows, dim, generator=g)
    out = torch.full((n, dim), float("nan"), device=DEV)
    hip.gather_rows(table.to(DEV), idx.to(DEV), out)
    assert torch.equal(out.cpu(), table[cl])
    lhs, rhs = (out.cpu().double() * dout.double()).sum(), (table.double() * got.double()).sum()
    assert abs(float(lhs - rhs)) <= (n + 2) * U32 * float((table[cl].double() * dout.double()).abs().sum())


# ---- sqdiff_mean / sqdiff_mean_bwd -------------------------------------------------------------------------------------
SQ_SHAPES = [(1, 1, 6), (3, 5, 12), (37, 7, 5), (300, 1, 6)]


def _sq_inputs(shape, dtype):
    g = torch.Generator().manual_seed(shape[0] * 131 + shape[2])
    o = (3 * torch.randn(*shape, generator=g, dtype=torch.float64) + 1).to(dtype)
    l = (3 * torch.randn(*shape, generator=g, dtype=torch.float64)).to(dtype)
    dout = (torch.randn(shape[2], generator=g, dtype=torch.float64) + 0.5 * torch.arange(shape[2]) - 1).float()
    return o, l, dout


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SQ_SHAPES)
def test_sqdiff_mean(hip, shape, dtype):
    o, l, dout = _sq_inputs(shape, dtype)
    rows = shape[0] * shape[1]
    got = hip.sqdiff_mean(o.to(DEV), l.to(DEV))
    assert got.dtype == torch.float32 and got.shape == (shape[2],)
    d2 = ((o.double() - l.double()) ** 2).reshape(rows, shape[2])
    # a thread adds ceil(rows / 256) terms, the tree 8 more; the difference, the square and the division round
    bound = (-(-rows // 256) + 9) * U32 * d2.sum(0) / rows
    err = (got.cpu().double() - d2.mean(0)).abs()
    assert torch.isfinite(got).all() and (err <= bound).all(), (err / bound).max()
    assert torch.equal(got, hip.sqdiff_mean(o.to(DEV), l.to(DEV)))

    oo = o.double().requires_grad_(True)
    (torch.mean((oo - l.double()) ** 2, dim=(0, 1)) * dout.double()).sum().backward()
    g = hip.sqdiff_mean_bwd(o.to(DEV), l.to(DEV), dout.to(DEV))
    assert g.dtype == dtype and g.shape == o.shape
    u_store = U32 if dtype == torch.float32 else UB16
    err = (g.cpu().double() - oo.grad).abs()
    assert torch.isfinite(g).all() and (err <= 4 * u_store * oo.grad.abs()).all(), (err / oo.grad.abs()).max() / u_store


@pytest.mark.parametrize("dtype", DTYPES)
def test_squared_diff_mean_vector_label_gradient_is_the_negation(hip, dtype):
    from inferbiomechanics_amd.loss.RegressionLossEvaluator import RegressionLossEvaluator as E
    o, l, dout = _sq_inputs((37, 7, 5), dtype)
    od, ld = o.to(DEV).requires_grad_(True), l.to(DEV).requires_grad_(True)
    with hip.record_launches() as rec:
        out = E.get_squared_diff_mean_vector(od, ld)
        (out.float() * dout.to(DEV)).sum().backward()
    assert [n for n, _ in rec.calls] == ["ib_sqdiff_mean", "ib_sqdiff_mean_bwd"]
    assert od.grad.abs().max() > 0 and torch.equal(ld.grad, -od.grad)
    # and it IS the kernel's gradient for the upstream gradient autograd handed over
    up = dout.to(DEV).to(dtype).float()                              # d / d out passes through out's dtype
    assert torch.equal(od.grad, hip.sqdiff_mean_bwd(od.detach(), ld.detach(), up))


# ---- scale_by_device_scalar --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 3, 4, 5, 7, 8, 9, 2051])             # around the 16-byte body (4 fp32 / 8 bf16) and its tail
def test_scale_by_device_scalar(hip, n, dtype):
    g = torch.Generator().manual_seed(n)
    y = (4 * torch.randn(n, generator=g, dtype=torch.float64)).to(dtype)
    s = torch.tensor([-0.3], dtype=torch.float32)                    # not a power of two: every product rounds
    buf = torch.full((n + 16,), SENT, dtype=dtype, device=DEV)
    buf[:n] = y.to(DEV)
    ret = hip.scale_by_device_scalar(buf[:n], s.to(DEV))
    assert ret.data_ptr() == buf.data_ptr()
    want = (y.float() * s).to(dtype)                                 # fp32 product, one rounding to the storage dtype
    assert torch.equal(buf[:n].cpu(), want)
    assert (buf[n:] == SENT).all(), "wrote past n"


@pytest.mark.parametrize("dtype", DTYPES)
def test_scale_by_device_scalar_accepts_nothing_to_do(hip, dtype):
    s = torch.tensor([-0.3], device=DEV)
    buf = torch.full((16,), SENT, dtype=dtype, device=DEV)
    hip.scale_by_device_scalar(buf[:0], s)                           # n == 0 at a real address
    assert hip.lib().ib_scale_by_device_scalar(buf.data_ptr(), s.data_ptr(), 0, hip.dtype_code(dtype), hip.stream_ptr()) == 0
    empty = torch.empty(0, dtype=dtype, device=DEV)                  # n == 0 with no allocation behind it
    assert hip.scale_by_device_scalar(empty, s) is empty
    torch.cuda.synchronize()
    assert (buf == SENT).all()


# ---- sum_partials ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parts", [1, 63, 64, 65, 256, 257, 1137])
def test_sum_partials(hip, parts):
    g = torch.Generator().manual_seed(parts)
    x = torch.randn(parts, generator=g) * torch.logspace(-2, 2, parts)[torch.randperm(parts, generator=g)]
    assert parts == 1 or ((x > 0).any() and (x < 0).any())
    scale = -0.37
    buf = torch.full((parts + 64,), float("nan"), device=DEV)        # a read past `parts` poisons the sum
    buf[:parts] = x.to(DEV)
    out = torch.full((3,), SENT, device=DEV)
    hip.sum_partials(buf, parts, scale, out[1:2])
    got = out.cpu()
    assert got[0] == SENT and got[2] == SENT and torch.isfinite(got[1])
    s32 = float(torch.tensor(scale, dtype=torch.float32))            # the scale the kernel receives
    ref = float(x.double().sum()) * s32
    # ceil(parts / 256) additions in a thread, 6 across the wave, 3 across the waves, the product with scale
    bound = (-(-parts // 256) + 10) * U32 * float(x.double().abs().sum()) * abs(s32)
    assert abs(float(got[1]) - ref) <= bound, (float(got[1]), ref, bound)
    out2 = torch.full((1,), SENT, device=DEV)
    hip.sum_partials(buf[:parts], parts, scale, out2)
    assert torch.equal(out2.cpu(), got[1:2]), "not bitwise repeatable"
    with pytest.raises(hip.HipError):
        hip.sum_partials(buf[:parts], parts + 1, scale, out2)
