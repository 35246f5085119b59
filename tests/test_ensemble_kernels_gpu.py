"""ib_ensemble_order on the GPU (csrc/ensemble.hip) against tests/ensemble_restatement.py.  -m gpu.

The kernel must equal the restatement as numbers (==, not bits: -0 and +0 may sort in either order); rank and inside exactly.
K runs over every padded size of the sorting network and its edge, both dtypes, and the shapes where the indexing can go
wrong: an unaligned window that ends at the last column, the full row, one element, 257 elements (just past one block) and
one launch past the grid's cap (2048 blocks of 256 lanes), where a lane takes a second element."""
import numpy as np
import pytest
import torch

from tests import ensemble_restatement as ER

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
KS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64]
# (B, rows, ld, c0, w)
SHAPES = [(2, 3, 11, 6, 5), (2, 3, 16, 0, 16), (1, 1, 1, 0, 1), (1, 1, 260, 2, 257)]
SENTINEL = 77.0


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from inferbiomechanics_amd import hip
    hip.lib()


def positions(L, K):
    from inferbiomechanics_amd.diffusion.ensemble import interval_levels, quantile_position
    return [quantile_position(q, K) for q in interval_levels(L)]


def same(got, want, what):
    g, w = got.detach().cpu().numpy().reshape(-1), np.asarray(want).reshape(-1)
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.dtype, w.dtype)
    bad = np.flatnonzero(~(g == w))
    assert bad.size == 0, (what, bad[:5].tolist(), g[bad[:5]].tolist(), w[bad[:5]].tolist())


def check(hip, x, cols, L, y):
    """one scored and one unscored launch over x against the restatement; x is left as it was"""
    B, K, rows, ld = x.shape
    before = x.clone()
    m = ER.members_of(x, *cols)
    want = ER.restate(m, positions(L, K), None if y is None else y.cpu().numpy().reshape(-1))
    got = hip.ensemble_order(x, cols, L, y)
    torch.cuda.synchronize()
    assert torch.equal(x.view(torch.int16 if x.dtype == BF else torch.int32),
                       before.view(torch.int16 if x.dtype == BF else torch.int32)), "x is only read"
    for k in ("lo", "median", "hi"):
        assert tuple(got[k].shape) == (B, rows, cols[1])
        same(got[k], want[k], k)
    if y is not None:
        same(got["crps"], want["crps"], "crps")
        same(got["rank"], want["rank"], "rank")
        same(got["inside"], want["inside"], "inside")
        assert int(got["rank"].max()) <= K
        alone = hip.ensemble_order(x, cols, L)
        assert sorted(alone) == ["hi", "lo", "median"]
        for k in alone:
            assert torch.equal(alone[k], got[k]), (k, "the quantiles do not depend on the score")
    return got, want


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("K", KS)
def test_against_the_restatement(K, dtype):
    from inferbiomechanics_amd import hip
    g = torch.Generator().manual_seed(1000 + K)
    for B, rows, ld, c0, w in SHAPES:
        x = (torch.randn(B, K, rows, ld, generator=g) * 3).to(dtype).to(DEV)
        y = (torch.randn(B, rows, w, generator=g) * 3).to(DEV)
        for L in (0.8, 0.5):
            check(hip, x, (c0, w), L, y)


def value_cases(K, dtype, g):
    """members [K, n] and truths [n]: one column per case, in the storage dtype's values"""
    r = lambda n, scale=1.0: (torch.randn(n, generator=g) * scale).to(dtype).float()
    cols, ys = [], []
    add = lambda m, y: (cols.append(m), ys.append(float(y)))
    add(torch.full((K,), 1.25), 1.25)                                  # all members equal, the truth on them
    add(torch.full((K,), -2.5), 0.0)                                   # all equal, the truth beside them
    rep = torch.randint(-2, 3, (K,), generator=g).float()
    add(rep, 1.0)                                                      # repeated values, the truth (likely) among them
    add(rep, 0.5)
    m = r(K)
    add(m, m[K // 2])                                                  # the truth equal to a member
    add(m, m.min() - 1.0)                                              # below all: rank 0
    add(m, m.max() + 1.0)                                              # above all: rank K
    add(m, m.min())                                                    # on the smallest: rank 0, a tie is not less
    add(m, m.max())
    signs = torch.arange(K).float() - (K - 1) / 2                      # both signs (and 0 at odd K)
    add(signs, 0.0)
    add(torch.cat([torch.zeros(1), -torch.zeros(1), signs])[:K] if K > 2 else signs, 0.0)   # +0 and -0 among the members
    s = m.sort().values
    add(s, 0.1)                                                        # already sorted
    add(s.flip(0), 0.1)                                                # reversed
    add(r(K, 1e-3), 1e-4)
    add(r(K, 1e3), -10.0)
    return torch.stack(cols, dim=1).contiguous(), torch.tensor(ys, dtype=torch.float32)


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("K", KS)
def test_value_cases(K, dtype):
    from inferbiomechanics_amd import hip
    m, y = value_cases(K, dtype, torch.Generator().manual_seed(50 + K))
    n = m.shape[1]
    x = m.view(1, K, 1, n).to(dtype).to(DEV)
    assert torch.equal(x.float().cpu().view(K, n), m), "the cases are exact in the storage dtype"
    got, want = check(hip, x, (0, n), 0.8, y.view(1, 1, n).to(DEV))
    rank = got["rank"].view(-1).tolist()
    assert rank[0] == 0 and rank[1] == K and rank[5] == 0 and rank[6] == K and rank[7] == 0
    inside = got["inside"].view(-1).tolist()
    assert inside[0] == 1 and inside[1] == 0 and inside[5] == 0 and inside[6] == 0
    crps = got["crps"].view(-1).tolist()
    assert crps[0] == 0.0 and crps[1] == 2.5, "a point mass scores its distance"
    for k in ("lo", "median", "hi"):
        assert got[k].view(-1)[0] == 1.25 and got[k].view(-1)[1] == -2.5
    # sorted and reversed members are the same ensemble
    for k in got:
        assert got[k].view(-1)[11] == got[k].view(-1)[12], k


def test_outputs_are_written_inside_their_bounds_only():
    """the C-ABI call itself, every output a slice of a larger buffer of sentinels"""
    from inferbiomechanics_amd import hip
    B, K, rows, ld, c0, w = 2, 5, 3, 11, 6, 5
    n, pad = B * rows * w, 64
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, K, rows, ld, generator=g).to(BF).to(DEV)
    y = torch.randn(n, generator=g).to(DEV)
    fbuf = [torch.full((n + 2 * pad,), SENTINEL, device=DEV) for _ in range(4)]
    bbuf = [torch.full((n + 2 * pad,), 200, dtype=torch.uint8, device=DEV) for _ in range(2)]
    pos = positions(0.8, K)
    ptr = lambda t: t[pad:pad + n].data_ptr()
    rc = hip.lib().ib_ensemble_order(x.data_ptr(), y.data_ptr(), ptr(fbuf[0]), ptr(fbuf[1]), ptr(fbuf[2]), ptr(fbuf[3]),
                                     ptr(bbuf[0]), ptr(bbuf[1]), B, K, rows, ld, c0, w, pos[0][0], pos[0][1], pos[1][0],
                                     pos[1][1], pos[2][0], pos[2][1], hip.BF16, hip.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    want = ER.restate(ER.members_of(x, c0, w), pos, y.cpu().numpy())
    for t, k in zip(fbuf + bbuf, ("lo", "median", "hi", "crps", "rank", "inside")):
        fill = SENTINEL if t.dtype == torch.float32 else 200
        assert bool((t[:pad] == fill).all()) and bool((t[pad + n:] == fill).all()), (k, "written out of bounds")
        same(t[pad:pad + n], want[k], k)


def test_past_the_grid_cap_a_lane_takes_a_second_element():
    from inferbiomechanics_amd import hip
    B, K, rows, ld, c0, w = 3, 3, 700, 256, 3, 253                      # 531 300 elements > 2048 * 256
    assert B * rows * w > 2048 * 256
    g = torch.Generator().manual_seed(9)
    x = torch.randn(B, K, rows, ld, generator=g).to(BF).to(DEV)
    y = torch.randn(B, rows, w, generator=g).to(DEV)
    check(hip, x, (c0, w), 0.5, y)


def test_more_than_64_members_is_refused():
    from inferbiomechanics_amd import hip
    x = torch.zeros(1, 65, 2, 4, device=DEV)
    with pytest.raises(hip.HipError, match="at most 64"):
        hip.ensemble_order(x, (0, 4), 0.8)
    out = torch.full((3, 8), SENTINEL, device=DEV)
    rc = hip.lib().ib_ensemble_order(x.data_ptr(), None, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), None, None,
                                     None, 1, 65, 2, 4, 0, 4, 0, 0.0, 32, 0.0, 64, 0.0, hip.F32, hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -5 and bool((out == SENTINEL).all()), "IB_E_UNSUPPORTED, nothing launched"
