"""The three kernels of classifier-free guidance (csrc/cfg.hip) on the GPU, bit for bit against tests/cfg_restatement.py:
ib_q_sample_cond_drop (free columns ib_q_sample_cond's, conditioning columns x0's or +0 by a per-window Philox decision that
depends on (seed, step, stream id, window) alone), ib_cfg_combine (ec + s (ec - eu), three fp32 roundings, first half only)
and ib_cfg_mirror (a copy of the free columns and the timesteps, nothing else written).

Shapes (B, T, D, C, ld): (3, 5, 44, 14, 48) -- C splits a vector of 4 and of 8, the row pitch is padded -- and
(1, 2, 300, 270, 304), the trainer's row with the vector 268 .. 271 astride C.  -m gpu."""
import numpy as np
import pytest
import torch

from tests import cfg_restatement as CR

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
SHAPES = [(3, 5, 44, 14, 48), (1, 2, 300, 270, 304)]
DTYPES = [torch.float32, BF]
STREAM = 5


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from inferbiomechanics_amd import hip as h
    h.lib()
    return h


@pytest.fixture(scope="module")
def tabs(hip):
    from inferbiomechanics_amd.diffusion.schedule import DiffusionTables
    return DiffusionTables(DEV)


def rnd(shape, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64).to(dtype)


def bits(v):
    return v.contiguous().view(torch.int16 if v.dtype == BF else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a.cpu()), bits(b.cpu()))


SENT = 7.0


def noised(hip, tabs, B, T, D, C, ld, dtype, p, seed=3, step=0, step_dev=None, with_out=True):
    """(x_t of q_sample_cond, x_t of q_sample_cond_drop, both as the whole pitched buffers, x0, dropped_out)"""
    x0, eps = rnd((B, T, D), 1, dtype).to(DEV), rnd((B, T, D), 2, dtype).to(DEV)
    t = (torch.arange(B, device=DEV) * 331) % 1000
    ref = torch.full((B * T, ld), SENT, dtype=dtype, device=DEV)
    got = torch.full((B * T, ld), SENT, dtype=dtype, device=DEV)
    out = torch.full((B,), 9, dtype=torch.uint8, device=DEV) if with_out else None
    hip.q_sample_cond(x0, eps, t, tabs.sqrt_ab, tabs.sqrt_1mab, ref[:, :D], C)
    hip.q_sample_cond_drop(x0, eps, t, tabs.sqrt_ab, tabs.sqrt_1mab, got[:, :D], C, p, seed, step=step, step_dev=step_dev,
                           stream_id=STREAM, dropped_out=out)
    torch.cuda.synchronize()
    return ref, got, x0, out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T,D,C,ld", SHAPES)
def test_drop_p0_is_q_sample_cond_and_p1_zeroes_every_condition(hip, tabs, B, T, D, C, ld, dtype):
    ref, got, x0, out = noised(hip, tabs, B, T, D, C, ld, dtype, 0.0)
    assert same_bits(got, ref), "p = 0 must be ib_q_sample_cond bit for bit, pad columns untouched"
    assert out.tolist() == [0] * B
    ref, got, x0, out = noised(hip, tabs, B, T, D, C, ld, dtype, 1.0)
    assert out.tolist() == [1] * B
    assert same_bits(got[:, :C], torch.zeros_like(got[:, :C])), "a dropped window's conditioning columns are +0"
    assert same_bits(got[:, C:], ref[:, C:]), "free and pad columns are ib_q_sample_cond's"
    # without dropped_out: the same x_t
    _, got2, _, _ = noised(hip, tabs, B, T, D, C, ld, dtype, 1.0, with_out=False)
    assert same_bits(got2, got)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,D,C,ld", [s[1:] for s in SHAPES])
def test_drop_half_follows_the_restated_mask(hip, tabs, T, D, C, ld, dtype):
    B, p, step = 64, 0.5, 11
    seed = CR.seed_with_count(B, p, step, STREAM, 16, 48)
    mask = CR.drop_mask(B, p, seed, step, STREAM)
    assert 16 <= int(mask.sum()) <= 48, "a mask that drops nothing or everything would hide a failure"
    ref, got, x0, out = noised(hip, tabs, B, T, D, C, ld, dtype, p, seed=seed, step=step)
    assert np.array_equal(out.cpu().numpy(), mask)
    want = CR.q_sample_cond_drop(ref[:, :D].reshape(B, T, D), x0, mask, C)
    assert same_bits(got[:, :D].reshape(B, T, D), want)
    assert same_bits(got[:, D:], ref[:, D:]), "pad columns were touched"
    # the first 8 windows decide alike in a batch of 8: the decision does not depend on B
    ref8, got8, x08, out8 = noised(hip, tabs, 8, T, D, C, ld, dtype, p, seed=seed, step=step)
    assert np.array_equal(out8.cpu().numpy(), mask[:8])
    assert np.array_equal(CR.drop_mask(8, p, seed, step, STREAM), mask[:8])
    assert same_bits(got8[:, :D].reshape(8, T, D), CR.q_sample_cond_drop(ref8[:, :D].reshape(8, T, D), x08, mask[:8], C))
    # nor on the pitch or the vector width: ld = D + 1 is the element-wise kernel (its free columns are the element-wise
    # ib_q_sample_cond's, which rounds fp32 in another form than the 4-wide one)
    ref1, got1, x01, out1 = noised(hip, tabs, B, T, D, C, D + 1, dtype, p, seed=seed, step=step)
    assert np.array_equal(out1.cpu().numpy(), mask)
    assert same_bits(got1[:, :D].reshape(B, T, D), CR.q_sample_cond_drop(ref1[:, :D].reshape(B, T, D), x01, mask, C))
    assert same_bits(got1[:, D:], ref1[:, D:])


def test_drop_mask_reads_the_device_step_word(hip, tabs):
    B, T, D, C, ld, p = 64, 5, 44, 14, 48, 0.5
    seed = CR.seed_with_count(B, p, 4, STREAM, 16, 48)
    masks = []
    for dev_step in (1, 2):
        ctr = torch.tensor([dev_step], dtype=torch.int32, device=DEV)
        _, _, _, out = noised(hip, tabs, B, T, D, C, ld, BF, p, seed=seed, step=3, step_dev=ctr)
        want = CR.drop_mask(B, p, seed, 3 + dev_step, STREAM)          # the counter word is step + *step_dev
        assert np.array_equal(out.cpu().numpy(), want)
        masks.append(want)
    assert not np.array_equal(masks[0], masks[1])
    assert 16 <= int(masks[0].sum()) <= 48


def test_bad_arguments_are_refused_without_a_launch(hip, tabs):
    B, T, D, C = 4, 2, 8, 3
    x0, eps = rnd((B, T, D), 1, BF).to(DEV), rnd((B, T, D), 2, BF).to(DEV)
    t = torch.zeros(B, dtype=torch.int64, device=DEV)
    xt = torch.empty_like(x0)
    with pytest.raises(ValueError):
        hip.q_sample_cond_drop(x0, eps, t, tabs.sqrt_ab, tabs.sqrt_1mab, xt, C, 1.5, 1)
    with pytest.raises(hip.HipError):
        hip.q_sample_cond_drop(x0, eps, t, tabs.sqrt_ab, tabs.sqrt_1mab, xt, D, 0.5, 1)
    lib, p_ = hip.lib(), lambda a: a.data_ptr()
    args = [p_(x0), p_(eps), p_(t), p_(tabs.sqrt_ab), p_(tabs.sqrt_1mab), p_(xt), D, B, T, D, tabs.sqrt_ab.numel(), C, 1, 0,
            None, 0, (1 << 32) + 1, None, hip.BF16, hip.stream_ptr()]
    assert lib.ib_q_sample_cond_drop(*args) < 0, "a threshold above 2^32 is refused"
    args[16] = 1 << 31
    assert lib.ib_q_sample_cond_drop(*([None] + args[1:])) < 0, "a null x0 is refused"
    assert lib.ib_cfg_combine(None, 1.0, 1, 8, hip.BF16, hip.stream_ptr()) < 0
    assert lib.ib_cfg_combine(p_(xt), 1.0, 0, 8, hip.BF16, hip.stream_ptr()) < 0
    assert lib.ib_cfg_mirror(p_(xt), None, 1, 1, 8, 8, 3, hip.BF16, hip.stream_ptr()) < 0
    assert lib.ib_cfg_mirror(p_(xt), p_(t), 1, 1, 8, 8, 8, hip.BF16, hip.stream_ptr()) < 0, "cond_cols = D leaves nothing free"
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T,D,C,ld", SHAPES + [(3, 5, 44, 14, 45)])       # 3 * 5 * 45 elements: the element-wise kernel
def test_cfg_combine(hip, B, T, D, C, ld, dtype):
    eps0 = torch.zeros((2 * B, T, ld), dtype=dtype)
    eps0[:, :, :D] = rnd((2 * B, T, D), 4, dtype)
    for s in (0.0, 1.5, -0.5):
        eps = eps0.to(DEV)
        hip.cfg_combine(eps, s)
        torch.cuda.synchronize()
        want = CR.cfg_combine(eps0, s)
        assert same_bits(eps, want), f"s = {s}"
        assert same_bits(eps[B:], eps0[B:]), "the second half was written"
        assert same_bits(eps[:B, :, D:], torch.zeros_like(eps0[:B, :, D:])), "zero pad columns must stay +0"
        if s == 0.0:
            assert same_bits(eps[:B], eps0[:B]), "s = 0 leaves the conditional prediction as it is"
        else:
            assert not same_bits(eps[:B], eps0[:B])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T,D,C,ld", SHAPES + [(3, 5, 44, 14, 45)])
def test_cfg_mirror(hip, B, T, D, C, ld, dtype):
    x0 = rnd((2 * B, T, ld), 6, dtype)
    x0[B:] = SENT                                            # the second half: a sentinel everywhere
    t0 = torch.arange(2 * B, dtype=torch.int64) * 7 + 1
    x, t = x0.to(DEV), t0.to(DEV)
    hip.cfg_mirror(x, t, C, D=D)
    torch.cuda.synchronize()
    wx, wt = CR.cfg_mirror(x0, t0, C, D)
    assert same_bits(x, wx) and torch.equal(t.cpu(), wt)
    assert same_bits(x[:B], x0[:B]), "the first half is read only"
    sent = lambda v: same_bits(v, torch.full_like(v, SENT))
    assert sent(x[B:, :, :C]) and sent(x[B:, :, D:]), "conditioning and pad columns of the second half are left as found"
    assert same_bits(x[B:, :, C:D], x0[:B, :, C:D])
