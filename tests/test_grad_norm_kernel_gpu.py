"""Clipping to a global gradient norm inside the fused optimizer (ib_grad_sumsq, ib_grad_norm_eval, ib_optim_step_gradnorm,
csrc/optim.hip) on the GPU.

  1. the norm: sizes at every edge of the slot layout (quads, the n % 4 tail, one slot +- 1, two slots, beyond the 1024-slot
     cap with n % 4 = 3, a slice that is 16-byte but not 4-KB aligned), normal inputs and one whose magnitudes span
     1e-20 .. 1e10.  norm within 1 fp32 ulp of float32(sqrt(sum(float64(g)^2))): the double sum's own relative error is below
     n 2^-53 (< 2e-9 at the largest n), the square root halves it, so the one rounding to fp32 is what is left.  coef and gs
     within 1 fp32 ulp of grad_norm.clip_coef(the device's total): the host's restatement of the same double arithmetic,
     one ulp for the libraries' sqrt.  Two runs bitwise equal.  g = 0: norm 0, coef 1; one inf: coef 0; one NaN: coef 1.
  2. decomposition, BITWISE: six optimizers, n = 3 (the tail alone), 256 (quads alone) and 8195, the step number from the host, from step_dev + step and from the ticket
     launch, with and without EMA + cosine schedule + decay table, grad_scale 1 and 0.5, max_norm below and above the norm:
     p, s1, s2, shadow, ema equal the entries older than the clip called with grad_scale = gs, gs read from the probe.
  3. AdamW with torch.nn.utils.clip_grad_norm_ on the CPU over ten steps, at the bound of the Adam trajectory test (2e-5).
-m gpu."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
OPTS = ["sgd", "adam", "rmsprop", "adagrad", "adadelta", "adamax"]
BASE_LR, WD = 1e-2, 0.1
NAMES = ("p", "s1", "s2", "shadow", "ema")
S, CAP = 16384, 1024
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, S - 1, S, S + 1, 2 * S, 2 * S + 1025, CAP * S + 3]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def ulps(a, b):
    """distance in fp32 places between two non-negative finite fp32 values"""
    ia, ib = (int(np.float32(v).view(np.int32)) for v in (a, b))
    return abs(ia - ib)


def host_norm(g):
    return float(np.float32(math.sqrt(float((g.double() ** 2).sum()))))


def measure(g, grad_scale=1.0, max_norm=float("inf")):
    """slots, total and {norm, coef, gs} of the device for the gradient g"""
    from inferbiomechanics_amd import hip
    slots = hip.grad_sumsq(g)
    total, stats = hip.grad_norm_eval(slots, grad_scale, max_norm)
    torch.cuda.synchronize()
    return slots.cpu(), float(total.cpu()[0]), [float(v) for v in stats.cpu()]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the norm
# ---------------------------------------------------------------------------------------------------------------------
def check_norm(g_host, g_dev):
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.grad_norm import clip_coef
    n = g_host.numel()
    want = host_norm(g_host)
    slots, total, (norm, coef, gs) = measure(g_dev)
    assert slots.numel() == hip.grad_sumsq_slots(n) == min(max(-(-n // S), 1), CAP)
    print(f"n={n} norm={norm!r} want={want!r} total={total!r}")
    assert ulps(norm, want) <= 1, (n, norm, want)
    # both this sum and torch's stay within n 2^-53 of the exact one (all terms are >= 0)
    assert abs(total - float((g_host.double() ** 2).sum())) <= 2 * n * 2.0 ** -53 * total, "the double sum's own error"
    assert (coef, gs) == (1.0, 1.0), "max_norm = inf never clips"
    for grad_scale, frac in ((1.0, 0.5), (0.5, 0.37), (0.5, 4.0)):
        mx = float(np.float32(frac * want * grad_scale))
        slots2, total2, got = measure(g_dev, grad_scale, mx)
        assert total2 == total and torch.equal(slots2.view(torch.int64), slots.view(torch.int64)), "two runs are bitwise equal"
        ref = clip_coef(total, grad_scale, mx)
        print(f"  grad_scale={grad_scale} max_norm={mx!r} device={got} host={ref}")
        assert all(ulps(a, b) <= 1 for a, b in zip(got, ref)), (n, grad_scale, mx, got, ref)
        if want > 1e-3:                                      # below that the 1e-6 in the denominator decides
            assert (got[1] < 1.0) == (frac < 1.0) and (frac < 1.0 or got[2] == grad_scale)


@pytest.mark.parametrize("n", SIZES)
def test_norm_of_normal_inputs(n):
    gen = torch.Generator().manual_seed(n % 1000)
    g = torch.randn(n, generator=gen)
    check_norm(g, g.to(DEV))


def test_norm_of_a_slice_that_is_not_4k_aligned():
    gen = torch.Generator().manual_seed(3)
    big = torch.randn(2 * S + 64, generator=gen).to(DEV)
    g = big[12:12 + S + 7]                                   # 48 bytes into the allocation: 16-byte aligned, no more
    assert g.data_ptr() % 16 == 0 and g.data_ptr() % 4096 != 0
    check_norm(g.cpu(), g)


def test_norm_over_thirty_decades():
    """magnitudes 1e-20 .. 1e10: the squares span 1e-40 .. 1e20 -- below fp32's normal range at one end, and the large ones
    would absorb everything else in an fp32 sum; the double sum holds them"""
    gen = torch.Generator().manual_seed(4)
    n = 3 * S + 5
    g = torch.randn(n, generator=gen) * (10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 30 - 20)).float()
    assert float(g.abs().max()) > 1e8 and float(g.abs()[g != 0].min()) < 1e-18
    check_norm(g, g.to(DEV))
    # the small end alone: every square is subnormal or zero in fp32
    small = g[g.abs() < 1e-19][:4099].contiguous()
    assert small.numel() > 500
    check_norm(small, small.to(DEV))


def test_zero_inf_and_nan_gradients():
    n = S + 5
    _, total, stats = measure(torch.zeros(n, device=DEV), 1.0, 1.0)
    assert total == 0.0 and stats == [0.0, 1.0, 1.0], "a zero gradient: norm 0, coefficient 1"
    g = torch.randn(n, generator=torch.Generator().manual_seed(5)).to(DEV)
    g[n - 2] = float("inf")
    _, total, stats = measure(g, 0.5, 1.0)
    assert math.isinf(total) and math.isinf(stats[0]) and stats[1:] == [0.0, 0.0], "an infinite norm: coefficient 0"
    g[7] = float("nan")
    _, total, stats = measure(g, 0.5, 1.0)
    assert math.isnan(total) and math.isnan(stats[0]) and stats[1:] == [1.0, 0.5], "a NaN norm: coefficient 1"


# ---------------------------------------------------------------------------------------------------------------------
# 2. decomposition
# ---------------------------------------------------------------------------------------------------------------------
RANGES = [(0, 1000), (1200, 30), (2048, 2052), (8192, 3)]        # the decay kernel test's: one at 0, the n % 4 tail
# the decomposition's sizes and their decay ranges (each covers the first quad and ends inside the buffer): 3 = no quad, the
# tail alone, one workgroup; 256 = quads alone, no tail; 8195 = eight workgroups of quads and a tail
SIZED_RANGES = {3: [(0, 3)], 256: [(0, 100), (120, 30), (200, 40)], 8195: RANGES}


def make_inputs(n, ranges):
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.lr_schedule import LrSchedule
    gen = torch.Generator().manual_seed(11)
    p0 = torch.randn(n, generator=gen).to(DEV)
    g = (torch.randn(n, generator=gen) * 1e-2).to(DEV)
    s10 = torch.rand(n, generator=gen).to(DEV) * 1e-3
    s20 = torch.rand(n, generator=gen).to(DEV) * 1e-3
    e0 = (p0 + torch.randn(n, generator=gen).to(DEV) * 1e-2).contiguous()
    slots = hip.grad_sumsq(g)
    torch.cuda.synchronize()
    return n, p0, g, s10, s20, e0, slots, hip.DecayTable(ranges, DEV), LrSchedule("cosine", 5, 15, 0.1), host_norm(g.cpu())


@pytest.fixture(scope="module")
def sized_inputs():
    return {n: make_inputs(n, ranges) for n, ranges in SIZED_RANGES.items()}


@pytest.fixture(scope="module")
def inputs(sized_inputs):
    return sized_inputs[8195]


def launch(opt, bufs, mode, s, full, grad_scale, clip=None):
    """one optimizer launch over fresh clones -> (p, s1, s2, shadow, ema) on the host, the stats it wrote (clip = max_norm)"""
    from inferbiomechanics_amd import hip
    n, p0, g, s10, s20, e0, slots, table, sch, _ = bufs
    p, s1, s2, e = p0.clone(), s10.clone(), s20.clone(), e0.clone()
    shadow = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    if mode == "host":
        kw = {"step": s}
    elif mode == "step_dev":
        kw = {"step": 1, "step_dev": torch.full((1,), s - 1, dtype=torch.int32, device=DEV)}
    else:
        kw = {"step_dev": torch.full((1,), s - 1, dtype=torch.int32, device=DEV),
              "ticket": torch.zeros(hip.optim_ticket_words(), dtype=torch.int32, device=DEV)}
    if full:
        kw.update(ema=e, ema_decay=0.9, ema_warmup=True, lr_schedule=sch, weight_decay=WD, decay_table=table)
    stats = torch.full((4,), -1.0, device=DEV)
    if clip is not None:
        kw.update(max_grad_norm=clip, norm_slots=slots, norm_stats=stats)
    hip.optim_step(opt, p, g, s1, s2, BASE_LR, grad_scale=grad_scale, shadow=shadow, **kw)
    torch.cuda.synchronize()
    if mode == "ticket":
        assert int(kw["step_dev"].cpu()) == s, "the ticket launch publishes the step"
        assert int(kw["ticket"].abs().sum().cpu()) == 0, "and leaves the ticket words zero"
    return (p.cpu(), s1.cpu(), s2.cpu(), shadow.cpu(), e.cpu()), stats.cpu()


@pytest.mark.parametrize("opt", OPTS)
@pytest.mark.parametrize("mode", ["host", "step_dev", "ticket"])
def test_clipped_update_is_the_old_entry_with_the_probes_scale(opt, mode, sized_inputs):
    for n in sorted(sized_inputs):
        clipped_update_is_the_old_entry(opt, mode, sized_inputs[n])


def clipped_update_is_the_old_entry(opt, mode, inputs):
    from inferbiomechanics_amd import hip
    slots, norm = inputs[6], inputs[9]
    for full, steps in ((True, [1, 6, 16]), (False, [6])):
        for grad_scale in (1.0, 0.5):
            for frac in (0.5, 2.0):
                mx = float(np.float32(frac * norm * grad_scale))
                _, probe = hip.grad_norm_eval(slots, grad_scale, mx)
                probe = probe.cpu()
                coef, gs = float(probe[1]), float(probe[2])
                assert (coef < 1.0 and gs < grad_scale) if frac < 1 else (coef == 1.0 and gs == grad_scale), (frac, coef, gs)
                for s in steps:
                    what = (inputs[0], opt, mode, full, grad_scale, frac, s)
                    ref, untouched = launch(opt, inputs, mode, s, full, gs)
                    got, stats = launch(opt, inputs, mode, s, full, grad_scale, clip=mx)
                    for a, b, nm in zip(ref, got, NAMES):
                        assert torch.equal(_bits(a), _bits(b)), (what, nm, int((_bits(a) != _bits(b)).sum()),
                                                                 (_bits(a) != _bits(b)).nonzero()[:4].flatten().tolist())
                    assert torch.equal(_bits(stats[:3]), _bits(probe)), (what, stats, probe)
                    assert float(stats[3]) == -1.0 and bool((untouched == -1.0).all())
                if frac < 1:
                    plain, _ = launch(opt, inputs, mode, steps[-1], full, grad_scale)
                    assert not torch.equal(plain[0], got[0]) or opt in ("adam", "adamax"), (what, "the clip reaches the update")


def test_bad_arguments_launch_nothing(inputs):
    from inferbiomechanics_amd import hip
    n, p0, g, s10, s20, e0, slots = inputs[:7]
    p = p0.clone()
    stats = torch.full((4,), -1.0, device=DEV)
    for bad in (dict(max_grad_norm=-1.0, norm_slots=slots, norm_stats=stats), dict(max_grad_norm=1.0, norm_stats=stats),
                dict(max_grad_norm=1.0, norm_slots=slots), dict(max_grad_norm=float("nan"), norm_slots=slots, norm_stats=stats),
                dict(max_grad_norm=1.0, norm_slots=slots, norm_stats=stats, sources=([], None, 0, [], []))):
        with pytest.raises(hip.HipError):
            hip.optim_step("sgd", p, g, None, None, 1e-2, **bad)
    P = lambda t: t.data_ptr()
    lib = hip.lib()
    for c in [(None, n, 1.0, P(stats)), (P(slots) + 8, n, 1.0, P(stats)), (P(slots), 0, 1.0, P(stats)), (P(slots), n, 0.0, P(stats)),
              (P(slots), n, 1.0, None), (P(slots), n, 1.0, P(stats) + 4)]:
        assert lib.ib_optim_step_gradnorm(0, P(p), P(g), None, None, n, 1e-2, 1.0, 1, None, None, None, None, 0.0, 0,
                                          0, 0, 0, 0.0, 0.0, None, 0, 0, *c, hip.stream_ptr()) == -1, c
    torch.cuda.synchronize()
    assert torch.equal(p, p0) and bool((stats == -1.0).all())


# ---------------------------------------------------------------------------------------------------------------------
# 3. against torch
# ---------------------------------------------------------------------------------------------------------------------
def close(actual, expected, rtol, what=""):
    """tests/test_hip_kernels.py's: the largest error against rtol times the largest expected magnitude"""
    a = actual.detach().to("cpu", torch.float64)
    e = expected.detach().to("cpu", torch.float64)
    assert a.shape == e.shape and torch.isfinite(a).all(), what
    err = (a - e).abs().max().item()
    ref = max(e.abs().max().item(), 1e-30)
    assert err <= rtol * ref, f"{what}: max err {err:.3e} > {rtol:.1e} * {ref:.3e}"


def test_clipped_adamw_follows_torch_clip_grad_norm():
    from inferbiomechanics_amd import hip
    from oracle import ref_cpu as R
    n, lr, wd = 257, 1e-2, 0.1
    p0 = R.det_fill((n,), 3, 0.5).float()
    grads = [R.det_fill((n,), 20 + s, 0.3 * (s + 1)).float() for s in range(10)]       # the norm grows with the step
    norms = sorted(float(g.norm()) for g in grads)
    max_norm = 0.5 * (norms[4] + norms[5])                   # the median: half of the steps clip
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([ref], lr=lr, weight_decay=wd)
    table = hip.DecayTable([(0, n)], DEV)
    p, s1, s2 = p0.clone().to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    stats = torch.zeros(4, device=DEV)
    coefs = []
    for s in range(10):
        ref.grad = grads[s].clone()
        tn = torch.nn.utils.clip_grad_norm_([ref], max_norm)
        opt.step()
        g = grads[s].to(DEV) * 4.0                          # the sum over four ranks; grad_scale = 1 / 4
        slots = hip.grad_sumsq(g)
        hip.optim_step("adam", p, g, s1, s2, lr=lr, step=s + 1, grad_scale=0.25, weight_decay=wd, decay_table=table,
                       max_grad_norm=max_norm, norm_slots=slots, norm_stats=stats)
        close(p, ref.detach(), 2e-5, f"clipped adamw step {s + 1}")
        st = stats.cpu()
        close(st[:1], tn.detach().reshape(1), 1e-6, "the norm torch reports")
        coefs.append(float(st[1]))
    print("coefficients:", coefs)
    assert any(c < 1.0 for c in coefs) and any(c == 1.0 for c in coefs), coefs
    assert min(coefs) < 0.7, "a clip that matters at this bound"
