"""Decoupled weight decay inside the fused optimizer kernel (ib_optim_step_decay / ib_optim_step_sources_decay and the table
builder ib_decay_table_build, csrc/optim.hip) on the GPU.  Every check but the last is BITWISE, no tolerance.

The yardstick is code older than the decay: the entries without it (`_ema`, `_sched`, plain), started from the same buffers
except that the quads to be decayed were first multiplied by f with a torch fp32 multiply, f = weight_decay.decay_factor (host
float64 arithmetic) of the rate the launch uses -- the host rate, or the probe's value (ib_lr_schedule_eval) under a schedule.
Nothing of the reference's decay comes from the new kernel.

  1. decomposition: six optimizers, the plain form (n = 8195: an n % 4 tail) and the gradient-sources form (slabs, column
     sums with a ragged 30-column range, kind-3 ranges), the step number from the host, from step_dev + step and from the
     ticket launch, with and without the EMA, with and without a cosine schedule (w = 5, T = 15, m = 0.1; steps 1, 5, 6, 15, 16);
  2. the factor itself: SGD, g = 0, p = 1 leaves decay_factor(lr_s, wd) on the decayed elements and 1 on the others;
  3. table edges: slices whose origin lies inside a range, ranges that end at the slice end, lie wholly below or above it,
     4-element ranges, a range at 0, adjacent ranges, bounds inside one wave's span, a length of 6 (counts as 8), the tail quad
     covered and not, 300 ranges, an empty table, wd = 0;
  4. a kind-3 range inside a decayed range keeps every buffer; 5. a decayed ragged column-sum range keeps its padding lanes;
  6. bad arguments give the error code and launch nothing;
  7. AdamW against torch.optim.AdamW on the CPU over ten steps, at the bound of the Adam trajectory test (2e-5).  -m gpu."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
OPTS = ["sgd", "adam", "rmsprop", "adagrad", "adadelta", "adamax"]
UPDATE_STEPS = [1, 5, 6, 15, 16]
BASE_LR = 1e-2
WD = 0.1
NAMES = ("p", "s1", "s2", "shadow", "ema")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def decay_mask(ranges, origin, n):
    """which of the n elements of a slice at `origin` the table decays: by quads, a length rounded up to a multiple of 4, the
    n % 4 tail with quad n / 4 (origin and every start are multiples of 4, so global and local quads coincide)"""
    m = torch.zeros((n + 3) // 4 * 4, dtype=torch.bool)
    for a, ln in ranges:
        lo, hi = a - origin, a + (ln + 3) // 4 * 4 - origin
        m[max(lo, 0):max(min(hi, m.numel()), 0)] = True
    return m[:n]


def f_of(rate):
    from inferbiomechanics_amd.weight_decay import decay_factor
    return decay_factor(rate, WD)


def sources_setup(n, gen):
    """slab ranges, column-sum ranges (one ragged: 30 columns, 2 padding elements behind it) and two kind-3 ranges of a
    flat buffer of n elements -> (make_sources(grad), updated-element mask)"""
    part = torch.randn(40, 256, generator=gen).to(DEV)
    slabs = [(64, 1000, 3), (2000, 256, 9)]
    slab_ws = [(torch.randn(ns, ln, generator=gen) * 1e-2).to(DEV) for _, ln, ns in slabs]
    cols = [(1200, 30, 17, 0), (3000, 64, 40, 32)]                 # (start, ncols, rows, first column in part)
    done = [(4000, 400), (6000, 4)]
    mask = torch.ones(n, dtype=torch.bool)
    for s, ln in done:
        mask[s:s + ln] = False
    mask[1230:1232] = False                                         # the ragged range's alignment padding

    def make(grad):
        items = [(ws, ns, grad[s:s + ln]) for (s, ln, ns), ws in zip(slabs, slab_ws)]
        segs = [(c0, nc, grad[s:s + nc], None, 0.5, part, rows) for s, nc, rows, c0 in cols]
        return (items, None, 0, segs, [grad[s:s + ln] for s, ln in done])
    return make, mask


# decayed ranges of the two forms.  plain: one at 0, the n % 4 tail (8192, 3).  sources: a slab range in part and in whole,
# the ragged column-sum range with its padding, half of the other one, and ranges over both kind-3 ranges and their borders
RANGES = {"plain": [(0, 1000), (1200, 30), (2048, 2052), (8192, 3)],
          "sources": [(0, 512), (1200, 30), (2000, 256), (3000, 32), (3900, 300), (5996, 12), (8000, 192)]}


@pytest.fixture(scope="module")
def schedule():
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.lr_schedule import LrSchedule
    sch = LrSchedule("cosine", 5, 15, 0.1)
    out = hip.lr_schedule_eval(BASE_LR, sch, torch.tensor(UPDATE_STEPS, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    rates = dict(zip(UPDATE_STEPS, (float(v) for v in out.cpu().numpy())))
    assert len(set(rates.values())) == 4 and rates[15] == rates[16], rates
    return sch, rates


@pytest.fixture(scope="module")
def inputs():
    """one set of buffers per form, made once: every case clones what it updates"""
    from inferbiomechanics_amd import hip
    out = {}
    for form, n in (("plain", 8195), ("sources", 8192)):
        gen = torch.Generator().manual_seed(11)
        p0 = torch.randn(n, generator=gen).to(DEV)
        g = (torch.randn(n, generator=gen) * 1e-2).to(DEV)
        s10 = torch.rand(n, generator=gen).to(DEV) * 1e-3
        s20 = torch.rand(n, generator=gen).to(DEV) * 1e-3
        e0 = (p0 + torch.randn(n, generator=gen).to(DEV) * 1e-2).contiguous()
        make, mask = sources_setup(n, gen) if form == "sources" else ((lambda grad: None), torch.ones(n, dtype=torch.bool))
        table = hip.DecayTable(RANGES[form], DEV)
        out[form] = (n, p0, g, s10, s20, e0, make, mask, table)
    return out


def launch(opt, bufs, mode, s, with_ema, lr, sch, decay=None, pre=None, lo=0, hi=None):
    """one optimizer launch over elements [lo, hi) of fresh clones of the buffers -> p, s1, s2, shadow, ema on the host.
    decay = (wd, table): the new entries.  pre = (mask, f): the reference -- p[mask] *= f by torch before the old entry."""
    from inferbiomechanics_amd import hip
    n, p0, g, s10, s20, e0, make = bufs[:7]
    hi = n if hi is None else hi
    p, s1, s2, e = p0.clone(), s10.clone(), s20.clone(), e0.clone()
    shadow = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    if pre is not None:
        mask, f = pre
        idx = mask.to(DEV)
        p[idx] = p[idx] * torch.tensor(f, dtype=torch.float32, device=DEV)
    if mode == "host":
        kw = {"step": s}
    elif mode == "step_dev":
        kw = {"step": 1, "step_dev": torch.full((1,), s - 1, dtype=torch.int32, device=DEV)}
    else:
        kw = {"step_dev": torch.full((1,), s - 1, dtype=torch.int32, device=DEV),
              "ticket": torch.zeros(hip.optim_ticket_words(), dtype=torch.int32, device=DEV)}
    sl = lambda t: t[lo:hi]
    if with_ema:
        kw.update(ema=sl(e), ema_decay=0.9, ema_warmup=True)
    if sch is not None:
        kw.update(lr_schedule=sch)
    if decay is not None:
        kw.update(weight_decay=decay[0], decay_table=decay[1], decay_origin=lo)
    src = make(g) if (lo, hi) == (0, n) else None
    hip.optim_step(opt, sl(p), sl(g), sl(s1), sl(s2), lr, grad_scale=0.5, shadow=sl(shadow), sources=src, **kw)
    torch.cuda.synchronize()
    if mode == "ticket":
        assert int(kw["step_dev"].cpu()) == s, "the ticket launch advances step_dev by one"
        assert int(kw["ticket"].abs().sum().cpu()) == 0, "and leaves the ticket words zero"
    return p.cpu(), s1.cpu(), s2.cpu(), shadow.cpu(), e.cpu()


def same(got, ref, what):
    for a, b, nm in zip(ref, got, NAMES):
        assert torch.equal(_bits(a), _bits(b)), (what, nm, int((_bits(a) != _bits(b)).sum()),
                                                 (_bits(a) != _bits(b)).nonzero()[:4].flatten().tolist())


# ---------------------------------------------------------------------------------------------------------------------
# 1. decomposition (fails at the parent: there is no decay)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", OPTS)
@pytest.mark.parametrize("form", ["plain", "sources"])
@pytest.mark.parametrize("mode", ["host", "step_dev", "ticket"])
def test_decayed_update_is_a_torch_multiply_then_the_old_update(opt, form, mode, schedule, inputs):
    sch, rates = schedule
    bufs = inputs[form]
    n, p0, mask, table = bufs[0], bufs[1].cpu(), bufs[7], bufs[8]
    dmask = decay_mask(RANGES[form], 0, n) & mask          # decayed AND updated by this launch (not kind 3, not padding)
    assert 0 < int(dmask.sum()) < int(mask.sum())
    for with_ema in (False, True):
        for use_sch, steps in ((True, UPDATE_STEPS), (False, [1, 6])):
            for s in steps:
                rate = rates[s] if use_sch else float(np.float32(BASE_LR))
                f = f_of(rate)
                assert 0.0 < f < 1.0
                ref = launch(opt, bufs, mode, s, with_ema, rate, None, pre=(dmask, f))
                got = launch(opt, bufs, mode, s, with_ema, BASE_LR, sch if use_sch else None, decay=(WD, table))
                what = (opt, form, mode, s, with_ema, use_sch)
                same(got, ref, what)
                assert torch.equal(_bits(got[0][~mask]), _bits(p0[~mask])), what      # only what the launch owns
                plain = launch(opt, bufs, mode, s, with_ema, rate, None)
                assert torch.equal(_bits(got[0][~dmask]), _bits(plain[0][~dmask])), (what, "undecayed elements: the old update")
                assert not torch.equal(got[0][dmask], plain[0][dmask]), (what, "the decay reaches the decayed ones")


# ---------------------------------------------------------------------------------------------------------------------
# 2. the factor
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plain", "sources"])
def test_sgd_without_gradient_leaves_the_factor(form, schedule, inputs):
    from inferbiomechanics_amd import hip
    sch, rates = schedule
    n, table = inputs[form][0], inputs[form][8]
    dmask = decay_mask(RANGES[form], 0, n)
    one, zero = torch.ones(n, device=DEV), torch.zeros(n, device=DEV)
    for lr, use_sch, s in [(BASE_LR, False, 3), (3e-4, False, 1), (1.0, False, 2)] + [(BASE_LR, True, s) for s in UPDATE_STEPS]:
        p = one.clone()
        src = ([], None, 0, [], []) if form == "sources" else None
        hip.optim_step("sgd", p, zero, None, None, lr, step=s, sources=src, weight_decay=WD, decay_table=table,
                       lr_schedule=sch if use_sch else None)
        torch.cuda.synchronize()
        f = np.float32(f_of(rates[s] if use_sch else lr))
        want = torch.where(dmask, torch.tensor(float(f)), torch.tensor(1.0))
        assert torch.equal(_bits(p.cpu()), _bits(want)), (form, lr, use_sch, s, float(f))
        assert f != np.float32(1.0)


# ---------------------------------------------------------------------------------------------------------------------
# 3. table edges
# ---------------------------------------------------------------------------------------------------------------------
WAVE = [(0, 4), (4, 8), (252, 8), (1020, 8)]            # a range at 0 touching [4, 12); bounds inside one wave's 256 elements
EDGES = {
    # slice [1024, 3072): a range wholly below, one the origin lies inside, a 4-element one with an adjacent neighbour, a
    # length of 6 (counts as 8), one ending exactly at the slice end, one wholly above
    "slice": (1024, 3072, [(0, 512), (768, 512), (1536, 4), (1540, 8), (2000, 6), (3000, 72), (4096, 100)]),
    "slice_inside_one_range": (1024, 3072, [(512, 4096)]),
    "slice_between_ranges": (1024, 3072, [(0, 1024), (3072, 1024)]),
    "wave_bounds_tail_covered": (0, 8195, WAVE + [(8192, 3)]),
    "wave_bounds_tail_uncovered": (0, 8195, WAVE + [(8188, 4)]),
    "tail_alone": (0, 8195, [(8192, 1)]),
    "ranges_300": (0, 8195, [(8 * k, 4) for k in range(300)]),
    "ranges_300_from_inside": (1204, 8192, [(8 * k, 4) for k in range(300)]),
}


@pytest.mark.parametrize("case", sorted(EDGES))
@pytest.mark.parametrize("opt", ["adam", "sgd"])
def test_table_edges(case, opt, inputs):
    from inferbiomechanics_amd import hip
    lo, hi, ranges = EDGES[case]
    bufs = inputs["plain"]
    table = hip.DecayTable(ranges, DEV)
    dmask = torch.zeros(bufs[0], dtype=torch.bool)
    dmask[lo:hi] = decay_mask(ranges, lo, hi - lo)
    assert dmask.any() == (case != "slice_between_ranges") and dmask[lo:hi].all() == (case == "slice_inside_one_range")
    if case == "wave_bounds_tail_covered":
        assert dmask[8192:8195].all() and not dmask[8188:8192].any()
    if case == "wave_bounds_tail_uncovered":
        assert not dmask[8192:8195].any() and dmask[8188:8192].all()
    if case == "slice":
        assert dmask[1024:1280].all() and dmask[2000:2008].all() and not dmask[2008] and dmask[3071] and dmask[1536:1548].all()
    f = f_of(BASE_LR)
    for with_ema in (False, True):
        ref = launch(opt, bufs, "host", 3, with_ema, BASE_LR, None, pre=(dmask, f), lo=lo, hi=hi)
        got = launch(opt, bufs, "host", 3, with_ema, BASE_LR, None, decay=(WD, table), lo=lo, hi=hi)
        same(got, ref, (case, opt, with_ema))
        outside = torch.ones(bufs[0], dtype=torch.bool)
        outside[lo:hi] = False
        assert torch.equal(_bits(got[0][outside]), _bits(bufs[1].cpu()[outside])), "nothing beyond the slice"


def _raw_plain(lib, hip, opt, p, g, s1, s2, shadow, ema, lr, step, sched, decay):
    """ib_optim_step_decay called directly (the binding takes the old entries at weight_decay = 0)"""
    P = lambda t: None if t is None else t.data_ptr()
    return lib.ib_optim_step_decay(hip.OPT[opt], P(p), P(g), P(s1), P(s2), p.numel(), lr, 0.5, step, None, None, P(shadow),
                                   P(ema), 0.9, 1, *sched, *decay, hip.stream_ptr())


@pytest.mark.parametrize("opt", ["adam", "rmsprop"])
def test_nothing_to_decay_is_the_old_entry_bitwise(opt, schedule, inputs):
    from inferbiomechanics_amd import hip
    lib = hip.lib()
    sch, rates = schedule
    bufs = inputs["plain"]
    n, p0, g, s10, s20, e0 = bufs[:6]
    full = hip.DecayTable([(0, 8196)], DEV)
    empty = hip.DecayTable([], DEV)
    for with_ema in (False, True):
        for sched, old_sch in (((0, 0, 0, 0.0), None), ((2, 5, 15, 0.1), sch)):
            ref = launch(opt, bufs, "host", 6, with_ema, BASE_LR, old_sch)
            for decay in ((WD, empty.buf.data_ptr(), 0, 0), (WD, None, 0, 0), (0.0, full.buf.data_ptr(), 1, 0)):
                p, s1, s2, e = p0.clone(), s10.clone(), s20.clone(), e0.clone()
                shadow = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
                assert _raw_plain(lib, hip, opt, p, g, s1, s2, shadow, e if with_ema else None, BASE_LR, 6, sched, decay) == 0
                torch.cuda.synchronize()
                same((p.cpu(), s1.cpu(), s2.cpu(), shadow.cpu(), e.cpu()), ref, (opt, with_ema, sched, decay[0], decay[2]))
            # and the full table with wd > 0 through the same direct call does decay: the call reaches the kernel
            p = p0.clone()
            assert _raw_plain(lib, hip, opt, p, g, s10.clone(), s20.clone(), None, None, BASE_LR, 6, sched,
                              (WD, full.buf.data_ptr(), 1, 0)) == 0
            torch.cuda.synchronize()
            assert not torch.equal(p.cpu(), ref[0])


# ---------------------------------------------------------------------------------------------------------------------
# 4. + 5. kind-3 ranges and the ragged column-sum range under a table that covers everything
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["adam", "sgd", "adadelta"])
def test_done_ranges_and_padding_lanes_keep_their_bits_under_full_decay(opt, inputs):
    from inferbiomechanics_amd import hip
    bufs = inputs["sources"]
    n, p0, g, s10, s20, e0, make, mask = bufs[:8]
    table = hip.DecayTable([(0, n)], DEV)
    f = f_of(BASE_LR)
    for mode in ("step_dev", "ticket"):
        ref = launch(opt, bufs, mode, 4, True, BASE_LR, None, pre=(mask, f))
        got = launch(opt, bufs, mode, 4, True, BASE_LR, None, decay=(WD, table))
        same(got, ref, (opt, mode))
        start = (p0.cpu(), s10.cpu(), s20.cpu(), torch.zeros(n, dtype=torch.bfloat16), e0.cpu())
        for (a, ln) in [(4000, 400), (6000, 4), (1230, 2)]:          # the two kind-3 ranges, the ragged range's padding lanes
            for t, t0, nm in zip(got, start, NAMES):
                if nm == "shadow" and a == 1230:                     # the quad's shadow is rewritten whole: bf16 of the kept p
                    t0 = start[0].to(torch.bfloat16)
                assert torch.equal(_bits(t[a:a + ln]), _bits(t0[a:a + ln])), (opt, mode, nm, a)
        # the ragged range's 30 columns and its neighbours were decayed and updated
        plain = launch(opt, bufs, mode, 4, True, BASE_LR, None)
        assert not torch.equal(got[0][1200:1230], plain[0][1200:1230]) and not torch.equal(got[0][3000:3064], plain[0][3000:3064])
        assert not torch.equal(got[0][1200:1230], p0.cpu()[1200:1230])


# ---------------------------------------------------------------------------------------------------------------------
# 6. bad arguments
# ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_give_the_error_code_and_launch_nothing():
    from inferbiomechanics_amd import hip
    lib = hip.lib()
    n = 1024
    P = lambda t: t.data_ptr()
    p, g = torch.full((n,), 5.0, device=DEV), torch.ones(n, device=DEV)
    ema = torch.full((n,), 3.0, device=DEV)
    good = hip.DecayTable([(0, 512)], DEV)
    canary = torch.full((64,), -7, dtype=torch.int64, device=DEV)
    nan = float("nan")
    cv = lambda a: ctypes.cast(a, ctypes.c_void_p)
    arr = lambda *v: (ctypes.c_int64 * len(v))(*v)
    for start, ln in [((8, 0), (4, 4)), ((0, 4), (8, 4)), ((0, 4), (6, 4)), ((-4,), (4,)), ((2,), (4,)), ((0,), (0,)), ((0,), (-4,)),
                      ((0, 0), (4, 4))]:
        assert lib.ib_decay_table_build(cv(arr(*start)), cv(arr(*ln)), len(start), P(canary), hip.stream_ptr()) == -1, (start, ln)
    assert lib.ib_decay_table_build(cv(arr(0)), cv(arr(4)), -1, P(canary), hip.stream_ptr()) == -1
    assert lib.ib_decay_table_build(cv(arr(0)), cv(arr(4)), 1, None, hip.stream_ptr()) == -1
    assert lib.ib_decay_table_build(None, cv(arr(4)), 1, P(canary), hip.stream_ptr()) == -1
    assert lib.ib_decay_table_build(cv(arr(0)), cv(arr(4)), 1, P(canary) + 8, hip.stream_ptr()) == -1
    with pytest.raises(hip.HipError):
        hip.DecayTable([(16, 8), (0, 8)], DEV)
    ok_s = (2, 5, 15, 0.1)
    T = P(good.buf)
    bad = [(ok_s, (-0.1, T, 1, 0)), (ok_s, (nan, T, 1, 0)), (ok_s, (0.1, T, -1, 0)), (ok_s, (0.1, None, 1, 0)), (ok_s, (0.1, T, 1, -4)),
           (ok_s, (0.1, T, 1, 2)), ((0, 0, 0, 0.0), (-1.0, T, 1, 0)), ((3, 0, 10, 0.0), (0.1, T, 1, 0)), ((1, 5, 5, 0.0), (0.1, T, 1, 0)),
           ((2, 0, 10, nan), (0.1, T, 1, 0))]
    for s, d in bad:
        assert lib.ib_optim_step_decay(hip.OPT["sgd"], P(p), P(g), None, None, n, 1e-2, 1.0, 1, None, None, None, P(ema), 0.5, 0,
                                       *s, *d, hip.stream_ptr()) == -1, (s, d)
        assert lib.ib_optim_step_sources_decay(hip.OPT["sgd"], P(p), P(g), None, None, n, 1e-2, 1.0, 1, None, None, None, 0, None,
                                               None, None, None, None, None, None, None, 0, 0, 0.0, None, P(ema), 0.5, 0,
                                               *s, *d, hip.stream_ptr()) == -1, (s, d)
    # a bad EMA under good decay arguments, through the binding
    with pytest.raises(hip.HipError):
        hip.optim_step("sgd", p, g, None, None, 1e-2, ema=ema, ema_decay=1.5, weight_decay=0.1, decay_table=good)
    with pytest.raises(hip.HipError):
        hip.optim_step("sgd", p, g, None, None, 1e-2, weight_decay=-0.1, decay_table=good)
    with pytest.raises(hip.HipError):
        hip.optim_step("sgd", p, g, None, None, 1e-2, weight_decay=0.1, decay_table=good, decay_origin=6)
    torch.cuda.synchronize()
    assert bool((p == 5.0).all()) and bool((ema == 3.0).all()) and bool((canary == -7).all()), "nothing was launched or uploaded"
    assert good.buf.cpu().tolist() == [0, 512]


# ---------------------------------------------------------------------------------------------------------------------
# 7. AdamW against torch
# ---------------------------------------------------------------------------------------------------------------------
def close(actual, expected, rtol, what=""):
    """tests/test_hip_kernels.py's: the largest error against rtol times the largest expected magnitude"""
    a = actual.detach().to("cpu", torch.float64)
    e = expected.detach().to("cpu", torch.float64)
    assert a.shape == e.shape, (what, a.shape, e.shape)
    assert torch.isfinite(a).all(), f"{what}: non-finite values"
    err = (a - e).abs().max().item()
    ref = max(e.abs().max().item(), 1e-30)
    assert err <= rtol * ref, f"{what}: max err {err:.3e} > {rtol:.1e} * {ref:.3e}"


def test_adamw_follows_torch_optim_adamw():
    from inferbiomechanics_amd import hip
    from oracle import ref_cpu as R
    n, lr, wd = 257, 1e-2, 0.1
    p0 = R.det_fill((n,), 3, 0.5).float()
    grads = [R.det_fill((n,), 20 + s, 0.3 * (s + 1)).float() for s in range(10)]
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([ref], lr=lr, weight_decay=wd)
    table = hip.DecayTable([(0, n)], DEV)                  # everything decayed; 257 = 64 quads and a tail of one
    p, s1, s2 = p0.clone().to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    shadow = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    for s in range(10):
        ref.grad = grads[s].clone()
        opt.step()
        hip.optim_step("adam", p, grads[s].to(DEV) * 4.0, s1, s2, lr=lr, step=s + 1, grad_scale=0.25, shadow=shadow,
                       weight_decay=wd, decay_table=table)
        close(p, ref.detach(), 2e-5, f"adamw step {s + 1}")
        assert torch.equal(shadow.cpu(), p.cpu().to(torch.bfloat16))
    plain = torch.nn.Parameter(p0.clone())
    o2 = torch.optim.Adam([plain], lr=lr)
    for s in range(10):
        plain.grad = grads[s].clone()
        o2.step()
    assert float((plain.detach() - ref.detach()).abs().max()) > 1e-3, "the decay is visible at this bound"
