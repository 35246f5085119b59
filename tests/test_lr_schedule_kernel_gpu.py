"""The learning-rate schedule inside the fused optimizer kernel (ib_optim_step_sched / ib_optim_step_sources_sched and the
probe ib_lr_schedule_eval, csrc/optim.hip) on the GPU.

  * the probe -- one launch of the device function the optimizer kernel itself calls -- equals LrSchedule.lr_at bitwise for
    the constant and linear kinds and inside every warmup (correctly rounded double operations only, no fused
    multiply-add), and is within 1 fp32 ulp of it on a cosine decay (the device's double cos may differ from the host's in
    its last place, which can flip the final rounding to fp32 and nothing more);
  * bad arguments give the error code and launch nothing;
  * the update: all six optimizers, the plain form (n = 8195: an n % 4 tail) and the gradient-sources form (slabs, column
    sums with a ragged 30-column range, ranges already done = kind 3), the step number from the host, from step_dev + step
    and from the self-counting ticket launch, with and without the EMA, at steps 1, 5, 6, 15, 16 of a cosine schedule with
    w = 5, T = 15, m = 0.1: p, s1, s2, the bf16 shadow and ema are BITWISE those of the entry without a schedule called
    with the host rate set to the probe's value for that step.  No tolerance anywhere.  -m gpu."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
OPTS = ["sgd", "adam", "rmsprop", "adagrad", "adadelta", "adamax"]
KINDS = ["constant", "linear", "cosine"]
STEPS = [1, 4, 5, 6, 10, 14, 15, 16, 1015, 2_000_000_000]
UPDATE_STEPS = [1, 5, 6, 15, 16]
BASE_LR = 1e-2


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def probe(lr, sch, steps):
    from inferbiomechanics_amd import hip
    out = hip.lr_schedule_eval(lr, sch, torch.tensor(steps, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# the probe
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m", [0.0, 0.1, 1.0])
@pytest.mark.parametrize("w,T", [(5, 15), (0, 15), (14, 15), (100, 1_000_000)])
def test_probe_equals_the_host_restatement(kind, m, w, T):
    from inferbiomechanics_amd.lr_schedule import LrSchedule
    sch = LrSchedule(kind, w, T, m)
    steps = STEPS + [w, w + 1, T - 1, T, T + 1, (w + T) // 2]
    steps = [s for s in steps if s >= 1]
    for lr in (1e-3, 1.0, 3e-4):
        got = probe(lr, sch, steps)
        ref = np.array([sch.lr_at(lr, s) for s in steps], dtype=np.float32)
        exact = np.array([kind != "cosine" or s <= w for s in steps])
        assert np.array_equal(got[exact].view(np.int32), ref[exact].view(np.int32)), (kind, m, w, T, lr, got, ref)
        ulp = np.spacing(np.abs(ref)).astype(np.float64)
        assert np.all(np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= ulp), (kind, m, w, T, lr, got, ref)
        # the three identities, on the device's own values
        if w > 0:
            assert got[steps.index(w)] == np.float32(lr)
        if kind != "constant":
            at_T = np.float32(np.float64(np.float32(lr)) * np.float64(sch.min_ratio))
            assert got[steps.index(T)] == got[steps.index(T + 1)] == got[steps.index(2_000_000_000)] == at_T


def test_probe_and_entries_check_their_arguments():
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.lr_schedule import LrSchedule
    lib = hip.lib()
    n = 1024
    steps = torch.arange(1, 9, dtype=torch.int32, device=DEV)
    out = torch.full((8,), -7.0, device=DEV)
    p, g = torch.ones(n, device=DEV), torch.ones(n, device=DEV)
    ema = torch.full((n,), 3.0, device=DEV)
    nan = float("nan")
    for kind, w, T, m in [(3, 0, 10, 0.0), (-1, 0, 10, 0.0), (1, -1, 10, 0.0), (1, 5, 5, 0.0), (2, 5, 4, 0.0), (1, 0, 10, -0.1),
                          (1, 0, 10, 1.5), (2, 0, 10, nan), (0, 0, 0, nan)]:
        assert lib.ib_lr_schedule_eval(1e-3, kind, w, T, m, steps.data_ptr(), out.data_ptr(), 8, hip.stream_ptr()) == -1
        assert lib.ib_optim_step_sched(hip.OPT["sgd"], p.data_ptr(), g.data_ptr(), None, None, n, 1e-2, 1.0, 1, None, None, None,
                                       ema.data_ptr(), 0.5, 0, kind, w, T, m, hip.stream_ptr()) == -1
        assert lib.ib_optim_step_sources_sched(hip.OPT["sgd"], p.data_ptr(), g.data_ptr(), None, None, n, 1e-2, 1.0, 1, None,
                                               None, None, 0, None, None, None, None, None, None, None, None, 0, 0, 0.0, None,
                                               ema.data_ptr(), 0.5, 0, kind, w, T, m, hip.stream_ptr()) == -1
    sch = LrSchedule("cosine", 5, 15, 0.1)
    with pytest.raises(hip.HipError):                                     # a bad EMA under a good schedule
        hip.optim_step("sgd", p, g, None, None, 1e-2, ema=ema, ema_decay=1.5, lr_schedule=sch)
    with pytest.raises(hip.HipError):
        hip.optim_step("sgd", p, g, None, None, 1e-2, ema=ema[:n - 4], ema_decay=0.5, lr_schedule=sch)
    with pytest.raises(hip.HipError):
        hip.lr_schedule_eval(1e-3, sch, steps.cpu())
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((p == 1.0).all()) and bool((ema == 3.0).all()), "nothing was launched"


# ---------------------------------------------------------------------------------------------------------------------
# the update
# ---------------------------------------------------------------------------------------------------------------------
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


@pytest.fixture(scope="module")
def schedule():
    from inferbiomechanics_amd.lr_schedule import LrSchedule
    sch = LrSchedule("cosine", 5, 15, 0.1)
    rates = dict(zip(UPDATE_STEPS, (float(v) for v in probe(BASE_LR, sch, UPDATE_STEPS))))
    assert len(set(rates.values())) == 4 and rates[15] == rates[16], rates      # warmup, peak, decay, floor: all differ
    return sch, rates


@pytest.fixture(scope="module")
def inputs():
    """one set of buffers per form, made once: every case clones what it updates"""
    out = {}
    for form, n in (("plain", 8195), ("sources", 8192)):
        gen = torch.Generator().manual_seed(11)
        p0 = torch.randn(n, generator=gen).to(DEV)
        g = (torch.randn(n, generator=gen) * 1e-2).to(DEV)
        s10 = torch.rand(n, generator=gen).to(DEV) * 1e-3
        s20 = torch.rand(n, generator=gen).to(DEV) * 1e-3
        e0 = (p0 + torch.randn(n, generator=gen).to(DEV) * 1e-2).contiguous()
        make, mask = sources_setup(n, gen) if form == "sources" else ((lambda grad: None), torch.ones(n, dtype=torch.bool))
        out[form] = (n, p0, g, s10, s20, e0, make, mask)
    return out


def launch(opt, bufs, mode, s, with_ema, lr, sch):
    from inferbiomechanics_amd import hip
    n, p0, g, s10, s20, e0, make, _ = bufs
    p, s1, s2, e = p0.clone(), s10.clone(), s20.clone(), e0.clone()
    shadow = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    if mode == "host":
        kw = {"step": s}
    elif mode == "step_dev":
        kw = {"step": 1, "step_dev": torch.full((1,), s - 1, dtype=torch.int32, device=DEV)}
    else:
        kw = {"step_dev": torch.full((1,), s - 1, dtype=torch.int32, device=DEV),
              "ticket": torch.zeros(hip.optim_ticket_words(), dtype=torch.int32, device=DEV)}
    if with_ema:
        kw.update(ema=e, ema_decay=0.9, ema_warmup=True)
    if sch is not None:
        kw.update(lr_schedule=sch)
    hip.optim_step(opt, p, g, s1, s2, lr, grad_scale=0.5, shadow=shadow, sources=make(g), **kw)
    torch.cuda.synchronize()
    if mode == "ticket":
        assert int(kw["step_dev"].cpu()) == s, "the ticket launch advances step_dev by one"
        assert int(kw["ticket"].abs().sum().cpu()) == 0, "and leaves the ticket words zero"
    elif mode == "step_dev":
        assert int(kw["step_dev"].cpu()) == s - 1
    return p.cpu(), s1.cpu(), s2.cpu(), shadow.cpu(), e.cpu()


@pytest.mark.parametrize("opt", OPTS)
@pytest.mark.parametrize("form", ["plain", "sources"])
@pytest.mark.parametrize("mode", ["host", "step_dev", "ticket"])
def test_scheduled_update_is_the_unscheduled_one_at_the_probes_rate(opt, form, mode, schedule, inputs):
    sch, rates = schedule
    bufs = inputs[form]
    p0, e0, mask = bufs[1].cpu(), bufs[5].cpu(), bufs[7]
    seen = []
    for with_ema in (False, True):
        for s in UPDATE_STEPS:
            ref = launch(opt, bufs, mode, s, with_ema, rates[s], None)          # the existing entry, host rate
            got = launch(opt, bufs, mode, s, with_ema, BASE_LR, sch)            # the scheduled entry, base rate
            what = (opt, form, mode, s, with_ema)
            for a, b, nm in zip(ref, got, ("p", "s1", "s2", "shadow", "ema")):
                assert torch.equal(_bits(a), _bits(b)), (what, nm)
            assert not torch.equal(got[0][mask], p0[mask]), what                 # something was updated ...
            assert torch.equal(_bits(got[0][~mask]), _bits(p0[~mask])), what     # ... and only what the launch owns
            assert torch.equal(got[4], e0) != with_ema, what
            if not with_ema:
                seen.append(got[0])
    # the rate does reach the update: steps at different rates give different parameters, steps 15 and 16 (both at the
    # floor) the same ones for the optimizers whose update does not depend on the step number
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2]) and not torch.equal(seen[2], seen[3])
    if opt not in ("adam", "adamax"):
        assert torch.equal(_bits(seen[3]), _bits(seen[4]))
