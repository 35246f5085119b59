"""The EMA pass of the fused optimizer kernel (ib_optim_step_ema / ib_optim_step_sources_ema, csrc/optim.hip) on the GPU,
through hip.optim_step: all six optimizers, the plain form (with an n % 4 tail) and the gradient-sources form (slabs,
column sums with a ragged end, ranges already done = kind 3), the step number from the host, from step_dev + step and
from the self-counting ticket launch.

  * p, s1, s2 and the bf16 shadow are bitwise those of the same launch without the EMA;
  * D = 0 gives ema == p_new, D = 1 without warmup leaves ema untouched (bitwise);
  * otherwise ema is within 1 fp32 ulp of a float64 restatement of fma(d, ema, fp32((1 - d) * p_new)), with the GPU's own
    p_new and d = fp32(min(D, (1 + step) / (10 + step))) (warmup) or fp32(D) (the product is the kernel's fp32 one: where
    d * ema and (1 - d) * p_new cancel, its rounding is many ulps of the result);
  * elements the launch does not update (kind-3 ranges, the alignment padding behind a ragged column-sum range) keep
    their EMA.  -m gpu."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
OPTS = ["sgd", "adam", "rmsprop", "adagrad", "adadelta", "adamax"]
DECAYS = [(0.9, True), (0.999, False), (0.5, True), (0.0, False), (1.0, False)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def decay(D, warmup, step):
    d = min(float(D), (1.0 + step) / (10.0 + step)) if warmup else float(D)
    return float(np.float32(d))


def restated(ema0, p_new, d):
    """float64 d * ema + fp32((1 - d) * p_new), with the kernel's fp32 d and fp32 (1 - d)"""
    omd = torch.tensor(float(np.float32(1.0) - np.float32(d)), dtype=torch.float32)
    return d * ema0.double() + (omd * p_new.float()).double()


def within_one_ulp(got, ref):
    r32 = ref.float()
    ulp = (torch.nextafter(r32.abs(), torch.full_like(r32, float("inf"))) - r32.abs()).double()
    return (got.double() - ref).abs() <= ulp


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


def run_pair(opt, n, form, mode, D, warmup, seed):
    gen = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=gen).to(DEV)
    g = (torch.randn(n, generator=gen) * 1e-2).to(DEV)
    s10 = torch.rand(n, generator=gen).to(DEV) * 1e-3
    s20 = torch.rand(n, generator=gen).to(DEV) * 1e-3
    e0 = (p0 + torch.randn(n, generator=gen).to(DEV) * 1e-2).contiguous()
    if form == "sources":
        make, mask = sources_setup(n, gen)
    else:
        make, mask = (lambda grad: None), torch.ones(n, dtype=torch.bool)
    outs = []
    for with_ema in (False, True):
        p, s1, s2, e = p0.clone(), s10.clone(), s20.clone(), e0.clone()
        shadow = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
        kw = {}
        if mode == "host":
            kw, step_no = {"step": 3}, 3
        elif mode == "step_dev":
            kw, step_no = {"step": 1, "step_dev": torch.full((1,), 6, dtype=torch.int32, device=DEV)}, 7
        else:
            kw, step_no = {"step_dev": torch.full((1,), 11, dtype=torch.int32, device=DEV),
                           "ticket": torch.zeros(2048, dtype=torch.int32, device=DEV)}, 12
        if with_ema:
            kw.update(ema=e, ema_decay=D, ema_warmup=warmup)
        from inferbiomechanics_amd import hip
        hip.optim_step(opt, p, g, s1, s2, 1e-2, grad_scale=0.5, shadow=shadow, sources=make(g), **kw)
        torch.cuda.synchronize()
        if mode == "ticket":
            assert int(kw["step_dev"].cpu()) == 12 and int(kw["ticket"].abs().sum().cpu()) == 0
        outs.append((p.cpu(), s1.cpu(), s2.cpu(), shadow.cpu(), e.cpu()))
    return outs, e0.cpu(), mask, step_no


@pytest.mark.parametrize("opt", OPTS)
@pytest.mark.parametrize("form,n", [("plain", 4099), ("plain", 8192), ("sources", 8192)])
@pytest.mark.parametrize("mode", ["host", "step_dev", "ticket"])
def test_ema_pass(opt, form, n, mode):
    for k, (D, warmup) in enumerate(DECAYS):
        (off, on), e0, mask, step_no = run_pair(opt, n, form, mode, D, warmup, seed=k)
        what = (opt, form, n, mode, D, warmup)
        for a, b, nm in zip(off[:4], on[:4], ("p", "s1", "s2", "shadow")):
            assert torch.equal(_bits(a), _bits(b)), (what, nm)      # the parameter update does not see the EMA
        p_new, e = on[0], on[4]
        assert torch.equal(_bits(e[~mask]), _bits(e0[~mask])), what  # ranges this launch does not update
        em, pm, e0m = e[mask], p_new[mask], e0[mask]
        if D == 0.0:
            assert torch.equal(em, pm), what
        elif D == 1.0 and not warmup:
            assert torch.equal(_bits(em), _bits(e0m)), what
        else:
            ref = restated(e0m, pm, decay(D, warmup, step_no))
            ok = within_one_ulp(em, ref)
            assert bool(ok.all()), (what, int((~ok).sum()), float((em.double() - ref).abs().max()))
        if D not in (0.0, 1.0):
            assert not torch.equal(em, e0m) and not torch.equal(em, pm), what


def test_ema_arguments_are_checked():
    from inferbiomechanics_amd import hip
    n = 1024
    p, g = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    buf = torch.zeros(n + 4, device=DEV)
    lib = hip.lib()
    for D in (-0.1, 1.5, float("nan")):
        with pytest.raises(hip.HipError):
            hip.optim_step("sgd", p, g, None, None, 1e-2, ema=buf[:n], ema_decay=D)
        assert lib.ib_optim_step_ema(hip.OPT["sgd"], p.data_ptr(), g.data_ptr(), None, None, n, 1e-2, 1.0, 1, None, None,
                                     None, buf.data_ptr(), D, 1, hip.stream_ptr()) == -1
    with pytest.raises(hip.HipError):                                     # 4-byte aligned only
        hip.optim_step("sgd", p, g, None, None, 1e-2, ema=buf[1:n + 1], ema_decay=0.9)
    with pytest.raises(hip.HipError):
        hip.optim_step("sgd", p, g, None, None, 1e-2, ema=buf[:n - 4], ema_decay=0.9)
    torch.cuda.synchronize()
    assert int(buf.abs().sum().cpu()) == 0                                 # nothing was launched
