"""Host side of the global gradient-norm clip without a GPU: clip_coef against hand-computed values, the thirteenth header and
the build, the slot count at its edges, the argument checks of the entries, the binding's choice of entries and the trainer's
step form in dry-run mode (off: the step as ever; on: one ib_grad_sumsq and one ib_optim_step_gradnorm over the whole buffer),
the state-dict round trip, the command line, and the new kernels' registers."""
import argparse
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

NAMES = ["ib_grad_norm_eval", "ib_grad_sumsq", "ib_grad_sumsq_workspace", "ib_optim_step_gradnorm"]
WD = float(np.float32(0.1))
INF, NAN = float("inf"), float("nan")


@pytest.fixture()
def dry():
    from inferbiomechanics_amd import hip
    hip.set_dry_run(True)
    yield hip
    hip.set_dry_run(False)


def f32(x):
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the coefficient
# ---------------------------------------------------------------------------------------------------------------------
def test_clip_coef_matches_hand_computed_values():
    from inferbiomechanics_amd.grad_norm import clip_coef
    # powers of two: norm = 2^20, max_norm = 2^10; 2^10 / (2^20 + 1e-6) = 2^-10 (1 - 9.5e-13), far inside half an fp32 ulp
    assert clip_coef(2.0 ** 40, 1.0, 2.0 ** 10) == (2.0 ** 20, 2.0 ** -10, 2.0 ** -10)
    # norm 4, max_norm 2: 2 / 4.000001 = 0.499999875000031..; fp32 below 0.5 has spacing 2^-25 = 2.98e-8, the value lies
    # 4.19 spacings below 0.5: the nearest fp32 is 0.5 - 4 * 2^-25
    assert clip_coef(16.0, 1.0, 2.0) == (4.0, 0.5 - 4 * 2.0 ** -25, 0.5 - 4 * 2.0 ** -25)
    # a norm at or below max_norm - 1e-6 is not clipped: exactly 1, and gs is grad_scale
    assert clip_coef(16.0, 1.0, 8.0) == (4.0, 1.0, 1.0)
    assert clip_coef(0.0, 1.0, 1.0) == (0.0, 1.0, 1.0), "a zero gradient: 1 / 1e-6 clamps to 1"
    # torch's rule at norm == max_norm: 1 / (1 + 1e-6) = 0.999999000001, 16.78 spacings of 2^-24 below 1
    assert clip_coef(1.0, 1.0, 1.0) == (1.0, 1.0 - 17 * 2.0 ** -24, 1.0 - 17 * 2.0 ** -24)
    # max_norm = inf measures: coefficient 1 whatever the norm, also for an infinite norm (inf / inf is NaN: 1)
    assert clip_coef(1e30, 1.0, INF) == (f32(1e15), 1.0, 1.0)
    assert clip_coef(INF, 1.0, INF) == (INF, 1.0, 1.0)
    # an infinite norm under a finite max_norm: coefficient 0
    assert clip_coef(INF, 1.0, 1.0) == (INF, 0.0, 0.0)
    # NaN: the comparison fails, coefficient 1
    n, c, g = clip_coef(NAN, 0.5, 1.0)
    assert math.isnan(n) and (c, g) == (1.0, 0.5)
    # grad_scale = 0.5 (two ranks): norm = 4 * 0.5 = 2; 1 / 2.000001 = 0.49999975000012, 8.39 spacings below 0.5 -> 8;
    # gs = 0.5 * coef is exact
    assert clip_coef(16.0, 0.5, 1.0) == (2.0, 0.5 - 2.0 ** -22, 0.25 - 2.0 ** -23)
    assert clip_coef(16.0, -0.5, 1.0) == (2.0, 0.5 - 2.0 ** -22, -(0.25 - 2.0 ** -23)), "|grad_scale| in the norm"
    # fp32 values: rounding again changes nothing
    for tot, gs, mx in ((3.7, 1.0, 0.3), (1234.5, 0.25, 2.0), (1e-12, 1.0, 1e-3)):
        out = clip_coef(tot, gs, mx)
        assert out == tuple(f32(v) for v in out) and 0.0 < out[1] <= 1.0


def test_max_grad_norm_refuses_bad_values():
    from inferbiomechanics_amd.engine import HipTrainer
    from inferbiomechanics_amd.grad_norm import check_max_grad_norm
    for bad in (-0.1, NAN, "much", None):
        with pytest.raises(ValueError, match="max_grad_norm"):
            check_max_grad_norm(bad)
    assert check_max_grad_norm(0) == 0.0 and check_max_grad_norm(0.1) == WD and check_max_grad_norm(INF) == INF
    with pytest.raises(ValueError, match="max_grad_norm"):
        HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, max_grad_norm=-1.0)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the header, the build, the slot count, the argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_thirteenth_header_has_its_own_table_and_is_built():
    from inferbiomechanics_amd import hip
    assert os.path.basename(hip.GRADNORM_HEADER_PATH) == "ib_hip_gradnorm.h" and os.path.exists(hip.GRADNORM_HEADER_PATH)
    assert hip.gradnorm_decls() == NAMES == sorted(hip._GRADNORM_SIGS)
    text = open(hip.GRADNORM_HEADER_PATH).read()
    assert '#include "ib_hip_decay.h"' in text
    for n in NAMES:
        assert len(re.findall(rf"\b(?:int|size_t) {n}\(", text)) == 1
        assert n not in hip._ENTRIES, "no name collides with another header's"
        assert hip._sig(n) == hip._GRADNORM_SIGS[n]
    assert len(hip._EXPORTS) == len(hip._ENTRIES) + 4
    assert hip._is_launch("ib_grad_sumsq") and hip._is_launch("ib_optim_step_gradnorm") and hip._is_launch("ib_grad_norm_eval")
    assert not hip._is_launch("ib_grad_sumsq_workspace")
    clip = [hip._vp, hip._i64, hip._f32, hip._vp]
    assert hip._sig("ib_optim_step_gradnorm")[1] == hip._sig("ib_optim_step_decay")[1][:-1] + clip + [hip._vp]
    assert hip._sig("ib_grad_sumsq") == (hip._c.c_int, [hip._vp, hip._i64, hip._vp, hip._vp])
    assert hip._sig("ib_grad_norm_eval") == (hip._c.c_int, [hip._vp, hip._i64, hip._f32, hip._f32, hip._vp, hip._vp, hip._vp])
    assert hip._sig("ib_grad_sumsq_workspace") == (hip._sz, [hip._i64])
    mk = open(os.path.join(os.path.dirname(hip.__file__), "csrc", "Makefile")).read()
    assert re.search(r"^build/optim\.o build_ab/optim\.o: \.\./\.\./include/ib_hip_gradnorm\.h$", mk, flags=re.M)
    assert mk.index("\nall:") < mk.index("ib_hip_gradnorm.h"), "the default goal stays `all`"
    src = open(os.path.join(os.path.dirname(hip.__file__), "csrc", "optim.hip")).read()
    assert "ib_hip_gradnorm.h" in src and "clipped_optim_kernel" not in src
    assert "std::is_same<void(Sched...), void(SchedArgs, DecayArgs, ClipArgs)>::value" in src, "the clip is optim_kernel's third pack element"
    for path in (hip.LIB_PATH, hip.AB_LIB_PATH):
        if not os.path.exists(path):
            pytest.fail(f"{path} is not built")
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        assert set(NAMES) <= {line.split()[-1] for line in out.splitlines() if line.strip()}, path
    root = os.path.dirname(os.path.dirname(hip.__file__))
    for doc in ("README.md", "INTEGRATION.md"):
        assert "ib_hip_gradnorm.h" in open(os.path.join(root, doc)).read(), doc
    assert "gradnorm_decls" in open(os.path.join(root, "__graft_entry__.py")).read(), "build() checks the header's exports"


def test_slot_count_at_its_edges():
    """G(n) = clamp(ceil(n / 16384), 1, 1024), 8 bytes a slot"""
    from inferbiomechanics_amd import hip
    ws = hip.lib().ib_grad_sumsq_workspace
    S, CAP = 16384, 1024
    assert ws(0) == 0 and ws(-5) == 0
    for n, G in [(1, 1), (S - 1, 1), (S, 1), (S + 1, 2), (2 * S, 2), (2 * S + 1, 3), (CAP * S - 1, CAP), (CAP * S, CAP),
                 (CAP * S + 1, CAP), ((CAP - 1) * S, CAP - 1), ((CAP - 1) * S + 1, CAP), (1 << 40, CAP)]:
        assert ws(n) == 8 * G, n
        assert hip.grad_sumsq_slots(n) == G
        assert hip.lib().ib_grad_sumsq_workspace(hip._SUMSQ_SLOT_ELEMS * G) == 8 * G, "the n a consumer of G slots passes"


def test_argument_errors_come_before_any_launch():
    """IB_E_ARG = -1; the device pointers are never dereferenced on the host, any non-null value stands for one"""
    from inferbiomechanics_amd import hip
    lib = hip.lib()
    dev = 1 << 20
    for g, n, s in [(None, 64, dev), (dev, 64, None), (dev + 4, 64, dev), (dev, 64, dev + 8), (dev, 0, dev), (dev, -1, dev)]:
        assert lib.ib_grad_sumsq(g, n, s, None) == -1, (g, n, s)
    for a in [(None, 64, 1.0, 1.0, dev, dev), (dev, 64, 1.0, 1.0, None, dev), (dev, 64, 1.0, 1.0, dev, None),
              (dev + 8, 64, 1.0, 1.0, dev, dev), (dev, 64, 1.0, 1.0, dev + 8, dev), (dev, 64, 1.0, 1.0, dev, dev + 4),
              (dev, 0, 1.0, 1.0, dev, dev), (dev, 64, 1.0, 0.0, dev, dev), (dev, 64, 1.0, -1.0, dev, dev),
              (dev, 64, 1.0, NAN, dev, dev)]:
        assert lib.ib_grad_norm_eval(*a, None) == -1, a
    ok_s, ok_d, ok_c = (2, 5, 15, 0.1), (0.1, dev, 1, 0), (dev, 64, 1.0, dev)
    step = lambda s=ok_s, d=ok_d, c=ok_c, p=4096, opt=0, ema=(None, 0.0, 0): lib.ib_optim_step_gradnorm(
        opt, p, 8192, None, None, 64, 1e-2, 1.0, 1, None, None, None, *ema, *s, *d, *c, None)
    for c in [(None, 64, 1.0, dev), (dev + 8, 64, 1.0, dev), (dev, 0, 1.0, dev), (dev, -3, 1.0, dev), (dev, 64, 0.0, dev),
              (dev, 64, -2.0, dev), (dev, 64, NAN, dev), (dev, 64, 1.0, None), (dev, 64, 1.0, dev + 4)]:
        for s in (ok_s, (0, 0, 0, 0.0)):
            assert step(s=s, c=c) == -1, (s, c)
    # every error of the _decay entry
    for d in [(-0.1, dev, 1, 0), (NAN, dev, 1, 0), (0.1, dev, -1, 0), (0.1, None, 1, 0), (0.1, dev, 1, -4), (0.1, dev, 1, 2),
              (0.1, dev + 4, 1, 0)]:
        assert step(d=d) == -1, d
    for s in [(3, 0, 10, 0.0), (1, 5, 5, 0.0), (1, 0, 10, 1.5), (2, 0, 10, NAN), (0, -2, 0, 0.0)]:
        assert step(s=s) == -1, s
    assert step(p=None) == -1 and step(p=4100) == -1 and step(opt=7) == -1 and step(opt=1) == -1, "Adam without its states"
    assert step(ema=(12288, 1.5, 0)) == -1 and step(ema=(12292, 0.5, 0)) == -1


def test_clipped_kernels_do_not_spill_to_scratch():
    """both clip forms of optim_kernel (the two of its eighteen instantiations whose mangled name carries a ClipArgs) and the
    norm kernels compile without spills or scratch (compile only)"""
    from tools import kernel_resources as kr
    if kr.hipcc() is None:
        pytest.skip("hipcc not installed")
    rows = kr.resources("optim.hip")
    optim = [k for k in rows if k["kernel"].startswith("optim_kernel<")]
    clipped = [k for k in optim if "8ClipArgs" in k["mangled"]]
    assert len(clipped) == 2 and len(optim) == 18 and not any(k["kernel"].startswith("optim_kernel<1") for k in clipped)
    assert sorted(k["kernel"] for k in clipped) == ["optim_kernel<0,0>", "optim_kernel<0,1>"], "with and without the EMA"
    norm = [k for k in rows if k["kernel"] in ("grad_sumsq_kernel", "grad_norm_eval_kernel")]
    assert len(norm) == 2
    for k in clipped + norm:
        assert not k["vgpr_spill"] and not k["sgpr_spill"] and not k["scratch"], k
        assert k["occupancy"] >= 4, k


# ---------------------------------------------------------------------------------------------------------------------
# 3. the binding
# ---------------------------------------------------------------------------------------------------------------------
def _buffers(n=64):
    return [torch.zeros(n) for _ in range(4)]


def _sources(g):
    ws = torch.zeros(2, 16)
    return ([(ws, 2, g[16:32])], None, 0, [], [g[32:48]])


def test_binding_chooses_the_entries(dry):
    from inferbiomechanics_amd.lr_schedule import KINDS as CODES, LrSchedule
    lib = dry.lib()
    p, g, s1, s2 = _buffers()
    ema = torch.zeros(64)
    sch = LrSchedule("cosine", 5, 15, 0.1)
    four = (CODES["cosine"], 5, 15, f32(0.1))
    tab = dry.DecayTable([(0, 16), (32, 6)], "cpu")
    slots = torch.zeros(1, dtype=torch.float64)
    stats = torch.zeros(4)
    # max_grad_norm = 0: the entries of before for every combination, whatever else is given
    for kw in ({}, {"max_grad_norm": 0.0}, {"max_grad_norm": 0, "norm_slots": slots, "norm_stats": stats}):
        lib.calls.clear()
        dry.optim_step("adam", p, g, s1, s2, 1e-3, step=3, **kw)
        dry.optim_step("adam", p, g, s1, s2, 1e-3, step=3, sources=_sources(g), **kw)
        dry.optim_step("adam", p, g, s1, s2, 1e-3, step=3, ema=ema, ema_decay=0.9, **kw)
        dry.optim_step("adam", p, g, s1, s2, 1e-3, step=3, sources=_sources(g), ema=ema, ema_decay=0.9, **kw)
        dry.optim_step("adam", p, g, s1, s2, 1e-3, step=3, lr_schedule=sch, **kw)
        dry.optim_step("adam", p, g, s1, s2, 1e-3, step=3, weight_decay=0.1, decay_table=tab, **kw)
        dry.optim_step("adam", p, g, s1, s2, 1e-3, step=3, sources=_sources(g), weight_decay=0.1, decay_table=tab, **kw)
        assert lib.calls == ["ib_optim_step", "ib_optim_step_sources", "ib_optim_step_ema", "ib_optim_step_sources_ema",
                             "ib_optim_step_sched", "ib_optim_step_decay", "ib_optim_step_sources_decay"], kw
    lib.calls.clear()
    lib.ema_ranges.clear()
    kw = {"max_grad_norm": 0.5, "norm_slots": slots, "norm_stats": stats}
    tail = (slots.data_ptr(), 16384, 0.5, stats.data_ptr(), 0)
    dry.optim_step("adam", p, g, s1, s2, 1e-3, step=3, grad_scale=0.5, **kw)
    name, a = lib.args[-1]
    assert name == "ib_optim_step_gradnorm" and len(a) == 28 and a[6] == 1e-3 and a[7] == 0.5 and a[12] is None
    assert a[15:19] == (0, 0, 0, 0.0) and a[19:23] == (0.0, None, 0, 0), "no schedule, an empty decay table"
    assert a[23:] == tail
    dry.optim_step("adam", p, g, s1, s2, 1e-3, step=3, ema=ema, ema_decay=0.9, ema_warmup=False, lr_schedule=sch,
                   weight_decay=0.1, decay_table=tab, decay_origin=128, **kw)
    name, a = lib.args[-1]
    assert name == "ib_optim_step_gradnorm" and a[12:15] == (ema.data_ptr(), 0.9, 0) and a[15:19] == four
    assert a[19:23] == (0.1, tab.buf.data_ptr(), 2, 128) and a[23:] == tail
    dry.optim_step("sgd", p, g, None, None, 1e-3, step=3, max_grad_norm=INF, norm_slots=slots, norm_stats=stats)
    assert lib.args[-1][0] == "ib_optim_step_gradnorm" and lib.args[-1][1][25] == INF
    assert lib.calls == ["ib_optim_step_gradnorm"] * 3
    assert lib.ema_ranges == [(ema.data_ptr(), 64, [])], "the EMA bookkeeping of the dry run"
    n = len(lib.calls)
    for bad in ({"max_grad_norm": 0.5}, {"max_grad_norm": 0.5, "norm_slots": slots}, {"max_grad_norm": 0.5, "norm_stats": stats},
                {"max_grad_norm": -0.5, "norm_slots": slots, "norm_stats": stats},
                {"max_grad_norm": NAN, "norm_slots": slots, "norm_stats": stats},
                {"max_grad_norm": 0.5, "norm_slots": slots.float(), "norm_stats": stats},
                {"max_grad_norm": 0.5, "norm_slots": slots, "norm_stats": stats[:2]},
                {"max_grad_norm": 0.5, "norm_slots": slots, "norm_stats": stats, "sources": _sources(g)}):
        with pytest.raises(dry.HipError):
            dry.optim_step("adam", p, g, s1, s2, 1e-3, step=3, **bad)
    assert len(lib.calls) == n, "a refused call launches nothing"
    # the wrappers of the norm pass and the probe
    big = torch.zeros(16385)
    sl = dry.grad_sumsq(big)
    assert sl.dtype == torch.float64 and sl.numel() == 2 and lib.args[-1] == ("ib_grad_sumsq", (big.data_ptr(), 16385, sl.data_ptr(), 0))
    total, st = dry.grad_norm_eval(sl, 0.5, 2.0)
    name, a = lib.args[-1]
    assert name == "ib_grad_norm_eval" and a[:4] == (sl.data_ptr(), 2 * 16384, 0.5, 2.0) and total.dtype == torch.float64
    assert total.numel() == 1 and st.numel() == 3 and st.dtype == torch.float32
    for bad in (lambda: dry.grad_sumsq(big, torch.zeros(3, dtype=torch.float64)), lambda: dry.grad_sumsq(big.double()),
                lambda: dry.grad_sumsq(torch.zeros(0)), lambda: dry.grad_norm_eval(sl, 1.0, 0.0),
                lambda: dry.grad_norm_eval(sl.float(), 1.0, 1.0)):
        with pytest.raises(dry.HipError):
            bad()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the trainer
# ---------------------------------------------------------------------------------------------------------------------
def _mlp():
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionMLP
    torch.manual_seed(0)
    return DiffusionMLP(30, [32, 48], temb_dim=16, temb_hidden=24)


def _transformer():
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    torch.manual_seed(0)
    return DiffusionTransformer(48, 32, d_model=512, num_heads=4, dim_feedforward=1024, num_layers=3, compute_dtype=torch.bfloat16)


def _batch(B=3, T=7, D=30, dt=torch.float32):
    g = torch.Generator().manual_seed(1)
    return (torch.randn(B, T, D, generator=g).to(dt), torch.randint(0, 1000, (B,), generator=g), torch.randn(B, T, D, generator=g).to(dt))


MODELS = {"mlp": (_mlp, lambda: _batch()), "transformer": (_transformer, lambda: _batch(128, 32, 48, torch.bfloat16))}


def _step_calls(hip, tr, batch):
    lib = hip.lib()
    lib.calls.clear()
    del lib.args[:]
    tr.step(batch)
    return list(lib.calls), [(n, a) for n, a in lib.args if n.startswith("ib_optim_step")]


def test_max_grad_norm_zero_is_the_trainer_without_the_argument(dry):
    from inferbiomechanics_amd.engine import HipTrainer
    for model in sorted(MODELS):
        mk, mb = MODELS[model]
        batch = mb()

        def norm(tr):
            names, opt = _step_calls(dry, tr, batch)
            p0 = tr.flat.data_ptr()
            return names, [(n, (a[1] - p0), a[5:9], len(a)) for n, a in opt]
        want = norm(HipTrainer(mk(), "diffusion", "adam", 1e-3, use_graph=False))
        for kw in (dict(max_grad_norm=0.0), dict(max_grad_norm=0)):
            tr = HipTrainer(mk(), "diffusion", "adam", 1e-3, use_graph=False, **kw)
            assert norm(tr) == want and not tr.clip and tr.norm_slots is None and tr.norm_stats is None, (model, kw)
            assert not any(n.startswith("ib_grad_") or "gradnorm" in n for n in want[0]), "no new launch"
            with pytest.raises(dry.HipError, match="max_grad_norm = 0"):
                tr.grad_norm()


@pytest.mark.parametrize("model", sorted(MODELS))
def test_clipped_step_is_one_norm_pass_and_one_launch_over_the_whole_buffer(dry, model):
    from inferbiomechanics_amd.engine import HipTrainer
    from inferbiomechanics_amd.lr_schedule import LrSchedule
    mk, mb = MODELS[model]
    batch = mb()
    plain = HipTrainer(mk(), "diffusion", "adam", 1e-3, use_graph=False)
    names_plain, opt_plain = _step_calls(dry, plain, batch)
    if model == "transformer":
        assert len(opt_plain) > 1 and any("_sources" in n for n in names_plain), "the step this one gives up"
    for mgn, kw in ((0.5, dict()), (INF, dict(ema_decay=0.999)),
                    (0.5, dict(lr_schedule=LrSchedule("cosine", 5, 15, 0.1), ema_decay=0.999, weight_decay=0.1))):
        tr = HipTrainer(mk(), "diffusion", "adam", 1e-3, use_graph=False, max_grad_norm=mgn, **kw)
        n = tr.flat.numel()
        assert tr.clip and tr.norm_slots.numel() == dry.grad_sumsq_slots(n) and tr.norm_slots.dtype == torch.float64
        assert not tr.bucket_opt
        for _ in range(2):
            names, opt = _step_calls(dry, tr, batch)
            assert not any("_sources" in k for k in names), "every gradient is materialised"
            assert names.count("ib_grad_sumsq") == 1 and names[-2:] == ["ib_grad_sumsq", "ib_optim_step_gradnorm"]
            assert [k for k, _ in opt] == ["ib_optim_step_gradnorm"], "no early launches"
            assert tr.plan.fuse_reduce_into_optimizer is False and getattr(tr.plan, "early_optimizer", None) is None
            sq = [a for k, a in dry.lib().args if k == "ib_grad_sumsq"][0]
            assert sq[:3] == (tr.grad.data_ptr(), n, tr.norm_slots.data_ptr())
            a = opt[0][1]
            assert (a[1], a[2], a[5]) == (tr.flat.data_ptr(), tr.grad.data_ptr(), n), "over [0, n)"
            assert a[7] == 1.0 and a[8] == 0 and a[9] == tr.step_dev.data_ptr() and a[10] == tr.ticket.data_ptr()
            assert a[23:27] == (tr.norm_slots.data_ptr(), 16384 * tr.norm_slots.numel(), mgn, tr.norm_stats.data_ptr())
            assert a[12:15] == ((tr.ema.data_ptr(), 0.999, 1) if "ema_decay" in kw else (None, 0.0, 1))
            assert a[15:19] == ((2, 5, 15, f32(0.1)) if "lr_schedule" in kw else (0, 0, 0, 0.0))
            assert a[19:23] == ((WD, tr.decay_table.buf.data_ptr(), tr.decay_table.n, 0) if "weight_decay" in kw else (0.0, None, 0, 0))
            if model == "transformer":
                assert a[11] == tr.model._shadow.data_ptr(), "the bf16 shadow is refreshed by the same launch"


def test_trainer_state_dict_round_trip_of_the_clip(dry):
    from inferbiomechanics_amd.engine import HipTrainer
    tr = HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, max_grad_norm=0.1)
    for _ in range(3):
        tr.step(_batch())
    sd = tr.optimizer_state_dict()
    assert sd["max_grad_norm"] == WD and sd["step"] == 3
    again = HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, max_grad_norm=0.1)
    again.load_optimizer_state_dict(sd)
    assert again.steps_done == 3
    for other in (dict(), dict(max_grad_norm=0.0), dict(max_grad_norm=0.2), dict(max_grad_norm=INF)):
        t2 = HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, **other)
        with pytest.raises(dry.HipError, match=r"the checkpoint's gradient-norm clip \(0\.1\) differs from this trainer's \((0|0\.2|inf)\)"):
            t2.load_optimizer_state_dict(sd)
        assert t2.steps_done == 0, "nothing was loaded"
    plain = HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False)
    plain_sd = plain.optimizer_state_dict()
    assert plain_sd["max_grad_norm"] == 0.0
    with pytest.raises(dry.HipError, match=r"gradient-norm clip \(0\) differs from this trainer's \(0\.1\)"):
        again.load_optimizer_state_dict(plain_sd)
    # a payload without the key is an older checkpoint: it counts as 0
    old = {k: v for k, v in plain_sd.items() if k != "max_grad_norm"}
    HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False).load_optimizer_state_dict(old)
    with pytest.raises(dry.HipError, match=r"gradient-norm clip \(0\) differs"):
        again.load_optimizer_state_dict(old)
    inf_tr = HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, max_grad_norm=INF)
    HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, max_grad_norm=INF).load_optimizer_state_dict(inf_tr.optimizer_state_dict())
    # torch.optim's grammar is as it was
    tsd = tr.torch_optimizer_state_dict()
    assert set(tsd) == {"state", "param_groups"}
    assert tsd["param_groups"] == plain.torch_optimizer_state_dict()["param_groups"]


# ---------------------------------------------------------------------------------------------------------------------
# 5. the command line
# ---------------------------------------------------------------------------------------------------------------------
def _train(*a):
    from inferbiomechanics_amd.cli.train import TrainCommand
    p = argparse.ArgumentParser()
    TrainCommand().register_subcommand(p.add_subparsers(dest="command"))
    return p.parse_args(["train"] + list(a))


def test_cli_flag_default_and_refusals():
    from inferbiomechanics_amd.cli.train import check_max_grad_norm_args
    assert _train().max_grad_norm == 0.0
    check_max_grad_norm_args(_train())
    check_max_grad_norm_args(_train("--eager"))
    check_max_grad_norm_args(_train("--max-grad-norm", "0", "--eager"))
    check_max_grad_norm_args(_train("--max-grad-norm", "1.0"))
    check_max_grad_norm_args(_train("--max-grad-norm", "inf"))
    with pytest.raises(SystemExit, match="--max-grad-norm needs the fused trainer: --eager"):
        check_max_grad_norm_args(_train("--max-grad-norm", "1.0", "--eager"))
    for bad in ("-0.1", "nan"):
        with pytest.raises(SystemExit, match="--max-grad-norm must be >= 0 and not NaN"):
            check_max_grad_norm_args(_train("--max-grad-norm", bad))


BASE = ['--no-wandb', '--synthetic-windows', '24', '--batch-size', '8', '--data-loading-workers', '0', '--model-type',
        'diffusion-mlp', '--feat-dim', '24', '--hidden-dims', '32', '32', '--stride', '1', '--history-len', '6', '--seed', '7']


def test_train_with_max_grad_norm_in_dry_run(dry, tmp_path, capsys):
    """a clipped run from start to resume: refused with --eager before anything is written, every step one norm pass and one
    clipped launch with the flag's value, the checkpoint carries it, a resumed run with another value is refused"""
    from inferbiomechanics_amd.main import main
    lib = dry.lib()
    d = str(tmp_path / "ck")
    with pytest.raises(SystemExit, match="--max-grad-norm needs the fused trainer"):
        main(['train', '--epochs', '1', '--checkpoint-dir', d, '--eager', '--max-grad-norm', '0.1'] + BASE)
    with pytest.raises(SystemExit, match="--max-grad-norm must be >= 0"):
        main(['train', '--epochs', '1', '--checkpoint-dir', d, '--max-grad-norm', '-1'] + BASE)
    assert not os.path.exists(d), "refused before anything was written"
    lib.calls.clear()
    del lib.args[:]
    assert main(['train', '--epochs', '1', '--checkpoint-dir', d, '--max-grad-norm', '0.1', '--opt-type', 'adam'] + BASE)
    opt = [(n, a) for n, a in lib.args if n.startswith("ib_optim_step")]
    assert len(opt) >= 3 and all(n == "ib_optim_step_gradnorm" and a[25] == WD for n, a in opt)
    assert lib.calls.count("ib_grad_sumsq") == len(opt)
    out = capsys.readouterr().out
    assert "Gradient clipping: global L2 norm at most 0.1" in out
    assert re.search(r"gradient norm \S+, clip coefficient \S+", out), "the report line"
    ck = torch.load(os.path.join(d, "diffusion-mlp", "epoch_0_batch_2.pt"), map_location="cpu")
    assert ck["optimizer_state_dict"]["max_grad_norm"] == WD
    with pytest.raises(SystemExit, match=r"gradient-norm clip \(0\.1\) differs from this trainer's \(0\.2\).*same --max-grad-norm"):
        main(['train', '--epochs', '2', '--checkpoint-dir', d, '--max-grad-norm', '0.2', '--opt-type', 'adam'] + BASE)
    with pytest.raises(SystemExit, match=r"gradient-norm clip \(0\.1\) differs from this trainer's \(0\)"):
        main(['train', '--epochs', '2', '--checkpoint-dir', d, '--opt-type', 'adam'] + BASE)
    lib.calls.clear()
    assert main(['train', '--epochs', '2', '--checkpoint-dir', d, '--max-grad-norm', '0.1', '--opt-type', 'adam'] + BASE)
    assert "ib_optim_step_gradnorm" in lib.calls
    lib.calls.clear()
    assert main(['train', '--epochs', '1', '--checkpoint-dir', str(tmp_path / "plain")] + BASE)
    assert not any(n.startswith("ib_grad_") or "gradnorm" in n for n in lib.calls)
