"""Host side of the learning-rate schedule without a GPU: LrSchedule.lr_at against hand-computed values and its identities,
the field checks, the binding's choice of entry point in dry-run mode (the four old entries for None and a constant schedule,
the `_sched` entries with the schedule's four numbers otherwise), the tenth header and the build lists, the argument checks
of the three entries, the command line's flags and refusals, and the trainer's state-dict round trip."""
import argparse
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

NAMES = ["ib_lr_schedule_eval", "ib_optim_step_sched", "ib_optim_step_sources_sched"]
KINDS = ["constant", "linear", "cosine"]
STEPS = [1, 4, 5, 6, 10, 14, 15, 16, 1015]
M01 = float(np.float32(0.1))                      # min_ratio is held as the fp32 value the kernel receives


@pytest.fixture()
def dry():
    from inferbiomechanics_amd import hip
    hip.set_dry_run(True)
    yield hip
    hip.set_dry_run(False)


def f32(x):
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the schedule itself
# ---------------------------------------------------------------------------------------------------------------------
# the factor f of w = 5, T = 15 at STEPS, worked out by hand (decimal arithmetic, 12 places): u = (s - 5) / 10 is 0.1, 0.5, 0.9
# at s = 6, 10, 14; (1 + cos(0.1 pi)) / 2 = 0.975528258148, (1 + cos(0.9 pi)) / 2 = 0.024471741852; m = fp32(0.1)
WARM = [0.2, 0.8, 1.0]
HAND = {
    ("constant", 0.0): WARM + [1.0] * 6, ("constant", M01): WARM + [1.0] * 6, ("constant", 1.0): WARM + [1.0] * 6,
    ("linear", 0.0): WARM + [0.9, 0.5, 0.1, 0.0, 0.0, 0.0],
    ("cosine", 0.0): WARM + [0.975528258148, 0.5, 0.024471741852, 0.0, 0.0, 0.0],
    ("linear", M01): WARM + [0.910000000149, 0.550000000745, 0.190000001341, 0.100000001490, 0.100000001490, 0.100000001490],
    ("cosine", M01): WARM + [0.977975432369, 0.550000000745, 0.122024569121, 0.100000001490, 0.100000001490, 0.100000001490],
    ("linear", 1.0): WARM + [1.0] * 6, ("cosine", 1.0): WARM + [1.0] * 6,
}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m", [0.0, 0.1, 1.0])
def test_lr_at_matches_hand_computed_values(kind, m):
    from inferbiomechanics_amd.lr_schedule import LrSchedule
    sch = LrSchedule(kind, 5, 15, m)
    assert sch.min_ratio == f32(m)
    for s, f in zip(STEPS, HAND[(kind, f32(m))]):
        assert sch.lr_at(1.0, s) == f32(f), (kind, m, s)
        assert sch.lr_at(0.5, s) == f32(0.5 * f), (kind, m, s)          # a power of two scales exactly
        # any base rate: two fp32 roundings (the rate, the result: 2^-24 each, relative) and the table's 12 places
        got = sch.lr_at(3e-4, s)
        assert got == f32(got) and abs(got - 3e-4 * f) <= 2.0 ** -23 * 1.001 * 3e-4 * f + 3e-4 * 1e-12, (kind, m, s)


def test_edges_no_warmup_late_warmup_and_a_huge_step():
    from inferbiomechanics_amd.lr_schedule import LrSchedule
    lr = 1e-3
    # w = 0: the first step is already past the warmup (no 0 / 0)
    assert LrSchedule("constant", 0, 0, 0.0).lr_at(lr, 1) == f32(lr)
    lin = LrSchedule("linear", 0, 10, 0.0)
    assert lin.lr_at(1.0, 1) == f32(0.9) and lin.lr_at(1.0, 5) == 0.5 and lin.lr_at(1.0, 10) == 0.0
    cos = LrSchedule("cosine", 0, 10, 0.25)
    assert cos.lr_at(1.0, 5) == f32(0.25 + 0.75 * 0.5 * (1.0 + math.cos(math.pi * 0.5))) and cos.lr_at(1.0, 10) == 0.25
    # w = T - 1: the decay is the single step T
    for kind in ("linear", "cosine"):
        late = LrSchedule(kind, 14, 15, 0.5)
        assert late.lr_at(1.0, 14) == 1.0 and late.lr_at(1.0, 13) == f32(13 / 14) and late.lr_at(1.0, 15) == 0.5
    # s near 2^31: s - w is formed without overflow, the clamp holds
    big = 2_000_000_000
    for kind in KINDS:
        sch = LrSchedule(kind, 5, 15, 0.1)
        assert sch.lr_at(lr, big) == (f32(lr) if kind == "constant" else f32(f32(lr) * M01))
    ramp = LrSchedule("linear", 2_000_000_000, 2_100_000_000, 0.0)
    assert ramp.lr_at(1.0, 1_000_000_000) == 0.5 and ramp.lr_at(1.0, 2_050_000_000) == 0.5


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w,T,m", [(5, 15, 0.0), (5, 15, 0.1), (100, 1000, 0.01), (1, 2, 0.5), (7, 8, 1.0)])
def test_identities_and_monotonicity(kind, w, T, m):
    from inferbiomechanics_amd.lr_schedule import LrSchedule
    sch = LrSchedule(kind, w, T, m)
    for lr in (1.0, 1e-4, 3e-3):
        assert sch.lr_at(lr, 1) == f32(f32(lr) / w)                     # step 1 runs at lr / w
        assert sch.lr_at(lr, w) == f32(lr)                              # step w at lr
        if kind != "constant":
            for s in (T, T + 1, 10 * T):
                assert sch.lr_at(lr, s) == f32(sch.min_ratio * f32(lr)), (s,)   # step T and later at m lr
    fs = [sch.factor(s) for s in range(1, T + 3)]
    assert all(b > a for a, b in zip(fs[:w - 1], fs[1:w])), "rising through the warmup"
    tail = fs[w - 1:]
    assert all(b <= a for a, b in zip(tail, tail[1:])), "never rising after it"
    if kind != "constant" and m < 1.0:
        assert all(b < a for a, b in zip(tail[:T - w], tail[1:T - w + 1])), "falling through the decay"
    assert all(0.0 <= f <= 1.0 for f in fs)


def test_min_ratio_one_is_constant_with_warmup_bitwise():
    from inferbiomechanics_amd.lr_schedule import LrSchedule
    ref = LrSchedule("constant", 5, 0, 0.0)
    for kind in ("linear", "cosine"):
        sch = LrSchedule(kind, 5, 15, 1.0)
        for lr in (1.0, 1e-3, 7e-5):
            for s in STEPS + [2, 3, 7, 11]:
                assert np.float32(sch.lr_at(lr, s)).view(np.int32) == np.float32(ref.lr_at(lr, s)).view(np.int32), (kind, lr, s)


def test_schedule_refuses_bad_fields():
    from inferbiomechanics_amd.lr_schedule import LrSchedule, active
    for bad in (lambda: LrSchedule("exp", 0, 10, 0.0), lambda: LrSchedule(1, 0, 10, 0.0), lambda: LrSchedule("linear", -1, 10, 0.0),
                lambda: LrSchedule("linear", 5, 5, 0.0), lambda: LrSchedule("cosine", 5, 4, 0.0), lambda: LrSchedule("cosine", 0, 0, 0.0),
                lambda: LrSchedule("linear", 0, 10, -0.1), lambda: LrSchedule("linear", 0, 10, 1.5),
                lambda: LrSchedule("linear", 0, 10, float("nan")), lambda: LrSchedule("linear", 0.5, 10, 0.0),
                lambda: LrSchedule("linear", 0, 1 << 31, 0.0), lambda: LrSchedule("constant", True, 0, 0.0),
                lambda: LrSchedule("linear", 0, 10, "low")):
        with pytest.raises(ValueError):
            bad()
    assert LrSchedule().is_constant() and LrSchedule("constant", 0, 99, 0.3).is_constant()
    assert not LrSchedule("constant", 1, 0, 0.0).is_constant() and not LrSchedule("linear", 0, 10, 1.0).is_constant()
    assert active(None) is None and active(LrSchedule()) is None
    sch = LrSchedule("cosine", 100, 1000, 0.1)
    assert active(sch) is sch and LrSchedule.from_fields(sch.fields()) == sch and LrSchedule.from_fields(None) is None
    assert sch.fields() == {"kind": "cosine", "warmup": 100, "total": 1000, "min_ratio": M01}
    assert (sch.kind_code, LrSchedule("linear", 0, 1, 0.0).kind_code, LrSchedule().kind_code) == (2, 1, 0)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the header, the build lists, the argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_tenth_header_has_its_own_table_and_is_built():
    from inferbiomechanics_amd import hip
    assert os.path.basename(hip.SCHED_HEADER_PATH) == "ib_hip_sched.h" and os.path.exists(hip.SCHED_HEADER_PATH)
    assert hip.sched_decls() == NAMES == sorted(hip._SCHED_SIGS)
    text = open(hip.SCHED_HEADER_PATH).read()
    for n in NAMES:
        assert len(re.findall(rf"\bint {n}\(", text)) == 1
        assert n not in hip._ALL_SIGS, "no name collides with another header's"
        res, args = hip._sig(n)
        assert res is hip._c.c_int and args[-1] is hip._vp and hip._is_launch(n)
    assert len(hip._BOUND) == len(hip._ALL_SIGS) + 3
    sched = [hip._c.c_int, hip._i32, hip._i32, hip._f32]
    assert hip._sig("ib_optim_step_sched")[1] == hip._sig("ib_optim_step_ema")[1][:-1] + sched + [hip._vp]
    assert hip._sig("ib_optim_step_sources_sched")[1] == hip._sig("ib_optim_step_sources_ema")[1][:-1] + sched + [hip._vp]
    assert hip._sig("ib_lr_schedule_eval")[1] == [hip._f32] + sched + [hip._vp, hip._vp, hip._i64, hip._vp]
    consts = dict(re.findall(r"^#define (IB_SCHED_[A-Z]+) (\d+)$", text, flags=re.M))
    from inferbiomechanics_amd.lr_schedule import KINDS as CODES
    assert {k: int(v) for k, v in consts.items()} == {f"IB_SCHED_{k.upper()}": v for k, v in CODES.items()}
    mk = open(os.path.join(os.path.dirname(hip.__file__), "csrc", "Makefile")).read()
    hdrs = re.search(r"^HDRS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "../../include/ib_hip_sched.h" in hdrs and len([h for h in hdrs if h.startswith("../../include/")]) == 10
    for path in (hip.LIB_PATH, hip.AB_LIB_PATH):
        if not os.path.exists(path):
            pytest.fail(f"{path} is not built")
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        assert set(NAMES) <= {line.split()[-1] for line in out.splitlines() if line.strip()}, path
    root = os.path.dirname(os.path.dirname(hip.__file__))
    for doc in ("README.md", "INTEGRATION.md"):
        assert "ib_hip_sched.h" in open(os.path.join(root, doc)).read(), doc
    assert "sched_decls" in open(os.path.join(root, "__graft_entry__.py")).read(), "build() checks the tenth header's exports"


def test_argument_errors_come_before_any_launch():
    """IB_E_ARG = -1; the pointers are never dereferenced on the host, any non-null value stands for one"""
    from inferbiomechanics_amd import hip
    lib = hip.lib()
    nan = float("nan")
    bad = [(3, 0, 10, 0.0), (-1, 0, 10, 0.0), (1, -1, 10, 0.0), (1, 5, 5, 0.0), (2, 5, 4, 0.0), (2, 0, 0, 0.0),
           (1, 0, 10, -0.01), (1, 0, 10, 1.01), (2, 0, 10, nan), (0, 0, 0, nan), (0, -2, 0, 0.0)]
    for kind, w, T, m in bad:
        assert lib.ib_lr_schedule_eval(1e-3, kind, w, T, m, 4096, 8192, 4, None) == -1, (kind, w, T, m)
        assert lib.ib_optim_step_sched(0, 4096, 8192, None, None, 64, 1e-2, 1.0, 1, None, None, None, None, 0.0, 0,
                                       kind, w, T, m, None) == -1, (kind, w, T, m)
        assert lib.ib_optim_step_sources_sched(0, 4096, 8192, None, None, 64, 1e-2, 1.0, 1, None, None, None, 0, None, None,
                                               None, None, None, None, None, None, 0, 0, 0.0, None, None, 0.0, 0,
                                               kind, w, T, m, None) == -1, (kind, w, T, m)
    ok = (2, 5, 15, 0.1)
    assert lib.ib_lr_schedule_eval(1e-3, *ok, None, 8192, 4, None) == -1
    assert lib.ib_lr_schedule_eval(1e-3, *ok, 4096, None, 4, None) == -1
    assert lib.ib_lr_schedule_eval(1e-3, *ok, 4096, 8192, 0, None) == -1
    # a good schedule does not excuse the optimizer's own checks, nor a bad EMA (a 4-byte aligned one, a decay of 1.5)
    assert lib.ib_optim_step_sched(0, None, 8192, None, None, 64, 1e-2, 1.0, 1, None, None, None, None, 0.0, 0, *ok, None) == -1
    assert lib.ib_optim_step_sched(0, 4096, 8192, None, None, 64, 1e-2, 1.0, 1, None, None, None, 4100, 0.5, 0, *ok, None) == -1
    assert lib.ib_optim_step_sched(0, 4096, 8192, None, None, 64, 1e-2, 1.0, 1, None, None, None, 12288, 1.5, 0, *ok, None) == -1


def test_scheduled_kernels_do_not_spill_and_keep_the_occupancy():
    """the instantiations with a SchedArgs behind main_blocks compile without spills or scratch, at the occupancy of the
    ones without (compile only, a few seconds)"""
    from tools import kernel_resources as kr
    if kr.hipcc() is None:
        pytest.skip("hipcc not installed")
    rows = [k for k in kr.resources("optim.hip") if k["kernel"].startswith("optim_kernel<")]
    sched = {k["kernel"]: k for k in rows if "SchedArgs" in k["mangled"]}
    plain = {k["kernel"]: k for k in rows if "SchedArgs" not in k["mangled"]}
    assert sorted(sched) == sorted(plain) == ["optim_kernel<0,0>", "optim_kernel<0,1>", "optim_kernel<1,0>", "optim_kernel<1,1>"]
    for name, k in sched.items():
        assert not k["vgpr_spill"] and not k["sgpr_spill"] and not k["scratch"], k
        assert k["occupancy"] == plain[name]["occupancy"], (k, plain[name])


# ---------------------------------------------------------------------------------------------------------------------
# 3. the binding
# ---------------------------------------------------------------------------------------------------------------------
def _buffers(n=64):
    return [torch.zeros(n) for _ in range(4)]


def _sources(g):
    ws = torch.zeros(2, 16)
    return ([(ws, 2, g[16:32])], None, 0, [], [g[32:48]])


def test_binding_reaches_the_old_entries_without_a_schedule(dry):
    from inferbiomechanics_amd.lr_schedule import LrSchedule
    lib = dry.lib()
    p, g, s1, s2 = _buffers()
    ema = torch.zeros(64)
    for sch in (None, LrSchedule(), LrSchedule("constant", 0, 500, 0.5)):
        kw = {} if sch is None else {"lr_schedule": sch}
        lib.calls.clear()
        dry.optim_step("adam", p, g, s1, s2, 1e-3, step=3, **kw)
        dry.optim_step("adam", p, g, s1, s2, 1e-3, step=3, sources=_sources(g), **kw)
        dry.optim_step("adam", p, g, s1, s2, 1e-3, step=3, ema=ema, ema_decay=0.9, **kw)
        dry.optim_step("adam", p, g, s1, s2, 1e-3, step=3, sources=_sources(g), ema=ema, ema_decay=0.9, **kw)
        assert lib.calls == ["ib_optim_step", "ib_optim_step_sources", "ib_optim_step_ema", "ib_optim_step_sources_ema"], sch
    with pytest.raises(dry.HipError, match="LrSchedule"):
        dry.optim_step("adam", p, g, s1, s2, 1e-3, step=3, lr_schedule=("cosine", 5, 15, 0.1))


@pytest.mark.parametrize("sch_args", [("cosine", 5, 15, 0.1), ("linear", 0, 9, 0.0), ("constant", 3, 0, 0.0)])
def test_binding_reaches_the_sched_entries_with_the_four_numbers(dry, sch_args):
    from inferbiomechanics_amd.lr_schedule import KINDS as CODES, LrSchedule
    lib = dry.lib()
    sch = LrSchedule(*sch_args)
    four = (CODES[sch_args[0]], sch_args[1], sch_args[2], f32(sch_args[3]))
    p, g, s1, s2 = _buffers()
    ema = torch.zeros(64)
    step_dev, ticket = torch.zeros(1, dtype=torch.int32), torch.zeros(dry.optim_ticket_words(), dtype=torch.int32)
    lib.calls.clear()
    del lib.args[:]
    lib.ema_ranges.clear()
    dry.optim_step("adam", p, g, s1, s2, 1e-3, step=3, lr_schedule=sch)
    name, a = lib.args[-1]
    assert name == "ib_optim_step_sched" and len(a) == 20
    assert a[:6] == (dry.OPT["adam"], p.data_ptr(), g.data_ptr(), s1.data_ptr(), s2.data_ptr(), 64) and a[6] == 1e-3, "the base rate"
    assert a[8:12] == (3, None, None, None) and a[12] is None and a[15:19] == four and a[19] == 0
    dry.optim_step("adam", p, g, s1, s2, 1e-3, step_dev=step_dev, ticket=ticket, ema=ema, ema_decay=0.9, ema_warmup=False,
                   lr_schedule=sch)
    name, a = lib.args[-1]
    assert name == "ib_optim_step_sched" and a[8:11] == (0, step_dev.data_ptr(), ticket.data_ptr())
    assert a[12:15] == (ema.data_ptr(), 0.9, 0) and a[15:19] == four
    dry.optim_step("adam", p, g, s1, s2, 1e-3, step=1, step_dev=step_dev, sources=_sources(g), lr_schedule=sch)
    name, a = lib.args[-1]
    assert name == "ib_optim_step_sources_sched" and len(a) == 33 and a[12] == 2 and a[25] is None and a[28:32] == four
    dry.optim_step("adam", p, g, s1, s2, 1e-3, step=1, step_dev=step_dev, sources=_sources(g), ema=ema, ema_decay=0.5,
                   lr_schedule=sch)
    name, a = lib.args[-1]
    assert name == "ib_optim_step_sources_sched" and a[25:28] == (ema.data_ptr(), 0.5, 1) and a[28:32] == four
    assert lib.calls == ["ib_optim_step_sched"] * 2 + ["ib_optim_step_sources_sched"] * 2
    # the dry run keeps the EMA bookkeeping of the scheduled launches: the two with an EMA, the second with its kind-3 range
    assert lib.ema_ranges == [(ema.data_ptr(), 64, []), (ema.data_ptr(), 64, [(32, 16)])]
    steps = torch.tensor([1, 5, 6], dtype=torch.int32)
    out = dry.lr_schedule_eval(1e-3, sch, steps)
    assert lib.args[-1] == ("ib_lr_schedule_eval", (1e-3,) + four + (steps.data_ptr(), out.data_ptr(), 3, 0))
    assert out.dtype == torch.float32 and tuple(out.shape) == (3,)
    n = len(lib.calls)
    for bad in (lambda: dry.lr_schedule_eval(1e-3, None, steps), lambda: dry.lr_schedule_eval(1e-3, sch, steps.long()),
                lambda: dry.lr_schedule_eval(1e-3, sch, steps[:0]), lambda: dry.lr_schedule_eval(1e-3, sch, steps, out=out[:2]),
                lambda: dry.lr_schedule_eval(1e-3, sch, steps, out=out.double())):
        with pytest.raises(dry.HipError):
            bad()
    assert len(lib.calls) == n, "a refused call launches nothing"


# ---------------------------------------------------------------------------------------------------------------------
# 4. the trainer
# ---------------------------------------------------------------------------------------------------------------------
def _mlp():
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionMLP
    torch.manual_seed(0)
    return DiffusionMLP(30, [32, 48], temb_dim=16, temb_hidden=24)


def _batch(B=3, T=7, D=30):
    g = torch.Generator().manual_seed(1)
    return (torch.randn(B, T, D, generator=g), torch.randint(0, 1000, (B,), generator=g), torch.randn(B, T, D, generator=g))


def _step_names(hip, tr):
    lib = hip.lib()
    lib.calls.clear()
    del lib.args[:]
    tr.step(_batch())
    return list(lib.calls), [a for n, a in lib.args if n.startswith("ib_optim_step")]


def test_trainer_passes_the_schedule_at_every_optimizer_launch(dry):
    from inferbiomechanics_amd.engine import HipTrainer
    from inferbiomechanics_amd.lr_schedule import LrSchedule
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    sch = LrSchedule("cosine", 5, 15, 0.1)
    plain = HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False)
    names_plain, _ = _step_names(dry, plain)
    for off in (None, LrSchedule(), LrSchedule("constant", 0, 77, 0.2)):
        tr = HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, lr_schedule=off)
        assert _step_names(dry, tr)[0] == names_plain and tr._sched_args() == {} and tr.current_lr() == 1e-3
        assert tr.optimizer_state_dict()["lr_schedule"] is None
    tr = HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, lr_schedule=sch)
    assert tr._sched_args() == {"lr_schedule": sch}
    for k in range(3):
        assert tr.current_lr() == sch.lr_at(1e-3, k + 1) and tr.steps_done == k
        names, opt_args = _step_names(dry, tr)
        assert [re.sub(r"_sched$", "", n) for n in names] == names_plain, "the same launches, no new ones"
        assert sum(n.endswith("_sched") for n in names) == len(opt_args) >= 1
        assert all(a[-5:-1] == (2, 5, 15, M01) and a[6] == 1e-3 for a in opt_args), "the base rate and the four numbers"
    # the transformer's per-layer launches from the backward and its last, self-counting launch: all scheduled, EMA or not
    mk = lambda: DiffusionTransformer(48, 32, d_model=512, num_heads=4, dim_feedforward=1024, num_layers=3,
                                      compute_dtype=torch.bfloat16)
    g = torch.Generator().manual_seed(1)
    batch = (torch.randn(128, 32, 48, generator=g).to(torch.bfloat16), torch.randint(0, 1000, (128,), generator=g),
             torch.randn(128, 32, 48, generator=g).to(torch.bfloat16))
    lib = dry.lib()
    seen = {}
    for kw in (dict(), dict(lr_schedule=sch), dict(lr_schedule=sch, ema_decay=0.999)):
        torch.manual_seed(0)
        t = HipTrainer(mk(), "diffusion", "adam", 1e-3, use_graph=False, **kw)
        lib.calls.clear()
        t.step(batch)
        seen[tuple(sorted(kw))] = [n for n in lib.calls]
    base, on, on_ema = seen[()], seen[("lr_schedule",)], seen[("ema_decay", "lr_schedule")]
    assert [re.sub(r"_sched$", "", n) for n in on] == base and on == on_ema
    assert sum(n.startswith("ib_optim_step") for n in base) > 1 and not any(n in ("ib_optim_step", "ib_optim_step_sources") for n in on)
    with pytest.raises(ValueError, match="LrSchedule"):
        HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, lr_schedule="cosine")


def test_trainer_state_dict_round_trip_of_the_schedule(dry):
    from inferbiomechanics_amd.engine import HipTrainer
    from inferbiomechanics_amd.lr_schedule import LrSchedule
    sch = LrSchedule("cosine", 5, 15, 0.1)
    tr = HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, lr_schedule=sch)
    for _ in range(4):
        tr.step(_batch())
    sd = tr.optimizer_state_dict()
    assert sd["lr_schedule"] == {"kind": "cosine", "warmup": 5, "total": 15, "min_ratio": M01} and sd["lr"] == 1e-3 and sd["step"] == 4
    again = HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, lr_schedule=LrSchedule("cosine", 5, 15, 0.1))
    again.load_optimizer_state_dict(sd)
    assert again.steps_done == 4 and again.current_lr() == sch.lr_at(1e-3, 5), "the schedule continues from the checkpoint's step"
    # another schedule, none at all, or a schedule over a checkpoint without one: refused, both named
    for other in (LrSchedule("cosine", 5, 16, 0.1), LrSchedule("linear", 5, 15, 0.1), LrSchedule("cosine", 5, 15, 0.2), None,
                  LrSchedule()):
        t2 = HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, lr_schedule=other)
        with pytest.raises(dry.HipError, match=r"schedule \(cosine\(warmup=5, total=15, min_ratio=0\.1\)\) differs") as e:
            t2.load_optimizer_state_dict(sd)
        assert ("none" if other is None or other.is_constant() else str(other)) in str(e.value)
        assert t2.steps_done == 0, "nothing was loaded"
    plain_sd = HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False).optimizer_state_dict()
    assert plain_sd["lr_schedule"] is None
    with pytest.raises(dry.HipError, match=r"schedule \(none\) differs"):
        again.load_optimizer_state_dict(plain_sd)
    HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, lr_schedule=LrSchedule()).load_optimizer_state_dict(plain_sd)
    # a payload without the key is an older checkpoint: it loads, the schedule continues from its step count
    old = {k: v for k, v in sd.items() if k != "lr_schedule"}
    t3 = HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, lr_schedule=sch)
    t3.load_optimizer_state_dict(old)
    assert t3.steps_done == 4 and t3.current_lr() == sch.lr_at(1e-3, 5)
    # torch.optim's grammar is as it was: the base rate in param_groups, no word of the schedule
    tsd = tr.torch_optimizer_state_dict()
    assert set(tsd) == {"state", "param_groups"} and all(g["lr"] == 1e-3 for g in tsd["param_groups"])
    assert "lr_schedule" not in tsd and all("lr_schedule" not in g for g in tsd["param_groups"])


# ---------------------------------------------------------------------------------------------------------------------
# 5. the command line
# ---------------------------------------------------------------------------------------------------------------------
def _train(*a):
    from inferbiomechanics_amd.cli.train import TrainCommand
    p = argparse.ArgumentParser()
    TrainCommand().register_subcommand(p.add_subparsers(dest="command"))
    return p.parse_args(["train"] + list(a))


def test_cli_flags_defaults_and_refusals():
    from inferbiomechanics_amd.cli.train import check_lr_schedule, resolve_lr_schedule
    from inferbiomechanics_amd.lr_schedule import LrSchedule
    a = _train()
    assert (a.lr_schedule, a.lr_warmup_steps, a.lr_total_steps, a.lr_min_ratio) == ("constant", 0, 0, 0.0)
    check_lr_schedule(a)
    assert resolve_lr_schedule(a, 100) is None, "the defaults are a run without a schedule"
    check_lr_schedule(_train("--eager"))
    a = _train("--lr-schedule", "cosine", "--lr-warmup-steps", "100", "--lr-total-steps", "5000", "--lr-min-ratio", "0.1")
    assert resolve_lr_schedule(a, 7) == LrSchedule("cosine", 100, 5000, 0.1)
    # --lr-total-steps 0: epochs x batches per epoch
    a = _train("--lr-schedule", "linear", "--lr-warmup-steps", "10", "--epochs", "3")
    assert resolve_lr_schedule(a, 40) == LrSchedule("linear", 10, 120, 0.0)
    # a warmup alone is a schedule; its total does not matter (a resumed run with more epochs is the same schedule)
    assert resolve_lr_schedule(_train("--lr-warmup-steps", "10", "--epochs", "3"), 40) == LrSchedule("constant", 10, 0, 0.0)
    with pytest.raises(SystemExit):
        _train("--lr-schedule", "exponential")
    for flags in (("--lr-schedule", "cosine", "--eager"), ("--lr-warmup-steps", "5", "--eager")):
        with pytest.raises(SystemExit, match="--eager runs torch.optim at one rate"):
            check_lr_schedule(_train(*flags))
    for m in ("-0.1", "1.5", "nan"):
        with pytest.raises(SystemExit, match=r"--lr-min-ratio must lie in \[0, 1\]"):
            check_lr_schedule(_train("--lr-schedule", "cosine", "--lr-total-steps", "10", "--lr-min-ratio", m))
    with pytest.raises(SystemExit, match="--lr-total-steps > --lr-warmup-steps, got 10 and 10"):
        check_lr_schedule(_train("--lr-schedule", "cosine", "--lr-total-steps", "10", "--lr-warmup-steps", "10"))
    with pytest.raises(SystemExit, match="--epochs x batches per epoch gives 8"):
        resolve_lr_schedule(_train("--lr-schedule", "linear", "--lr-warmup-steps", "8", "--epochs", "2"), 4)
    with pytest.raises(SystemExit, match="must be >= 0"):
        check_lr_schedule(_train("--lr-warmup-steps", "-3"))


BASE = ['--no-wandb', '--synthetic-windows', '24', '--batch-size', '8', '--data-loading-workers', '0', '--model-type',
        'diffusion-mlp', '--feat-dim', '24', '--hidden-dims', '32', '32', '--stride', '1', '--history-len', '6', '--seed', '7']


def test_train_with_a_schedule_in_dry_run(dry, tmp_path, capsys):
    """a scheduled run from start to resume: every optimizer launch is a `_sched` one with the flags' numbers, the rate is
    printed, the checkpoint carries the schedule, and a resumed run with other flags is refused with both named"""
    from inferbiomechanics_amd.main import main
    lib = dry.lib()
    d = str(tmp_path / "ck")
    flags = ['--lr-schedule', 'cosine', '--lr-warmup-steps', '2', '--lr-min-ratio', '0.1']
    with pytest.raises(SystemExit, match="--eager"):
        main(['train', '--epochs', '1', '--checkpoint-dir', d, '--eager'] + BASE + flags)
    assert not os.path.exists(d), "refused before anything was written"
    lib.calls.clear()
    del lib.args[:]
    assert main(['train', '--epochs', '2', '--checkpoint-dir', d] + BASE + flags)          # 3 batches per epoch: T = 6
    opt = [(n, a) for n, a in lib.args if n.startswith("ib_optim_step")]
    assert len(opt) >= 6 and all(n.endswith("_sched") and a[-5:-1] == (2, 2, 6, M01) for n, a in opt)
    out = capsys.readouterr().out
    assert "Learning-rate schedule: cosine(warmup=2, total=6, min_ratio=0.1)" in out
    # the default base rate is 1e-4: step 4 is half way down the cosine (0.55 of it), step 7 is past T (0.1 of it)
    assert re.search(r"epoch 0: learning rate 5\.5e-05 at step 4", out) and re.search(r"epoch 1: learning rate 1e-05 at step 7", out)
    ck = torch.load(os.path.join(d, "diffusion-mlp", "epoch_1_batch_2.pt"), map_location="cpu")
    assert ck["optimizer_state_dict"]["lr_schedule"] == {"kind": "cosine", "warmup": 2, "total": 6, "min_ratio": M01}
    # more epochs change the derived total: refused, both named, the way out named
    with pytest.raises(SystemExit, match=r"cosine\(warmup=2, total=6, min_ratio=0\.1\).*cosine\(warmup=2, total=9, min_ratio=0\.1\)"
                                         r".*--lr-total-steps explicitly"):
        main(['train', '--epochs', '3', '--checkpoint-dir', d] + BASE + flags)
    with pytest.raises(SystemExit, match=r"differs from this trainer's \(none\)"):
        main(['train', '--epochs', '3', '--checkpoint-dir', d] + BASE)
    lib.calls.clear()
    assert main(['train', '--epochs', '3', '--checkpoint-dir', d, '--lr-total-steps', '6'] + BASE + flags)
    assert "ib_optim_step_sched" in lib.calls or "ib_optim_step_sources_sched" in lib.calls
    # without the flags: the launches without a schedule, no rate printed, the key None
    capsys.readouterr()
    lib.calls.clear()
    assert main(['train', '--epochs', '1', '--checkpoint-dir', str(tmp_path / "plain")] + BASE)
    assert not any(n.endswith("_sched") for n in lib.calls) and "learning rate" not in capsys.readouterr().out.lower()
    ck = torch.load(os.path.join(str(tmp_path / "plain"), "diffusion-mlp", "epoch_0_batch_2.pt"), map_location="cpu")
    assert ck["optimizer_state_dict"]["lr_schedule"] is None
