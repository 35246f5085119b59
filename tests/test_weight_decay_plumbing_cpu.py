"""Host side of the decoupled weight decay without a GPU: decay_factor against hand-computed values, the trainer's range table
in dry-run mode (exactly the ndim >= 2 parameters, sorted, disjoint, 64-aligned starts, a decay_filter changes it), the table
and the origin every optimizer launch carries, weight_decay = 0 as the trainer without the argument, the state-dict round
trip, the command line, the eleventh header and the build lists, and the argument checks of the entries."""
import argparse
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

NAMES = ["ib_decay_table_build", "ib_decay_table_bytes", "ib_optim_step_decay", "ib_optim_step_sources_decay"]
WD = float(np.float32(0.1))


@pytest.fixture()
def dry():
    from inferbiomechanics_amd import hip
    hip.set_dry_run(True)
    yield hip
    hip.set_dry_run(False)


def f32(x):
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the factor
# ---------------------------------------------------------------------------------------------------------------------
def test_decay_factor_matches_hand_computed_values():
    from inferbiomechanics_amd.weight_decay import decay_factor
    # powers of two are exact in fp32: 1 - 2^-7 * 2^-3 = 1 - 2^-10 = 0.9990234375
    assert decay_factor(2.0 ** -7, 2.0 ** -3) == 0.9990234375
    assert decay_factor(0.5, 0.5) == 0.75 and decay_factor(1.0, 1.0) == 0.0 and decay_factor(1.0, 2.0) == -1.0
    # fp32(1e-2) = 0.00999999977648258209228515625, fp32(0.1) = 0.100000001490116119384765625 (both exact decimals); their
    # product is 0.000999999992549419413918258...; f64: 1 - that = 0.999000000007450580586...; the fp32 neighbours are
    # 0.99900001287460327 and 0.99899995326995850: the nearer is the upper one
    assert decay_factor(1e-2, 0.1) == 0.99900001287460327148 == f32(0.999)
    assert abs(decay_factor(1e-2, 0.1) - (1.0 - 0.00999999977648258209228515625 * 0.100000001490116119384765625)) <= 2.0 ** -25
    for lr in (1e-2, 1e-4, 3e-4, 1.0, 0.0):
        assert decay_factor(lr, 0.0) == 1.0, "exactly 1 without decay"
    assert decay_factor(0.0, 0.3) == 1.0
    # an fp32 value: rounding it again changes nothing
    for lr, wd in ((1e-3, 0.01), (3e-4, 0.05), (1e-4, 1e-2)):
        f = decay_factor(lr, wd)
        assert f == f32(f) and f == f32(1.0 - f32(lr) * f32(wd)) and 0.0 < f < 1.0
    assert decay_factor(1e-4, 1e-4) == 1.0, "a product below half an fp32 ulp of 1 decays nothing"


def test_weight_decay_refuses_bad_values():
    from inferbiomechanics_amd.engine import HipTrainer
    from inferbiomechanics_amd.weight_decay import check_weight_decay, default_decay_filter
    for bad in (-0.1, float("nan"), float("inf"), "much", None):
        with pytest.raises(ValueError, match="weight_decay"):
            check_weight_decay(bad)
    assert check_weight_decay(0) == 0.0 and check_weight_decay(0.1) == WD
    assert default_decay_filter("w", (3, 4)) and default_decay_filter("e", (2, 3, 4))
    assert not default_decay_filter("b", (7,)) and not default_decay_filter("s", ())
    with pytest.raises(ValueError, match="weight_decay"):
        HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, weight_decay=-1.0)
    with pytest.raises(ValueError, match="decay_filter"):
        HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, weight_decay=0.1, decay_filter="all")


# ---------------------------------------------------------------------------------------------------------------------
# 2. the header, the build lists, the argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_eleventh_header_has_its_own_table_and_is_built():
    from inferbiomechanics_amd import hip
    assert os.path.basename(hip.DECAY_HEADER_PATH) == "ib_hip_decay.h" and os.path.exists(hip.DECAY_HEADER_PATH)
    assert hip.decay_decls() == NAMES == sorted(hip._DECAY_SIGS)
    text = open(hip.DECAY_HEADER_PATH).read()
    for n in NAMES:
        assert len(re.findall(rf"\b(?:int|size_t) {n}\(", text)) == 1
        assert n not in hip._BOUND, "no name collides with another header's"
    assert len(hip._LOADED) == len(hip._BOUND) + 4
    assert hip._is_launch("ib_decay_table_build") and not hip._is_launch("ib_decay_table_bytes")
    decay = [hip._f32, hip._vp, hip._c.c_int, hip._i64]
    assert hip._sig("ib_optim_step_decay")[1] == hip._sig("ib_optim_step_sched")[1][:-1] + decay + [hip._vp]
    assert hip._sig("ib_optim_step_sources_decay")[1] == hip._sig("ib_optim_step_sources_sched")[1][:-1] + decay + [hip._vp]
    assert hip._sig("ib_decay_table_build") == (hip._c.c_int, [hip._vp, hip._vp, hip._c.c_int, hip._vp, hip._vp])
    assert hip._sig("ib_decay_table_bytes") == (hip._sz, [hip._c.c_int])
    mk = open(os.path.join(os.path.dirname(hip.__file__), "csrc", "Makefile")).read()
    hdrs = [w for line in re.findall(r"^HDRS\s*\+?=(.*)$", mk, flags=re.M) for w in line.split()]
    assert "../../include/ib_hip_decay.h" in hdrs and len([h for h in hdrs if h.startswith("../../include/")]) == 11
    for path in (hip.LIB_PATH, hip.AB_LIB_PATH):
        if not os.path.exists(path):
            pytest.fail(f"{path} is not built")
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        assert set(NAMES) <= {line.split()[-1] for line in out.splitlines() if line.strip()}, path
    root = os.path.dirname(os.path.dirname(hip.__file__))
    for doc in ("README.md", "INTEGRATION.md"):
        assert "ib_hip_decay.h" in open(os.path.join(root, doc)).read(), doc
    assert "decay_decls" in open(os.path.join(root, "__graft_entry__.py")).read(), "build() checks the eleventh header's exports"
    lib = hip.lib()
    assert (lib.ib_decay_table_bytes(0), lib.ib_decay_table_bytes(1), lib.ib_decay_table_bytes(300)) == (16, 16, 4800)
    assert lib.ib_decay_table_bytes(-1) == 0


def _i64(*v):
    return (ctypes.c_int64 * max(len(v), 1))(*v)


def test_argument_errors_come_before_any_launch():
    """IB_E_ARG = -1; the device pointers are never dereferenced on the host, any non-null value stands for one"""
    from inferbiomechanics_amd import hip
    lib = hip.lib()
    cv = lambda a: ctypes.cast(a, ctypes.c_void_p)
    dev = 1 << 20                                        # stands for a device pointer: a refused build never writes to it
    for start, ln in [((8, 0), (4, 4)), ((0, 4), (8, 4)), ((0, 4), (6, 4)), ((-4,), (4,)), ((2,), (4,)), ((0,), (0,)), ((0,), (-4,)),
                      ((0, 0), (4, 4)), ((0, 16, 8), (4, 4, 4))]:
        assert lib.ib_decay_table_build(cv(_i64(*start)), cv(_i64(*ln)), len(start), dev, None) == -1, (start, ln)
    assert lib.ib_decay_table_build(cv(_i64(0)), cv(_i64(4)), -1, dev, None) == -1
    assert lib.ib_decay_table_build(cv(_i64(0)), cv(_i64(4)), 1, None, None) == -1
    assert lib.ib_decay_table_build(None, cv(_i64(4)), 1, dev, None) == -1
    assert lib.ib_decay_table_build(cv(_i64(0)), None, 1, dev, None) == -1
    assert lib.ib_decay_table_build(cv(_i64(0)), cv(_i64(4)), 1, dev + 8, None) == -1, "a table that is not 16-byte aligned"
    assert lib.ib_decay_table_build(None, None, 0, dev, None) == 0, "an empty table: nothing to upload"
    nan = float("nan")
    ok_s = (2, 5, 15, 0.1)
    plain = lambda s, d: lib.ib_optim_step_decay(0, 4096, 8192, None, None, 64, 1e-2, 1.0, 1, None, None, None, None, 0.0, 0,
                                                 *s, *d, None)
    srcs = lambda s, d: lib.ib_optim_step_sources_decay(0, 4096, 8192, None, None, 64, 1e-2, 1.0, 1, None, None, None, 0, None,
                                                        None, None, None, None, None, None, None, 0, 0, 0.0, None, None, 0.0,
                                                        0, *s, *d, None)
    for d in [(-0.1, dev, 1, 0), (nan, dev, 1, 0), (0.1, dev, -1, 0), (0.1, None, 1, 0), (0.1, dev, 1, -4), (0.1, dev, 1, 2),
              (0.1, dev, 1, 6), (0.1, dev + 4, 1, 0)]:
        for s in (ok_s, (0, 0, 0, 0.0)):
            assert plain(s, d) == -1 and srcs(s, d) == -1, (s, d)
    good = (0.1, dev, 1, 0)
    for s in [(3, 0, 10, 0.0), (1, 5, 5, 0.0), (1, 0, 10, 1.5), (2, 0, 10, nan), (0, -2, 0, 0.0)]:
        assert plain(s, good) == -1 and srcs(s, good) == -1, s
    # good decay arguments do not excuse the optimizer's own checks, nor a bad EMA
    assert lib.ib_optim_step_decay(0, None, 8192, None, None, 64, 1e-2, 1.0, 1, None, None, None, None, 0.0, 0, *ok_s, *good, None) == -1
    assert lib.ib_optim_step_decay(0, 4096, 8192, None, None, 64, 1e-2, 1.0, 1, None, None, None, 12288, 1.5, 0, *ok_s, *good, None) == -1
    assert lib.ib_optim_step_decay(7, 4096, 8192, None, None, 64, 1e-2, 1.0, 1, None, None, None, None, 0.0, 0, *ok_s, *good, None) == -1


def test_decayed_kernels_do_not_spill_to_scratch_and_keep_the_occupancy():
    """the instantiations with a DecayArgs compile without VGPR spills or scratch, at the occupancy of the ones without
    (compile only, a few seconds).  The two clip forms (a ClipArgs behind the DecayArgs: a head with an LDS tree in front of
    the kernel) are test_grad_norm_plumbing_cpu.py's."""
    from tools import kernel_resources as kr
    if kr.hipcc() is None:
        pytest.skip("hipcc not installed")
    rows = [k for k in kr.resources("optim.hip") if k["kernel"].startswith("optim_kernel<") and "ClipArgs" not in k["mangled"]]
    decay = [k for k in rows if "DecayArgs" in k["mangled"]]
    plain = {k["kernel"]: k for k in rows if "DecayArgs" not in k["mangled"] and "SchedArgs" not in k["mangled"]}
    assert len(decay) == 8 and len(rows) == 16 and len(plain) == 4
    for k in decay:
        assert not k["vgpr_spill"] and not k["scratch"], k
        assert k["occupancy"] == plain[k["kernel"]]["occupancy"], (k, plain[k["kernel"]])


# ---------------------------------------------------------------------------------------------------------------------
# 3. the binding
# ---------------------------------------------------------------------------------------------------------------------
def _buffers(n=64):
    return [torch.zeros(n) for _ in range(4)]


def _sources(g):
    ws = torch.zeros(2, 16)
    return ([(ws, 2, g[16:32])], None, 0, [], [g[32:48]])


def test_binding_builds_the_table_and_chooses_the_entries(dry):
    from inferbiomechanics_amd.lr_schedule import KINDS as CODES, LrSchedule
    lib = dry.lib()
    del lib.args[:]
    tab = dry.DecayTable([(0, 16), (32, 6)], "cpu")
    name, a = lib.args[-1]
    assert name == "ib_decay_table_build" and a[2] == 2 and a[3] == tab.buf.data_ptr() and a[4] == 0
    rd = lambda p: ctypes.cast(p, ctypes.POINTER(ctypes.c_int64))
    assert [rd(a[0])[j] for j in range(2)] == [0, 32] and [rd(a[1])[j] for j in range(2)] == [16, 6]
    assert tab.n == 2 and tab.buf.dtype == torch.int64 and tab.buf.numel() * 8 == 32
    empty = dry.DecayTable([], "cpu")
    assert empty.n == 0 and empty.buf.numel() * 8 == 16 and lib.args[-1][1][2] == 0
    p, g, s1, s2 = _buffers()
    ema = torch.zeros(64)
    sch = LrSchedule("cosine", 5, 15, 0.1)
    four = (CODES["cosine"], 5, 15, f32(0.1))
    # weight_decay = 0: the entries of before, whatever else is given
    for kw in ({}, {"weight_decay": 0.0}, {"weight_decay": 0.0, "decay_table": tab, "decay_origin": 64}):
        lib.calls.clear()
        dry.optim_step("adam", p, g, s1, s2, 1e-3, step=3, **kw)
        dry.optim_step("adam", p, g, s1, s2, 1e-3, step=3, sources=_sources(g), **kw)
        dry.optim_step("adam", p, g, s1, s2, 1e-3, step=3, ema=ema, ema_decay=0.9, **kw)
        dry.optim_step("adam", p, g, s1, s2, 1e-3, step=3, sources=_sources(g), ema=ema, ema_decay=0.9, **kw)
        dry.optim_step("adam", p, g, s1, s2, 1e-3, step=3, lr_schedule=sch, **kw)
        assert lib.calls == ["ib_optim_step", "ib_optim_step_sources", "ib_optim_step_ema", "ib_optim_step_sources_ema",
                             "ib_optim_step_sched"], kw
    lib.calls.clear()
    lib.ema_ranges.clear()
    kw = {"weight_decay": 0.1, "decay_table": tab, "decay_origin": 128}
    tail = (0.1, tab.buf.data_ptr(), 2, 128, 0)
    dry.optim_step("adam", p, g, s1, s2, 1e-3, step=3, **kw)
    name, a = lib.args[-1]
    assert name == "ib_optim_step_decay" and len(a) == 24 and a[6] == 1e-3 and a[12] is None
    assert a[15:19] == (0, 0, 0, 0.0), "no schedule: constant without warmup, the host's rate"
    assert a[19:] == tail
    dry.optim_step("adam", p, g, s1, s2, 1e-3, step=3, ema=ema, ema_decay=0.9, ema_warmup=False, lr_schedule=sch, **kw)
    name, a = lib.args[-1]
    assert name == "ib_optim_step_decay" and a[12:15] == (ema.data_ptr(), 0.9, 0) and a[15:19] == four and a[19:] == tail
    dry.optim_step("adam", p, g, s1, s2, 1e-3, step=3, lr_schedule=LrSchedule("constant", 0, 99, 0.5), **kw)
    assert lib.args[-1][1][15:19] == (0, 0, 0, 0.0), "a constant schedule without warmup is none"
    dry.optim_step("adam", p, g, s1, s2, 1e-3, step=3, sources=_sources(g), **kw)
    name, a = lib.args[-1]
    assert name == "ib_optim_step_sources_decay" and len(a) == 37 and a[12] == 2 and a[25] is None and a[32:] == tail
    dry.optim_step("adam", p, g, s1, s2, 1e-3, step=3, sources=_sources(g), ema=ema, ema_decay=0.5, lr_schedule=sch, **kw)
    name, a = lib.args[-1]
    assert name == "ib_optim_step_sources_decay" and a[25:28] == (ema.data_ptr(), 0.5, 1) and a[28:32] == four and a[32:] == tail
    assert lib.calls == ["ib_optim_step_decay"] * 3 + ["ib_optim_step_sources_decay"] * 2
    assert lib.ema_ranges == [(ema.data_ptr(), 64, []), (ema.data_ptr(), 64, [(32, 16)])], "the EMA bookkeeping of the dry run"
    n = len(lib.calls)
    for bad in ({"weight_decay": 0.1}, {"weight_decay": 0.1, "decay_table": tab.buf}, {"weight_decay": -0.1, "decay_table": tab},
                {"weight_decay": float("nan"), "decay_table": tab}, {"weight_decay": 0.1, "decay_table": tab, "decay_origin": 2},
                {"weight_decay": 0.1, "decay_table": tab, "decay_origin": -4}):
        with pytest.raises(dry.HipError):
            dry.optim_step("adam", p, g, s1, s2, 1e-3, step=3, **bad)
    assert len(lib.calls) == n, "a refused call launches nothing"


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


def _covered(ranges):
    """the set of 64-element blocks the ranges cover + the checks every table must pass"""
    blocks, prev = set(), 0
    for a, ln in ranges:
        assert a % 64 == 0 and ln > 0 and ln % 64 == 0 and a >= prev, ranges
        assert a > prev or prev == 0, "touching ranges are merged"
        blocks.update(range(a // 64, (a + ln) // 64))
        prev = a + ln
    return blocks


def _blocks_of(layout, names):
    out = set()
    for k in names:
        off, n = layout[k]
        out.update(range(off // 64, -(-(off + n) // 64)))
    return out


@pytest.mark.parametrize("model", sorted(MODELS))
def test_trainer_table_covers_exactly_the_matrices(dry, model):
    from inferbiomechanics_amd.engine import HipTrainer
    mk, _ = MODELS[model]
    tr = HipTrainer(mk(), "diffusion", "adam", 1e-3, use_graph=False, weight_decay=0.1)
    shapes = {k: tuple(v.shape) for k, v in tr.model.named_parameters()}
    want = [k for k in tr.layout if len(shapes[k]) >= 2]
    assert tr.decayed == want and 0 < len(want) < len(shapes), "some are decayed, some are not"
    assert tr.decay_table.ranges == tr.decay_ranges and tr.decay_table.n == len(tr.decay_ranges) <= 64
    assert _covered(tr.decay_ranges) == _blocks_of(tr.layout, want)
    assert not _covered(tr.decay_ranges) & _blocks_of(tr.layout, [k for k in tr.layout if k not in want])
    assert tr.weight_decay == WD
    # a filter changes the covered set: biases only, everything, nothing
    only_b = HipTrainer(mk(), "diffusion", "adam", 1e-3, use_graph=False, weight_decay=0.1,
                        decay_filter=lambda name, shape: len(shape) < 2)
    rest = [k for k in tr.layout if k not in want]
    assert only_b.decayed == rest and _covered(only_b.decay_ranges) == _blocks_of(tr.layout, rest)
    every = HipTrainer(mk(), "diffusion", "adam", 1e-3, use_graph=False, weight_decay=0.1, decay_filter=lambda name, shape: True)
    assert every.decay_ranges == [(0, tr.flat.numel())], "all neighbours merged into one range"
    none = HipTrainer(mk(), "diffusion", "adam", 1e-3, use_graph=False, weight_decay=0.1, decay_filter=lambda name, shape: False)
    assert none.decay_ranges == [] and none.decay_table.n == 0
    seen = []
    HipTrainer(mk(), "diffusion", "adam", 1e-3, use_graph=False, weight_decay=0.1,
               decay_filter=lambda name, shape: seen.append((name, shape)) or False)
    assert seen == [(k, shapes[k]) for k in tr.layout], "the filter sees every name with its shape"


def _step_calls(hip, tr, batch):
    lib = hip.lib()
    lib.calls.clear()
    del lib.args[:]
    tr.step(batch)
    return list(lib.calls), [(n, a) for n, a in lib.args if n.startswith("ib_optim_step")]


@pytest.mark.parametrize("model", sorted(MODELS))
def test_every_optimizer_launch_carries_the_table_and_its_origin(dry, model):
    from inferbiomechanics_amd.engine import HipTrainer
    from inferbiomechanics_amd.lr_schedule import LrSchedule
    mk, mb = MODELS[model]
    batch = mb()
    plain = HipTrainer(mk(), "diffusion", "adam", 1e-3, use_graph=False)
    names_plain, opt_plain = _step_calls(dry, plain, batch)
    assert plain.decay_table is None and plain._decay_args(0) == {}
    for kw in (dict(), dict(ema_decay=0.999), dict(lr_schedule=LrSchedule("cosine", 5, 15, 0.1), ema_decay=0.999)):
        tr = HipTrainer(mk(), "diffusion", "adam", 1e-3, use_graph=False, weight_decay=0.1, **kw)
        p0 = tr.flat.data_ptr()
        for _ in range(2):
            names, opt = _step_calls(dry, tr, batch)
            assert [re.sub(r"_(decay|ema|sched)$", "", n) for n in names] == [re.sub(r"_(ema)$", "", n) for n in names_plain]
            assert len(opt) == len(opt_plain) >= (1 if model == "mlp" else 2) and all(n.endswith("_decay") for n, _ in opt)
            for (n, a), (_, b) in zip(opt, opt_plain):
                assert a[-5:-1] == (WD, tr.decay_table.buf.data_ptr(), tr.decay_table.n, (a[1] - p0) // 4), (n, a[-5:])
                assert (a[1] - p0) % 16 == 0 and a[5] == b[5] and (a[1] - p0) == (b[1] - plain.flat.data_ptr()), "the same slices"
                assert a[-9:-5] == ((2, 5, 15, f32(0.1)) if "lr_schedule" in kw else (0, 0, 0, 0.0))
    if model == "transformer":
        assert len({a[1] for _, a in opt}) > 1, "launches over several slices, each with its own origin"


def test_weight_decay_zero_is_the_trainer_without_the_argument(dry):
    from inferbiomechanics_amd.engine import HipTrainer
    for model in sorted(MODELS):
        mk, mb = MODELS[model]
        batch = mb()

        def norm(tr):
            names, opt = _step_calls(dry, tr, batch)
            p0 = tr.flat.data_ptr()
            return names, [(n, (a[1] - p0), a[5:9], len(a)) for n, a in opt]
        want = norm(HipTrainer(mk(), "diffusion", "adam", 1e-3, use_graph=False))
        for kw in (dict(weight_decay=0.0), dict(weight_decay=0), dict(weight_decay=0.0, decay_filter=lambda n, s: True)):
            tr = HipTrainer(mk(), "diffusion", "adam", 1e-3, use_graph=False, **kw)
            assert norm(tr) == want and tr.decay_table is None and "ib_decay_table_build" not in dry.lib().calls, (model, kw)


def test_the_launch_that_only_counts_the_step_decays_nothing(dry):
    """everything updated by earlier launches: the last launch is one block over the buffer's last 64 elements, all of them
    named as done (kind 3), which the kernel skips before the decay"""
    from inferbiomechanics_amd.engine import HipTrainer
    tr = HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, weight_decay=0.1, decay_filter=lambda n, s: True)
    n = tr.flat.numel()
    tr._early_done = [(0, n)]
    lib = dry.lib()
    del lib.args[:]
    tr._finish_step(None)
    name, a = lib.args[-1]
    assert name == "ib_optim_step_sources_decay" and a[5] == 64 and a[-2] == n - 64 and a[12] == 1
    rd = lambda p, ct: ctypes.cast(p, ctypes.POINTER(ct))
    assert (rd(a[13], ctypes.c_int64)[0], rd(a[14], ctypes.c_int64)[0], rd(a[15], ctypes.c_int32)[0]) == (0, 64, 3)


def test_trainer_state_dict_round_trip_of_the_decay(dry):
    from inferbiomechanics_amd.engine import HipTrainer
    tr = HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, weight_decay=0.1)
    for _ in range(3):
        tr.step(_batch())
    sd = tr.optimizer_state_dict()
    assert sd["weight_decay"] == WD and sd["decayed"] == tr.decayed and sd["step"] == 3
    again = HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, weight_decay=0.1)
    again.load_optimizer_state_dict(sd)
    assert again.steps_done == 3
    for other in (dict(), dict(weight_decay=0.0), dict(weight_decay=0.2)):
        t2 = HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, **other)
        with pytest.raises(dry.HipError, match=r"the checkpoint's weight decay \(0\.1\) differs from this trainer's \((0|0\.2)\)"):
            t2.load_optimizer_state_dict(sd)
        assert t2.steps_done == 0, "nothing was loaded"
    t3 = HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, weight_decay=0.1, decay_filter=lambda n, s: True)
    with pytest.raises(dry.HipError, match=r"weight decay \(0\.1 over other parameters\) differs"):
        t3.load_optimizer_state_dict(sd)
    plain = HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False)
    plain_sd = plain.optimizer_state_dict()
    assert plain_sd["weight_decay"] == 0.0 and plain_sd["decayed"] == []
    with pytest.raises(dry.HipError, match=r"weight decay \(0\) differs from this trainer's \(0\.1\)"):
        again.load_optimizer_state_dict(plain_sd)
    # a payload without the key is an older checkpoint: it loads into a trainer without decay and counts as weight_decay 0
    old = {k: v for k, v in plain_sd.items() if k not in ("weight_decay", "decayed")}
    HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False).load_optimizer_state_dict(old)
    HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, weight_decay=0.0,
               decay_filter=lambda n, s: True).load_optimizer_state_dict(old)
    with pytest.raises(dry.HipError, match=r"weight decay \(0\) differs"):
        again.load_optimizer_state_dict(old)
    # torch.optim's grammar is as it was: no word of the decay
    tsd = tr.torch_optimizer_state_dict()
    assert set(tsd) == {"state", "param_groups"}
    assert tsd["param_groups"] == plain.torch_optimizer_state_dict()["param_groups"], "no weight_decay of this trainer's in there"
    assert "decay" in HipTrainer.torch_optimizer_state_dict.__doc__


# ---------------------------------------------------------------------------------------------------------------------
# 5. the command line
# ---------------------------------------------------------------------------------------------------------------------
def _train(*a):
    from inferbiomechanics_amd.cli.train import TrainCommand
    p = argparse.ArgumentParser()
    TrainCommand().register_subcommand(p.add_subparsers(dest="command"))
    return p.parse_args(["train"] + list(a))


def test_cli_flag_default_and_refusals():
    from inferbiomechanics_amd.cli.train import check_weight_decay_args
    assert _train().weight_decay == 0.0
    check_weight_decay_args(_train())
    check_weight_decay_args(_train("--eager"))
    check_weight_decay_args(_train("--weight-decay", "0", "--eager"))
    for opt in ("sgd", "adam", "rmsprop", "adagrad", "adadelta", "adamax"):
        check_weight_decay_args(_train("--weight-decay", "0.01", "--opt-type", opt))
    with pytest.raises(SystemExit, match="--weight-decay needs the fused trainer: --eager"):
        check_weight_decay_args(_train("--weight-decay", "0.01", "--eager"))
    for bad in ("-0.1", "nan", "inf"):
        with pytest.raises(SystemExit, match="--weight-decay must be finite and >= 0"):
            check_weight_decay_args(_train("--weight-decay", bad))


BASE = ['--no-wandb', '--synthetic-windows', '24', '--batch-size', '8', '--data-loading-workers', '0', '--model-type',
        'diffusion-mlp', '--feat-dim', '24', '--hidden-dims', '32', '32', '--stride', '1', '--history-len', '6', '--seed', '7']


def test_train_with_weight_decay_in_dry_run(dry, tmp_path, capsys):
    """a decayed run from start to resume: refused with --eager before anything is written, every optimizer launch a `_decay`
    one with the flag's value, the checkpoint carries it, a resumed run with another value is refused"""
    from inferbiomechanics_amd.main import main
    lib = dry.lib()
    d = str(tmp_path / "ck")
    with pytest.raises(SystemExit, match="--weight-decay needs the fused trainer"):
        main(['train', '--epochs', '1', '--checkpoint-dir', d, '--eager', '--weight-decay', '0.1'] + BASE)
    assert not os.path.exists(d), "refused before anything was written"
    lib.calls.clear()
    del lib.args[:]
    assert main(['train', '--epochs', '1', '--checkpoint-dir', d, '--weight-decay', '0.1', '--opt-type', 'adam'] + BASE)
    opt = [(n, a) for n, a in lib.args if n.startswith("ib_optim_step")]
    assert len(opt) >= 3 and all(n.endswith("_decay") and a[-5] == WD and a[-3] >= 1 for n, a in opt)
    assert lib.calls.count("ib_decay_table_build") == 1, "the table is built once"
    assert "Weight decay 0.1 (decoupled)" in capsys.readouterr().out
    ck = torch.load(os.path.join(d, "diffusion-mlp", "epoch_0_batch_2.pt"), map_location="cpu")
    assert ck["optimizer_state_dict"]["weight_decay"] == WD and len(ck["optimizer_state_dict"]["decayed"]) >= 1
    with pytest.raises(SystemExit, match=r"weight decay \(0\.1\) differs from this trainer's \(0\.2\).*same --weight-decay"):
        main(['train', '--epochs', '2', '--checkpoint-dir', d, '--weight-decay', '0.2', '--opt-type', 'adam'] + BASE)
    with pytest.raises(SystemExit, match=r"weight decay \(0\.1\) differs from this trainer's \(0\)"):
        main(['train', '--epochs', '2', '--checkpoint-dir', d, '--opt-type', 'adam'] + BASE)
    lib.calls.clear()
    assert main(['train', '--epochs', '2', '--checkpoint-dir', d, '--weight-decay', '0.1', '--opt-type', 'adam'] + BASE)
    assert "ib_optim_step_decay" in lib.calls or "ib_optim_step_sources_decay" in lib.calls
    lib.calls.clear()
    assert main(['train', '--epochs', '1', '--checkpoint-dir', str(tmp_path / "plain")] + BASE)
    assert not any(n.endswith("_decay") or n == "ib_decay_table_build" for n in lib.calls)
