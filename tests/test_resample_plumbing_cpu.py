"""Host side of RePaint resampling without a GPU: the walk and the jump table (diffusion/schedule.py), the sixth header and
the Makefile lists, the launch sequence of a resampled loop in dry-run traces (tools/sampler_trace.py's instruments), the
samplers', the predictor's and the command line's refusals -- and the statistics that are the reason for the feature: on the
2-D Gaussian inpainting problem of docs/EXPERIMENTS.md (tests/resample_restatement.py, float64 on the project's own tables) the
plain masked loop converges to the wrong conditional and the resampled one removes most of the error."""
import argparse
import os
import re

import pytest
import torch

from tests import resample_restatement as RR
from tools import sampler_trace
from tools.plan_trace import _Trace

BF = torch.bfloat16
NAME = "ib_resample_renoise"
T, D = sampler_trace.SMALL["T"], sampler_trace.SMALL["D"]
S = sampler_trace.S


@pytest.fixture()
def dry():
    from inferbiomechanics_amd import hip
    hip.set_dry_run(True)
    yield hip
    hip.set_dry_run(False)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the walk and the table
# ---------------------------------------------------------------------------------------------------------------------
def test_walk_of_five_steps():
    from inferbiomechanics_amd.diffusion.schedule import resample_walk
    assert resample_walk(5, 2, 2) == [("step", 0), ("step", 1), ("step", 2), ("jump", 3, 0), ("step", 1), ("step", 2), ("step", 3),
                                      ("step", 4), ("jump", 5, 1), ("step", 3), ("step", 4)]


@pytest.mark.parametrize("S_,jump,times,evals", [(20, 2, 10, 182), (20, 5, 2, 35), (100, 10, 10, 910), (5, 2, 2, 9), (7, 3, 4, 25),
                                                 (6, 5, 3, 16)])
def test_walk_counts_and_positions(S_, jump, times, evals):
    from inferbiomechanics_amd.diffusion.schedule import resample_evaluations, resample_walk
    walk = resample_walk(S_, jump, times)
    assert sum(op[0] == "step" for op in walk) == evals == S_ + (-(-S_ // jump) - 1) * (times - 1) * jump
    assert resample_evaluations(S_, jump, times) == evals
    assert walk[-1] == ("step", S_ - 1) and walk[0] == ("step", 0) and walk[1] == ("step", 1)
    # the walk is consistent: a step starts where the state is, a jump leaves from where it is and lands on a position >= 1
    p, visits, left = 0, [], {}
    for op in walk:
        assert op[1] == p, (op, p)
        if op[0] == "step":
            p += 1
        else:
            assert p - jump >= 1 and (S_ - p) % jump == 0
            visits.append(op[2])
            left[p] = left.get(p, 0) + 1
            p -= jump
    assert p == S_ and visits == list(range(len(visits)))
    points = [S_ - m * jump for m in range(S_) if S_ - m * jump - jump > 0]
    assert left == {q: times - 1 for q in points}, "every jump point is left backwards times - 1 times in total"


def test_walk_plain_and_refusals():
    from inferbiomechanics_amd.diffusion.schedule import check_resample, resample_walk
    for jump in (1, 2, 4):
        assert resample_walk(5, jump, 1) == [("step", p) for p in range(5)]
    assert check_resample(None, 5) is None and check_resample((2, 1), 5) is None and check_resample((2, 3), 5) == (2, 3)
    for bad in ((0, 2), (5, 2), (-1, 2), (6, 2)):
        with pytest.raises(ValueError, match="jump"):
            resample_walk(5, *bad)
    for bad in ((2, 0), (2, -3)):
        with pytest.raises(ValueError, match="times"):
            resample_walk(5, *bad)
    with pytest.raises(ValueError, match="jump"):
        resample_walk(5, 7, 1)                                         # times = 1 does not excuse a bad jump
    for bad in (3, (2,), (2, 2.5), "ab", (1, 2, 3)):
        with pytest.raises(ValueError, match="resample"):
            check_resample(bad, 5)


@pytest.mark.parametrize("spacing", ["time", "logsnr"])
@pytest.mark.parametrize("jump", [1, 2, 7])
def test_table_rows(spacing, jump):
    from inferbiomechanics_amd.diffusion import schedule as sch
    S_ = 20
    c = sch.resample_coefficients(1000, S_, jump, spacing)
    assert tuple(c.shape) == (S_ + 1, 2) and c.dtype == torch.float64
    assert not c[:jump].any(), "rows p < jump are (0, 0)"
    assert float(((c[jump:] ** 2).sum(1) - 1).abs().max()) <= 1e-15
    ab = sch.alphas_cumprod(1000)
    ts = sch.sample_timesteps(1000, S_, spacing).tolist()
    L = [float(ab[t]) for t in ts] + [1.0]
    for p in range(jump, S_ + 1):
        assert abs(float(c[p, 0]) ** 2 - L[p - jump] / L[p]) <= 1e-15, p
    # the level of position p is the one the observation table pins at row p
    oc = sch.observation_coefficients(1000, S_, spacing)
    assert torch.allclose(oc[:, 0] ** 2, torch.tensor(L, dtype=torch.float64), rtol=0, atol=1e-15)
    for bad in (0, S_, -1):
        with pytest.raises(ValueError):
            sch.resample_coefficients(1000, S_, bad, spacing)


def test_tables_object_keeps_the_step_tables():
    from inferbiomechanics_amd.diffusion import schedule as sch
    t = sch.DiffusionTables(torch.device("cpu"), num_sample_steps=10)
    assert t.resample_coef is None and t.resample_jump == 0
    assert t.serves(10) and not t.serves(10, resample_jump=3)
    before = (t.ddim_coef.data_ptr(), t.obs_coef.data_ptr(), t.ddim_t.data_ptr())
    t.set_resample(3)
    assert (t.ddim_coef.data_ptr(), t.obs_coef.data_ptr(), t.ddim_t.data_ptr()) == before, "the captured step's tables stay"
    assert t.serves(10, resample_jump=3) and t.serves(10) and not t.serves(10, resample_jump=2)
    assert t.resample_coef.dtype == torch.float32 and tuple(t.resample_coef.shape) == (11, 2)
    assert torch.equal(t.resample_coef, sch.resample_coefficients(1000, 10, 3).to(torch.float32))
    with pytest.raises(ValueError):
        t.set_resample(10)
    assert t.serves(10, resample_jump=3), "a refused jump leaves the table as it was"
    t.set_sampler(20)
    assert t.resample_coef is None and not t.serves(20, resample_jump=3), "a new grid drops the jump table"
    t.set_resample(3)
    t.set_resample(0)
    assert t.resample_coef is None


# ---------------------------------------------------------------------------------------------------------------------
# 2. the header and the build lists
# ---------------------------------------------------------------------------------------------------------------------
def test_sixth_header_is_parsed_into_its_own_table_and_built():
    from inferbiomechanics_amd import hip
    assert os.path.basename(hip.RESAMPLE_HEADER_PATH) == "ib_hip_resample.h" and os.path.exists(hip.RESAMPLE_HEADER_PATH)
    assert hip.resample_symbols() == [NAME] == sorted(hip._RESAMPLE_SIGS) and hip._RESAMPLE_SIGS in hip._TABLES
    assert len(hip._TABLES) == 6
    include = os.path.dirname(hip.RESAMPLE_HEADER_PATH)
    count = sum(len(re.findall(rf"\bint {NAME}\(", open(os.path.join(include, f)).read())) for f in os.listdir(include))
    assert count == 1, "the symbol is declared once across all headers"
    assert all(NAME not in t for t in (hip._SIGS, hip._STITCH_SIGS, hip._HEAD_SIGS, hip._SDE_SIGS, hip._CFG_SIGS))
    res, args = hip._sig(NAME)
    vp, i64, i32, u32, u64, ci = hip._vp, hip._i64, hip._i32, hip._c.c_uint32, hip._c.c_uint64, hip._c.c_int
    assert res is ci and hip._is_launch(NAME)
    assert args == [vp] * 7 + [i64, i32, vp, i32, u32, vp, vp, vp, vp, u64] + [i64] * 6 + [ci, vp]
    mk = open(os.path.join(os.path.dirname(hip.__file__), "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, flags=re.M).group(1).split()
    hdrs = re.search(r"^HDRS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "resample.hip" in srcs and "../../include/ib_hip_resample.h" in hdrs
    text = open(os.path.join(os.path.dirname(hip.__file__), "csrc", "philox.h")).read()
    assert re.search(r"\b4 = the re-noise", text) and RR.DOMAIN_JUMP == 4
    src = open(os.path.join(os.path.dirname(hip.__file__), "csrc", "resample.hip")).read()
    assert re.search(r"kDomainJump\s*=\s*4u", src)


def test_library_exports_and_refuses_before_launching():
    import subprocess
    from inferbiomechanics_amd import hip
    for path in (hip.LIB_PATH, hip.AB_LIB_PATH):
        if not os.path.exists(path):
            pytest.fail(f"{path} is not built")
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        assert NAME in {line.split()[-1] for line in out.splitlines() if line.strip()}, path
    # a null state is IB_E_ARG = -1 before anything is launched
    assert hip.lib().ib_resample_renoise(None, None, None, None, None, None, None, 10, 0, None, 1, 0, None, None, None, None, 0,
                                         1, 1, 8, 8, 8, 8, 0, None) == -1


def test_binding_checks(dry):
    hip, lib = dry, dry.lib()
    from inferbiomechanics_amd.diffusion.schedule import stitch_layout
    N, W, Tw, ld, S_ = 2, 1, 8, 16, 10
    x, x0, z = (torch.zeros(N, W, Tw, ld) for _ in range(3))
    mask = torch.zeros(Tw, ld, dtype=torch.uint8)
    coef, oc = torch.zeros(S_ + 1, 2), torch.zeros(S_ + 1, 2)
    ts, t_out = torch.zeros(S_, dtype=torch.int64), torch.zeros(N * W, dtype=torch.int64)
    start, cover, _, _ = stitch_layout(Tw, Tw, Tw)
    ids, ctr = torch.tensor([5, 2 ** 32 - 1]), torch.zeros(1, dtype=torch.int32)
    go = lambda **kw: hip.resample_renoise(kw.get("x", x), kw.get("x0", x0), kw.get("z", z), kw.get("mask", mask),
                                           kw.get("coef", coef), kw.get("oc", oc), ts, start, cover, kw.get("ids", ids),
                                           (7 << 32) + 1, kw.get("back", 3), kw.get("visit", 4), kw.get("t_out", t_out),
                                           step_dev=ctr, D=12)
    go()
    name, a = lib.args[-1]
    assert name == NAME
    assert a == (x.data_ptr(), x0.data_ptr(), z.data_ptr(), mask.data_ptr(), coef.data_ptr(), oc.data_ptr(), ts.data_ptr(), S_, 0,
                 ctr.data_ptr(), 3, 4, t_out.data_ptr(), start.data_ptr(), cover.data_ptr(), ids.data_ptr(), (7 << 32) + 1,
                 N, W, Tw, Tw, 12, ld, hip.F32, 0)
    hip.resample_renoise(x, None, None, None, coef, None, ts, start, cover, ids, 1, 1, 2 ** 32 - 1, t_out)   # everything free
    assert lib.args[-1][1][1:4] == (None, None, None) and lib.args[-1][1][11] == 2 ** 32 - 1
    for bad in (dict(back=0), dict(back=S_ + 1), dict(visit=-1), dict(visit=1 << 32), dict(coef=torch.zeros(S_, 2)),
                dict(coef=torch.zeros(S_ + 1, 3)), dict(oc=torch.zeros(S_, 2)), dict(t_out=torch.zeros(N * W + 1, dtype=torch.int64)),
                dict(ids=ids[:1]), dict(ids=ids.to(torch.int32)), dict(x0=None), dict(mask=mask[:, :8]), dict(z=z[:, :, :, :8]),
                dict(x=x[..., :12]), dict(x=torch.zeros(N, Tw, ld))):
        with pytest.raises(hip.HipError):
            go(**bad)
    assert len(lib.calls) == 2


# ---------------------------------------------------------------------------------------------------------------------
# 3. the samplers' launch sequence
# ---------------------------------------------------------------------------------------------------------------------
def _mask():
    mask = torch.zeros(T, D, dtype=torch.bool)
    mask[:, :20] = True
    return mask


def _names(canon):
    return [e if isinstance(e, str) else e[0] for e in canon]


@pytest.mark.parametrize("dtype", [BF, torch.float32])
def test_resampled_launch_sequence_is_the_walk(dtype):
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler
    from inferbiomechanics_amd.diffusion.schedule import resample_walk
    B = 3

    def trace(**kw):
        with _Trace() as tr, sampler_trace.Run(tr) as r:
            smp = ConditionalDDIMSampler(r.model(dtype, **sampler_trace.SMALL), S, use_graph=False, seed=5, **kw)
            smp.sample(r.randn(B, T, D), r.randn(B, T, D), _mask(), window_ids=[9, 4, 11])
            return tr.canonical(), list(tr.log), smp

    plain, _, sp = trace()
    for off in (dict(resample=None), dict(resample=(2, 1))):
        canon, _, s0 = trace(**off)
        assert canon == plain, "resampling off is today's sampler: launches, arguments, signature, buffers"
        assert "win" not in s0._bufs and "one_window" not in s0._bufs
    canon, log, smp = trace(resample=(2, 2))
    names = _names(canon)
    ops = [n for n in names if n in ("ib_ddim_cond_step", NAME, "ib_counter_add")]
    want = []
    for op in resample_walk(S, 2, 2):
        want += ["ib_ddim_cond_step", "ib_counter_add"] if op[0] == "step" else [NAME, "ib_counter_add"]
    assert ops == want, "the launch sequence is the walk"
    assert names.count("ib_ddim_cond_step") == 9 and names.count(NAME) == 2
    adds = [a[1] for n, a in log if n == "ib_counter_add"]
    assert adds == [1, 1, 1, -2, 1, 1, 1, 1, -2, 1, 1]
    b = smp._bufs
    # the step is today's: the same launches per step, and the same signature (the jump is no part of the captured step)
    pnames = _names(plain)
    cut = lambda ns: [i for i, n in enumerate(ns) if n == "ib_counter_add"]
    assert names[:cut(names)[2] + 1] == pnames[:cut(pnames)[2] + 1], "up to the first jump the trace is the plain loop's"
    assert len(smp._sig) == len(sp._sig) and tuple(b["win"].shape) == (B,) and b["win"].tolist() == [9, 4, 11]
    start, cover, _ = b["one_window"]
    assert start.tolist() == [0] and cover.tolist() == [[0, 1]] * T
    tabs = smp.model.tables(b["x"].device)
    Dp = b["x"].shape[-1]
    from inferbiomechanics_amd import hip
    code = hip.BF16 if dtype == BF else hip.F32
    jumps = [a for n, a in log if n == NAME]
    for visit, a in enumerate(jumps):
        assert a == (b["x"].data_ptr(), b["x0"].data_ptr(), b["z"].data_ptr(), b["mask"].data_ptr(), tabs.resample_coef.data_ptr(),
                     tabs.obs_coef.data_ptr(), tabs.ddim_t.data_ptr(), S, 0, b["ctr"].data_ptr(), 2, visit, b["t"].data_ptr(),
                     start.data_ptr(), cover.data_ptr(), b["win"].data_ptr(), 5, B, 1, T, T, D, Dp, code, 0)
    assert tabs.resample_jump == 2


def test_steps_truncates_after_that_many_evaluations(dry):
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler
    r = sampler_trace.Run()
    lib = dry.lib()
    smp = ConditionalDDIMSampler(r.model(BF, **sampler_trace.SMALL), S, use_graph=False, resample=(2, 2))
    for steps, evals, jumps in ((1, 1, 0), (3, 3, 0), (4, 4, 1), (7, 7, 1), (8, 8, 2), (9, 9, 2), (50, 9, 2), (None, 9, 2)):
        lib.calls.clear()
        smp.sample(r.randn(2, T, D), r.randn(2, T, D), _mask(), steps=steps)
        assert (lib.calls.count("ib_ddim_cond_step"), lib.calls.count(NAME)) == (evals, jumps), steps


def test_settings_change_between_calls(dry):
    """on, other values, off: the jump table follows, the step's signature and buffers stay"""
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler
    r = sampler_trace.Run()
    lib = dry.lib()
    smp = ConditionalDDIMSampler(r.model(BF, **sampler_trace.SMALL), S, use_graph=False)
    call = lambda: smp.sample(r.randn(2, T, D), r.randn(2, T, D), _mask())
    call()
    sig, x_ptr = smp._sig, smp._bufs["x"].data_ptr()
    tabs = smp.model.tables(smp._bufs["x"].device)
    for setting, jumps, back in (((2, 2), 2, 2), ((3, 3), 2, 3), (None, 0, None), ((1, 2), 4, 1), ((2, 1), 0, None)):
        smp.resample = setting
        lib.calls.clear()
        lib.args.clear()
        call()
        assert lib.calls.count(NAME) == jumps, setting
        assert smp._sig == sig and smp._bufs["x"].data_ptr() == x_ptr, "the step did not change: nothing is captured again"
        for n, a in lib.args:
            if n == NAME:
                assert a[10] == back and a[4] == tabs.resample_coef.data_ptr() and tabs.resample_jump == back
    smp.resample = (S, 2)
    with pytest.raises(ValueError, match="jump"):
        call()


def test_stitched_and_guided_sequences(dry):
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler, StochasticStitchedSampler
    r = sampler_trace.Run()
    lib = dry.lib()
    m = r.model(BF, **sampler_trace.SMALL)
    smp = StochasticStitchedSampler(m, S, eta=0.0, hop=sampler_trace.HOP, use_graph=False, seed=5, resample=(2, 2))
    cols = _mask()[0].clone()
    lib.calls.clear()
    lib.args.clear()
    smp.sample(r.randn(2, 17, D), r.randn(2, 17, D), cols, trial_ids=[7, 3])
    assert lib.calls.count("ib_stitch_ddim_step") == 9 and lib.calls.count(NAME) == 2
    lay = smp.layout
    (a, _) = [a for n, a in lib.args if n == NAME]
    assert a[13:16] == (lay["start"].data_ptr(), lay["cover"].data_ptr(), smp._bufs["win"].data_ptr())
    assert a[17:21] == (2, lay["W"], T, 17) and smp._bufs["win"].tolist() == [7, 3]
    # guided: every jump is followed by the counter and the mirror
    C = sampler_trace.COND_COLS
    mg = r.model(BF, cond_cols=C, **sampler_trace.SMALL)
    mg.cond_drop = 0.1
    g = ConditionalDDIMSampler(mg, S, use_graph=False, observations="clean", guidance=1.5, resample=(2, 2))
    mask = torch.zeros(T, D, dtype=torch.bool)
    mask[:, :C] = True
    lib.calls.clear()
    g.sample(r.randn(2, T, D), r.randn(2, T, D), mask)
    names = list(lib.calls)
    at = [i for i, n in enumerate(names) if n == NAME]
    assert len(at) == 2 and all(names[i:i + 3] == [NAME, "ib_counter_add", "ib_cfg_mirror"] for i in at)
    assert names.count("ib_cfg_combine") == 9 and names.count("ib_cfg_mirror") == 1 + 9 + 2


def test_one_window_trials_take_the_per_window_update(dry):
    """F == T under resampling: ib_ddim_cond_step, as ConditionalDDIMSampler launches it; the choice is in the signature, so
    the step is captured again when the setting changes.  The plain loop and longer trials keep the stitched entry"""
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler, StochasticStitchedSampler
    r = sampler_trace.Run()
    lib = dry.lib()
    m = r.model(torch.float32, **sampler_trace.SMALL)
    z, obs, cols = r.randn(2, T, D), r.randn(2, T, D), _mask()[0].clone()
    smp = StochasticStitchedSampler(m, S, eta=0.0, hop=sampler_trace.HOP, use_graph=False, seed=5, resample=(2, 2))

    def run(sampler, *a, **kw):
        lib.calls.clear()
        lib.args.clear()
        sampler.sample(*a, **kw)
        return [n for n in lib.calls if n.endswith("_step") or n == NAME], list(lib.args)

    names, args = run(smp, z, obs, cols, trial_ids=[7, 3])
    ref = ConditionalDDIMSampler(m, S, use_graph=False, seed=5, resample=(2, 2))
    want, wargs = run(ref, z, obs, _mask(), window_ids=[7, 3])
    assert names == want and names.count("ib_ddim_cond_step") == 9 and names.count(NAME) == 2
    shape = lambda log, n: [a[-6:-1] for k, a in log if k == n]
    assert shape(args, "ib_ddim_cond_step") == shape(wargs, "ib_ddim_cond_step"), "the same sizes, pitch and dtype"
    sizes = lambda log: [a[7:9] + a[10:12] + a[16:25] for k, a in log if k == NAME]     # everything but the pointers
    assert sizes(args) == sizes(wargs)
    assert "one_window_step" in smp._sig
    on = smp._sig
    smp.resample = None
    names, _ = run(smp, z, obs, cols)
    assert names == ["ib_stitch_ddim_step"] * S and "one_window_step" not in smp._sig and smp._sig != on
    smp.resample = (2, 2)
    names, _ = run(smp, r.randn(2, 17, D), r.randn(2, 17, D), cols)
    assert names.count("ib_stitch_ddim_step") == 9 and "ib_ddim_cond_step" not in names and "one_window_step" not in smp._sig


# ---------------------------------------------------------------------------------------------------------------------
# 4. refusals: samplers, predictor, command line
# ---------------------------------------------------------------------------------------------------------------------
def test_sampler_refusals(dry):
    from inferbiomechanics_amd.diffusion import sampler as mod
    r = sampler_trace.Run()
    m = r.model(BF, **sampler_trace.SMALL)
    with pytest.raises(ValueError, match="eta = 0"):
        mod.ConditionalDDIMSampler(m, S, eta=0.5, resample=(2, 2))
    for solver in ("dpmpp2m", "dpmpp2m_sde"):
        with pytest.raises(ValueError, match="history"):
            mod.ConditionalDDIMSampler(m, S, solver=solver, spacing="logsnr", resample=(2, 2))
    with pytest.raises(ValueError, match="history"):
        mod.StochasticStitchedSampler(m, S, eta=0.0, solver="dpmpp2m_sde", spacing="logsnr", resample=(2, 2))
    with pytest.raises(ValueError, match="eta = 0"):
        mod.StochasticStitchedSampler(m, S, eta=0.5, resample=(2, 2))
    for bad in ((0, 2), (S, 2), (2, 0)):
        with pytest.raises(ValueError, match="resample"):
            mod.ConditionalDDIMSampler(m, S, resample=bad)
    with pytest.raises(ValueError, match=r"StochasticStitchedSampler\(eta=0, resample="):
        mod.StitchedDDIMSampler(m, S, resample=(2, 2))
    with pytest.raises(TypeError):
        mod.StochasticStitchedSampler(m, S, eta=0.0, resamples=(2, 2))
    assert mod.ConditionalDDIMSampler(m, S, eta=0.5, resample=(2, 1)).resample == (2, 1)   # times = 1: the plain loop
    # a call without observations: nothing to harmonise with
    smp = mod.StochasticStitchedSampler(m, S, eta=0.0, resample=(2, 2))
    with pytest.raises(ValueError, match="observations"):
        smp.sample(torch.zeros(1, 17, D))
    assert smp._sig is None, "a refused call leaves the sampler as it was"
    # the attributes may be changed between calls: still refused
    smp = mod.ConditionalDDIMSampler(m, S, resample=(2, 2))
    smp.eta = 0.5
    with pytest.raises(ValueError, match="eta = 0"):
        smp.sample(torch.zeros(2, T, D), torch.zeros(2, T, D), _mask())
    st = mod.StitchedDDIMSampler(m, S)
    st.resample = (2, 2)
    with pytest.raises(ValueError, match="StochasticStitchedSampler"):
        st.sample(torch.zeros(1, 17, D), torch.zeros(1, 17, D), _mask()[0].clone())


def test_predictor_paths(dry):
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import LOSS_KEY_ORDER, LOSS_KEY_WIDTHS
    from inferbiomechanics_amd.models.DiffusionLabelPredictor import DiffusionLabelPredictor
    r = sampler_trace.Run()
    lib = dry.lib()
    m = r.model(BF, **sampler_trace.LABELS)
    with pytest.raises(ValueError, match="eta = 0"):
        DiffusionLabelPredictor(m, S, eta=0.5, resample=(2, 2))
    with pytest.raises(ValueError, match="history"):
        DiffusionLabelPredictor(m, S, solver="dpmpp2m", spacing="logsnr", resample=(2, 2))
    assert DiffusionLabelPredictor(m, S).resample is None and DiffusionLabelPredictor(m, S, resample=(2, 1)).resample is None
    pred = DiffusionLabelPredictor(m, S, seed=11, use_graph=False, resample=(2, 2))
    lib.calls.clear()
    out = pred(sampler_trace._label_inputs(r, 2, 10), draw=3)
    assert [tuple(out[k].shape) for k in LOSS_KEY_ORDER] == [(2, 10, w) for w in LOSS_KEY_WIDTHS]
    assert lib.calls.count(NAME) == 2 and lib.calls.count("ib_ensemble_stats") == 1, "K = 1 takes the id path too"
    assert pred.sampler._bufs["win"].tolist() == pred.member_ids(3, 2) == [3, 4]
    with pytest.raises(ValueError, match="predict_trial_ensemble"):
        pred.predict_trial(sampler_trace._label_inputs(r, 2, 20), hop=4)
    ens = DiffusionLabelPredictor(m, S, seed=11, use_graph=False, resample=(2, 2), num_samples=3)
    lib.calls.clear()
    ens.predict_trial_ensemble(sampler_trace._label_inputs(r, 2, 20), hop=4, draw=1)
    smp = ens._trial_ens[1]
    assert smp.eta == 0.0 and smp.resample == (2, 2) and lib.calls.count(NAME) == 2
    assert smp._bufs["win"].tolist() == ens.member_ids(1, 2) == [3, 4, 5, 6, 7, 8]
    assert ens.last_std is not None


def test_command_line_flags_and_refusals():
    from inferbiomechanics_amd.cli._common import checked_resample
    from inferbiomechanics_amd.cli.analyze import AnalyzeCommand
    from inferbiomechanics_amd.cli.visualize import VisualizeCommand
    for cmd, word in ((AnalyzeCommand(), "analyze"), (VisualizeCommand(), "visualize")):
        parser = argparse.ArgumentParser()
        cmd.register_subcommand(parser.add_subparsers(dest="command"))
        a = parser.parse_args([word])
        assert (a.resample_jump, a.resample_times) == (0, 1) and checked_resample(a, 100, 0.0, "ddim") is None
        a = parser.parse_args([word, "--resample-jump", "2", "--resample-times", "10"])
        assert checked_resample(a, 20, 0.0, "ddim") == (2, 10)
        with pytest.raises(SystemExit, match="--sample-eta 0"):
            checked_resample(a, 20, 0.5, "ddim")
        for solver in ("dpmpp2m", "dpmpp2m_sde"):
            with pytest.raises(SystemExit, match="--sampler ddim"):
                checked_resample(a, 20, 0.0, solver)
        for J, steps in ((20, 20), (25, 20), (-1, 20), (1, 1)):
            with pytest.raises(SystemExit, match="--resample-jump"):
                checked_resample(argparse.Namespace(resample_jump=J, resample_times=3), steps, 0.0, "ddim")
        with pytest.raises(SystemExit, match="--resample-jump"):
            checked_resample(argparse.Namespace(resample_jump=0, resample_times=3), 20, 0.0, "ddim")
        with pytest.raises(SystemExit, match="--resample-times"):
            checked_resample(argparse.Namespace(resample_jump=2, resample_times=0), 20, 0.0, "ddim")


def test_analyze_reaches_the_resampled_loop(dry, tmp_path):
    """`analyze --resample-jump J --resample-times R` on a freshly trained small checkpoint: the jumps are launched"""
    from inferbiomechanics_amd.main import main
    ck = str(tmp_path / "ck")
    base = ['--no-wandb', '--checkpoint-dir', ck, '--data-loading-workers', '0', '--model-type', 'diffusion-mlp',
            '--hidden-dims', '32', '32', '--synthetic-windows', '2']
    assert main(['train', '--feat-dim', '177', '--epochs', '1', '--max-steps', '1', '--batch-size', '4'] + base[:-2]
                + ['--synthetic-windows', '8'])
    lib = dry.lib()
    lib.calls.clear()
    assert main(['analyze', '--sample-steps', '5', '--resample-jump', '2', '--resample-times', '2'] + base)
    assert lib.calls.count(NAME) == 2 * 2 * 2, "two splits, two windows each (one per sampler call), two jumps per call"
    assert lib.calls.count("ib_ddim_cond_step") == 2 * 2 * 9
    for bad, word in ((['--sample-eta', '0.5'], "--sample-eta 0"), (['--sampler', 'dpmpp2m', '--sample-spacing', 'logsnr'],
                                                                      "--sampler ddim")):
        with pytest.raises(SystemExit, match=word):
            main(['analyze', '--sample-steps', '5', '--resample-jump', '2', '--resample-times', '2'] + bad + base)
    with pytest.raises(SystemExit, match="--resample-jump"):
        main(['analyze', '--sample-steps', '5', '--resample-jump', '5', '--resample-times', '2'] + base)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the statistics: the reason for the feature
# ---------------------------------------------------------------------------------------------------------------------
def test_resampling_removes_most_of_the_replacement_bias():
    """2-D Gaussian data with unit variances and correlation 0.9, the analytic optimal denoiser, the first coordinate observed
    at 1.5: the posterior of the second is N(1.35, 0.436^2).  K = 20 000 start draws, S = 20, time grid, eta = 0.  Measured
    when this was written: plain loop mean 0.669, std 0.661 (more steps do not help: S = 100 gives 0.672, 0.708); (jump 2,
    times 10) mean 1.259, std 0.400 in 182 evaluations; (5, 5) mean 1.103, std 0.561 in 80.  The standard error of the mean
    is 0.003."""
    K, S_ = 20000, 20
    mean, std = RR.gaussian_problem(0.9, 1.5)
    assert abs(mean - 1.35) < 1e-12 and abs(std - 0.436) < 1e-3
    plain, e0 = RR.gaussian_walk(S_, None, K)
    res, e1 = RR.gaussian_walk(S_, (2, 10), K)
    mid, e2 = RR.gaussian_walk(S_, (5, 5), K)
    assert (e0, e1, e2) == (20, 182, 80)
    em = lambda x: abs(float(x.mean()) - mean)
    es = lambda x: abs(float(x.std()) - std)
    print(f"plain: mean {plain.mean():.4f} std {plain.std():.4f} | (2, 10): mean {res.mean():.4f} std {res.std():.4f} | "
          f"(5, 5): mean {mid.mean():.4f} std {mid.std():.4f} | posterior {mean:.4f} {std:.4f}")
    assert em(plain) > 0.5, "the replacement method is biased on this problem: that is what is being cured"
    assert em(res) <= 0.25 * em(plain)
    assert es(res) < es(plain)
    assert em(res) < em(mid) < em(plain), "more resampling, less bias"
