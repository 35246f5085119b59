"""Host side of classifier-free guidance without a GPU: the fifth header and the Makefile lists, the drop threshold, the
trainer's, the samplers' and the command line's refusals, the checkpoint round trip of cond_drop, and the launch sequence of
the guided step in dry-run traces (tools/sampler_trace.py's instruments): forward over 2B windows, ib_cfg_combine, the row's
update over B windows, ib_cfg_mirror, ib_counter_add -- and at guidance = 0 the unguided sampler's trace, entry for entry."""
import argparse
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import cfg_restatement as CR
from tools import sampler_trace
from tools.plan_trace import _Trace

BF = torch.bfloat16
NAMES = ["ib_cfg_combine", "ib_cfg_mirror", "ib_q_sample_cond_drop"]
T, D, C = sampler_trace.SMALL["T"], sampler_trace.SMALL["D"], sampler_trace.COND_COLS
S = sampler_trace.S


@pytest.fixture()
def dry():
    from inferbiomechanics_amd import hip
    hip.set_dry_run(True)
    yield hip
    hip.set_dry_run(False)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the header, the build lists, the threshold
# ---------------------------------------------------------------------------------------------------------------------
def test_fifth_header_is_parsed_into_its_own_table_and_built():
    from inferbiomechanics_amd import hip
    assert os.path.basename(hip.CFG_HEADER_PATH) == "ib_hip_cfg.h" and os.path.exists(hip.CFG_HEADER_PATH)
    assert hip.cfg_symbols() == NAMES and sorted(hip._CFG_SIGS) == NAMES
    text = open(hip.CFG_HEADER_PATH).read()
    for n in NAMES:
        assert len(re.findall(rf"\bint {n}\(", text)) == 1, f"{n}: one signature per declared symbol"
        assert all(n not in t for t in (hip._SIGS, hip._STITCH_SIGS, hip._HEAD_SIGS, hip._SDE_SIGS))
        res, args = hip._sig(n)
        assert res is hip._c.c_int and args[-1] is hip._vp and args[-2] is hip._c.c_int and hip._is_launch(n)
    q, qd = hip._sig("ib_q_sample_cond")[1], hip._sig("ib_q_sample_cond_drop")[1]
    u64, u32 = hip._c.c_uint64, hip._c.c_uint32
    assert qd == q[:-2] + [u64, hip._i32, hip._vp, u32, u64, hip._vp] + q[-2:], "ib_q_sample_cond's arguments, then the drop's"
    assert hip._sig("ib_cfg_combine")[1] == [hip._vp, hip._f32, hip._i64, hip._i64, hip._c.c_int, hip._vp]
    assert hip._sig("ib_cfg_mirror")[1] == [hip._vp, hip._vp] + [hip._i64] * 5 + [hip._c.c_int, hip._vp]
    mk = open(os.path.join(os.path.dirname(hip.__file__), "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, flags=re.M).group(1).split()
    hdrs = re.search(r"^HDRS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "cfg.hip" in srcs and "../../include/ib_hip_cfg.h" in hdrs
    for path in (hip.LIB_PATH, hip.AB_LIB_PATH):
        if not os.path.exists(path):
            pytest.fail(f"{path} is not built")
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
        assert set(NAMES) <= exported, path
    lib = hip.lib()
    # argument errors are reported before anything is launched (IB_E_ARG = -1)
    assert lib.ib_q_sample_cond_drop(None, None, None, None, None, None, 8, 1, 1, 8, 1000, 3, 1, 0, None, 0, 5, None, 0,
                                     None) == -1
    assert lib.ib_cfg_combine(None, 1.0, 1, 8, 0, None) == -1
    assert lib.ib_cfg_mirror(None, None, 1, 1, 8, 8, 3, 0, None) == -1


def test_drop_domain_is_named_in_philox_h():
    from inferbiomechanics_amd import hip
    text = open(os.path.join(os.path.dirname(hip.__file__), "csrc", "philox.h")).read()
    assert re.search(r"kDomainDrop\s*=\s*3u", text) and CR.DOMAIN_DROP == 3


def test_threshold_values():
    from inferbiomechanics_amd import hip
    assert hip.cond_drop_threshold(0.0) == 0
    assert hip.cond_drop_threshold(1.0) == 1 << 32
    assert hip.cond_drop_threshold(2.0 ** -32) == 1
    assert hip.cond_drop_threshold(0.5) == 1 << 31
    assert hip.cond_drop_threshold(0.1) == int(0.1 * 2 ** 32) == CR.threshold(0.1)
    for bad in (-0.1, 1.0000001, float("nan")):
        with pytest.raises(ValueError):
            hip.cond_drop_threshold(bad)
    # the restated mask: nothing at 0, everything at 1, and the smallest threshold drops exactly the zero words
    assert not CR.drop_mask(64, 0.0, 7, 3, 1).any() and CR.drop_mask(64, 1.0, 7, 3, 1).all()
    assert not CR.drop_mask(64, 2.0 ** -32, 7, 3, 1).any()
    m = CR.drop_mask(64, 0.5, 7, 3, 1)
    assert np.array_equal(CR.drop_mask(8, 0.5, 7, 3, 1), m[:8]), "the decision depends on the window, not on B"
    assert not np.array_equal(CR.drop_mask(64, 0.5, 7, 4, 1), m) and not np.array_equal(CR.drop_mask(64, 0.5, 7, 3, 2), m)


def test_binding_checks(dry):
    hip, lib = dry, dry.lib()
    x0, eps = torch.zeros(2, 3, 8), torch.zeros(2, 3, 8)
    t, tab = torch.zeros(2, dtype=torch.int64), torch.zeros(1000)
    ctr = torch.zeros(1, dtype=torch.int32)
    hip.q_sample_cond_drop(x0, eps, t, tab, tab, torch.empty_like(x0), 3, 0.25, (7 << 32) + 1, step_dev=ctr, stream_id=2,
                           dropped_out=torch.zeros(2, dtype=torch.uint8))
    name, a = lib.args[-1]
    assert name == "ib_q_sample_cond_drop" and a[12:17] == ((7 << 32) + 1, 0, ctr.data_ptr(), 2, 1 << 30)
    with pytest.raises(hip.HipError, match="cond_cols"):
        hip.q_sample_cond_drop(x0, eps, t, tab, tab, torch.empty_like(x0), 8, 0.25, 1)
    with pytest.raises(hip.HipError, match="dropped_out"):
        hip.q_sample_cond_drop(x0, eps, t, tab, tab, torch.empty_like(x0), 3, 0.25, 1, dropped_out=torch.zeros(3, dtype=torch.uint8))
    pair, t2 = torch.zeros(4, 3, 8), torch.zeros(4, dtype=torch.int64)
    hip.cfg_combine(pair, 1.5)
    hip.cfg_mirror(pair, t2, 3, D=6)
    assert lib.args[-2] == ("ib_cfg_combine", (pair.data_ptr(), 1.5, 2, 24, hip.F32, 0))
    assert lib.args[-1] == ("ib_cfg_mirror", (pair.data_ptr(), t2.data_ptr(), 2, 3, 6, 8, 3, hip.F32, 0))
    for bad in (lambda: hip.cfg_combine(torch.zeros(3, 3, 8), 1.0), lambda: hip.cfg_mirror(pair, t2[:2], 3),
                lambda: hip.cfg_mirror(pair, t2, 8), lambda: hip.cfg_mirror(pair, t2, 3, D=9),
                lambda: hip.cfg_mirror(pair[:, :, :6], t2, 3)):
        with pytest.raises(hip.HipError):
            bad()
    assert len(lib.calls) == 3


# ---------------------------------------------------------------------------------------------------------------------
# 2. the trainer
# ---------------------------------------------------------------------------------------------------------------------
def _mlp():
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionMLP
    return DiffusionMLP(30, [32, 48], temb_dim=16, temb_hidden=24)


def _batch(B=3, Tw=7, Dw=30):
    g = torch.Generator().manual_seed(1)
    return (torch.randn(B, Tw, Dw, generator=g), torch.randint(0, 1000, (B,), generator=g), torch.randn(B, Tw, Dw, generator=g))


def test_trainer_refusals(dry):
    from inferbiomechanics_amd.engine import HipTrainer
    from inferbiomechanics_amd.models.FeedForwardRegressionBaseline import FeedForwardBaseline
    for p in (-0.1, 1.5):
        with pytest.raises(ValueError, match="cond_drop"):
            HipTrainer(_mlp(), "diffusion", "sgd", 1e-2, use_graph=False, cond_cols=5, cond_drop=p)     # p out of range
    with pytest.raises(ValueError, match="cond_cols"):
        HipTrainer(_mlp(), "diffusion", "sgd", 1e-2, use_graph=False, cond_cols=0, cond_drop=0.1)       # nothing to drop
    args = argparse.Namespace(predict_grf_components=list(range(6)), predict_cop_components=list(range(6)),
                              predict_moment_components=list(range(6)), predict_wrench_components=list(range(12)))
    m = FeedForwardBaseline(23, 2, 50, "all_frames", "sigmoid", 5, 10, hidden_dims=[32])
    with pytest.raises(ValueError):
        HipTrainer(m, "regression", "sgd", 1e-2, args=args, use_graph=False, cond_drop=0.1)
    assert HipTrainer(_mlp(), "diffusion", "sgd", 1e-2, use_graph=False, cond_cols=5).cond_drop == 0.0


def test_trainer_swaps_exactly_one_launch(dry):
    from inferbiomechanics_amd.engine import HipTrainer
    lib = dry.lib()

    def names(**kw):
        torch.manual_seed(3)
        tr = HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, cond_cols=5, **kw)
        lib.calls.clear()
        lib.args.clear()
        tr.step(_batch())
        return tr, list(lib.calls), list(lib.args)

    _, plain, _ = names()
    _, zero, _ = names(cond_drop=0.0)
    assert zero == plain and "ib_q_sample_cond_drop" not in plain
    tr, drop, args = names(cond_drop=0.25)
    assert [("ib_q_sample_cond" if n == "ib_q_sample_cond_drop" else n) for n in drop] == plain
    assert drop.count("ib_q_sample_cond_drop") == 1
    (a,) = [a for n, a in args if n == "ib_q_sample_cond_drop"]
    # keyed like the step's draw: the trainer's seed, its device-resident step word, its rank
    assert a[12:18] == (tr.noise_seed, 0, tr.step_dev.data_ptr(), tr.noise_stream, 1 << 30, None) and a[11] == 5
    assert ("cond_drop", 0.25) in tr._sig and ("cond_cols", 5) in tr._sig
    assert not any(k[0] == "cond_drop" for k in names(cond_drop=0.0)[0]._sig)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the command line and the checkpoint
# ---------------------------------------------------------------------------------------------------------------------
def test_cond_drop_flag_validation():
    from inferbiomechanics_amd.cli.train import TrainCommand, check_cond_drop
    parser = argparse.ArgumentParser()
    TrainCommand().register_subcommand(parser.add_subparsers(dest="command"))
    parse = lambda *a: parser.parse_args(["train", "--model-type", "diffusion-mlp"] + list(a))
    assert parse().cond_drop == 0.0
    check_cond_drop(parse())
    check_cond_drop(parse("--cond-cols", "10", "--cond-drop", "0.1"))
    check_cond_drop(parse("--cond-cols", "10", "--cond-drop", "1"))
    with pytest.raises(SystemExit, match="--eager"):
        check_cond_drop(parse("--cond-cols", "10", "--cond-drop", "0.1", "--eager"))
    for bad in (("--cond-drop", "0.1"), ("--cond-cols", "10", "--cond-drop", "1.5"), ("--cond-cols", "10", "--cond-drop", "-0.5")):
        with pytest.raises(SystemExit, match="--cond-drop"):
            check_cond_drop(parse(*bad))
    with pytest.raises(SystemExit, match="--cond-drop"):
        check_cond_drop(parser.parse_args(["train", "--cond-cols", "10", "--cond-drop", "0.1"]))       # feedforward


def test_checkpoint_carries_cond_drop(tmp_path):
    from inferbiomechanics_amd.cli.abstract_command import AbstractCommand
    from inferbiomechanics_amd.cli.train import save_checkpoint
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionMLP

    class Opt:
        def state_dict(self):
            return {}

    make = lambda: DiffusionMLP(40, [32], temb_dim=16, temb_hidden=24)
    m = make()
    assert m.cond_drop == 0.0
    d0, d1 = str(tmp_path / "plain"), str(tmp_path / "drop")
    m.cond_cols = 10
    assert "cond_drop" not in torch.load(save_checkpoint(d0, 0, 1, m, Opt()))
    m.cond_drop = 0.125
    saved = torch.load(save_checkpoint(d1, 0, 1, m, Opt()))
    assert saved["cond_drop"] == 0.125 and saved["cond_cols"] == 10
    cmd, fresh = AbstractCommand(), make()
    cmd.load_latest_checkpoint(fresh, checkpoint_dir=d1)
    assert fresh.cond_drop == 0.125 and fresh.cond_cols == 10
    cmd.load_latest_checkpoint(fresh, checkpoint_dir=d0)       # no key: 0
    assert fresh.cond_drop == 0.0


def test_cli_trains_with_cond_drop_and_refuses_another_value_on_resume(dry, tmp_path):
    from inferbiomechanics_amd.main import main
    ck = tmp_path / "ck"
    base = ['--no-wandb', '--synthetic-windows', '24', '--batch-size', '8', '--checkpoint-dir', str(ck),
            '--data-loading-workers', '0', '--model-type', 'diffusion-mlp', '--feat-dim', '24', '--hidden-dims', '32', '32',
            '--stride', '1', '--history-len', '6', '--compute-dtype', 'bf16', '--seed', '7', '--max-steps', '2',
            '--cond-cols', '10']
    lib = dry.lib()
    lib.calls.clear()
    assert main(['train', '--epochs', '1', '--cond-drop', '0.25'] + base)
    # two training steps with the drop; the dev-set evaluation keeps the conditional launch
    assert lib.calls.count("ib_q_sample_cond_drop") == 2 and lib.calls.count("ib_q_sample_cond") >= 1
    (name,) = os.listdir(ck / "diffusion-mlp")
    saved = torch.load(ck / "diffusion-mlp" / name)
    assert saved["cond_drop"] == 0.25 and saved["cond_cols"] == 10
    with pytest.raises(SystemExit, match=r"trained with --cond-drop 0\.25, this run asks for 0\.5"):
        main(['train', '--epochs', '2', '--cond-drop', '0.5'] + base)
    with pytest.raises(SystemExit, match=r"trained with --cond-drop 0\.25, this run asks for 0\.0"):
        main(['train', '--epochs', '2'] + base)
    with pytest.raises(SystemExit, match="--eager"):
        main(['train', '--epochs', '2', '--cond-drop', '0.25', '--eager'] + base)
    assert main(['train', '--epochs', '2', '--cond-drop', '0.25'] + base)


def test_analyze_and_visualize_refuse_guidance_without_cond_drop():
    from inferbiomechanics_amd.cli._common import checked_guidance
    from inferbiomechanics_amd.cli.analyze import AnalyzeCommand
    from inferbiomechanics_amd.cli.visualize import VisualizeCommand
    for cmd, word in ((AnalyzeCommand(), "analyze"), (VisualizeCommand(), "visualize")):
        parser = argparse.ArgumentParser()
        cmd.register_subcommand(parser.add_subparsers(dest="command"))
        assert parser.parse_args([word]).guidance == 0.0
        assert parser.parse_args([word, "--guidance", "1.5"]).guidance == 1.5
    m = _mlp()
    assert checked_guidance(argparse.Namespace(guidance=0.0), m) == 0.0
    with pytest.raises(SystemExit, match="train --cond-drop"):
        checked_guidance(argparse.Namespace(guidance=1.5), m)
    m.cond_drop = 0.1
    assert checked_guidance(argparse.Namespace(guidance=1.5), m) == 1.5


# ---------------------------------------------------------------------------------------------------------------------
# 4. the samplers
# ---------------------------------------------------------------------------------------------------------------------
def _model(r, dtype, cond_drop=0.1):
    m = r.model(dtype, cond_cols=C, **sampler_trace.SMALL)
    m.cond_drop = cond_drop
    return m


def _mask():
    mask = torch.zeros(T, D, dtype=torch.bool)
    mask[:, :C] = True
    return mask


def test_sampler_refusals(dry):
    from inferbiomechanics_amd.diffusion import sampler as mod
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    m = DiffusionTransformer(D, T, d_model=64, num_heads=4, dim_feedforward=128, num_layers=2, compute_dtype=BF)
    m.cond_cols, m.cond_drop = C, 0.1
    makers = (lambda **kw: mod.ConditionalDDIMSampler(m, S, **kw), lambda **kw: mod.StitchedDDIMSampler(m, S, hop=3, **kw),
              lambda **kw: mod.StochasticStitchedSampler(m, S, eta=0.5, hop=3, **kw))
    for make in makers:
        assert make().guidance == 0.0 and make(observations="clean", guidance=1.5).guidance == 1.5
        with pytest.raises(ValueError, match="observations='clean'"):
            make(guidance=1.5)                                                       # 'noised' observations
        with pytest.raises(ValueError):
            make(observations="clean", guidance=float("inf"))
    m.cond_drop = 0.0
    for make in makers:
        with pytest.raises(ValueError, match="train --cond-drop"):
            make(observations="clean", guidance=1.5)                                 # the model never saw the null condition
        assert make(observations="clean", guidance=0.0).guidance == 0.0
    m.cond_drop = 0.1
    smp = makers[0](observations="clean", guidance=1.5)
    smp.observations = "noised"                                                      # changed between calls: still refused
    with pytest.raises(ValueError, match="guidance"):
        smp.sample(torch.zeros(2, T, D), torch.zeros(2, T, D), _mask())
    with pytest.raises(ValueError, match="guidance"):
        makers[1](observations="clean", guidance=1.5).sample(torch.zeros(2, 17, D))   # no observations at all


def _steps(names):
    """the launches of a trace cut after every ib_counter_add, the head of the call (what precedes the first forward) off"""
    out, cur = [], []
    for n in names:
        cur.append(n)
        if n == "ib_counter_add":
            out.append(cur)
            cur = []
    return out


UPDATES = {("ddim", 0.0): "ib_ddim_cond_step", ("ddim", 0.5): "ib_ddim_cond_step_noise", ("dpmpp2m", 0.0): "ib_dpmpp_cond_step",
           ("dpmpp2m_sde", 0.5): "ib_sde_dpmpp_step"}


@pytest.mark.parametrize("dtype", [BF, torch.float32])
@pytest.mark.parametrize("solver,spacing,eta", [s for s in sampler_trace.SETTINGS if (s[0], s[2]) in UPDATES])
def test_guided_per_window_trace(dtype, solver, spacing, eta):
    """the guided step is the unguided step's launches at 2B windows with the seam around the update"""
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler
    B = 3

    def trace(guidance):
        with _Trace() as tr, sampler_trace.Run(tr) as r:
            smp = ConditionalDDIMSampler(_model(r, dtype), S, use_graph=False, eta=eta, seed=5, solver=solver, spacing=spacing,
                                         observations="clean", **({} if guidance is None else {"guidance": guidance}))
            smp.sample(r.randn(B, T, D), r.randn(B, T, D), _mask())
            smp.sample(r.randn(B, T, D), r.randn(B, T, D), _mask())
            return tr.canonical(), list(tr.log), smp

    plain, _, _ = trace(None)
    zero, _, s0 = trace(0.0)
    assert zero == plain, "guidance = 0 is the unguided sampler: launches, arguments, signature, buffers"
    assert "xin" not in s0._bufs and "cfg" not in s0._sig
    canon, log, smp = trace(1.5)
    names = [e if isinstance(e, str) else e[0] for e in canon]
    pnames = [e if isinstance(e, str) else e[0] for e in plain]
    upd = UPDATES[(solver, eta)]
    gsteps, psteps = _steps(names), _steps(pnames)
    assert len(gsteps) == len(psteps) == 2 * S
    for k, (g, p) in enumerate(zip(gsteps, psteps)):
        if k % S == 0:                   # the call's head: the unguided one, then one eager ib_cfg_mirror
            cut = g.index("ib_cfg_mirror")
            head, g = g[:cut], g[cut + 1:]
            assert head == p[:len(head)] and head[-1] == "ib_fill_i64"
            p = p[len(head):]
        assert g[-4:] == ["ib_cfg_combine", upd, "ib_cfg_mirror", "ib_counter_add"], (k, g[-5:])
        assert p[-2:] == [upd, "ib_counter_add"]
        assert g[:-4] == p[:-2], "the forward's launches are the unguided forward's"
    b = smp._bufs
    Dp = b["xin"].shape[-1]
    assert tuple(b["xin"].shape) == tuple(b["eps"].shape) == (2 * B, T, Dp) and tuple(b["t"].shape) == (2 * B,)
    assert b["x"].data_ptr() == b["xin"].data_ptr() and tuple(b["x"].shape) == (B, T, Dp)
    assert smp._sig[-4:] == ("cfg", 1.5, C, b["xin"].data_ptr())
    code = hip.BF16 if dtype == BF else hip.F32
    comb = [a for n, a in log if n == "ib_cfg_combine"]
    mirr = [a for n, a in log if n == "ib_cfg_mirror"]
    upds = [a for n, a in log if n == upd]
    assert len(comb) == 2 * S and len(mirr) == 2 * S + 2 and len(upds) == 2 * S
    assert all(a == (b["eps"].data_ptr(), 1.5, B, T * Dp, code, 0) for a in comb)
    assert all(a == (b["xin"].data_ptr(), b["t"].data_ptr(), B, T, D, Dp, C, code, 0) for a in mirr)
    # the update runs over the first half: state, noise and the B timesteps it writes
    for a in upds:
        assert a[0] == b["xin"].data_ptr() and a[1] == b["eps"].data_ptr() and b["t"].data_ptr() in a
        assert 2 * B not in a[2:] or solver == "dpmpp2m_sde"
    # the forward saw 2B windows: its last GEMM, the output projection, writes 2B * T rows into the noise buffer
    last = [a for n, a in log if n == "ib_linear_fwd"][-1]
    assert 2 * B * T in last and b["eps"].data_ptr() in last


@pytest.mark.parametrize("stochastic", [False, True])
def test_guided_stitched_trace(stochastic):
    from inferbiomechanics_amd.diffusion.sampler import StitchedDDIMSampler, StochasticStitchedSampler
    N, F = 2, 17

    def trace(guidance):
        with _Trace() as tr, sampler_trace.Run(tr) as r:
            kw = dict(hop=sampler_trace.HOP, use_graph=False, observations="clean", seed=5)
            kw.update({} if guidance is None else {"guidance": guidance})
            m = _model(r, BF)
            smp = StochasticStitchedSampler(m, S, eta=0.5, **kw) if stochastic else StitchedDDIMSampler(m, S, **kw)
            smp.sample(r.randn(N, F, D), r.randn(N, F, D), _mask()[0].clone())
            return tr.canonical(), list(tr.log), smp

    plain, _, _ = trace(None)
    zero, _, _ = trace(0.0)
    assert zero == plain
    canon, log, smp = trace(1.5)
    upd = "ib_stitch_ddim_step_noise" if stochastic else "ib_stitch_ddim_step"
    names = [e if isinstance(e, str) else e[0] for e in canon]
    gsteps = _steps(names)
    assert len(gsteps) == S
    for g in gsteps:
        assert g[-4:] == ["ib_cfg_combine", upd, "ib_cfg_mirror", "ib_counter_add"]
    W = smp.layout["W"]
    b = smp._bufs
    assert tuple(b["xin"].shape[:2]) == (2 * N * W, T) and names.count("ib_cfg_mirror") == S + 1
    # the start: ib_ddim_cond_init, then the eager mirror (after the first-copy invariant, which launches nothing here)
    assert names.index("ib_ddim_cond_init") < names.index("ib_cfg_mirror") < names.index("ib_cfg_combine")
    (u0,) = [a for n, a in log if n == upd][:1]
    assert u0[0] == b["xin"].data_ptr() and u0[1] == b["eps"].data_ptr()


def test_predictor_passes_guidance_to_every_sampler(dry):
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    from inferbiomechanics_amd.models.DiffusionLabelPredictor import DiffusionLabelPredictor
    Dl, Tl = sampler_trace.LABELS["D"], sampler_trace.LABELS["T"]
    m = DiffusionTransformer(Dl, Tl, d_model=64, num_heads=4, dim_feedforward=128, num_layers=2, compute_dtype=BF)
    m.cond_cols = Dl - 30
    with pytest.raises(ValueError, match="train --cond-drop"):
        DiffusionLabelPredictor(m, S, guidance=1.5)
    m.cond_drop = 0.1
    r = sampler_trace.Run()
    lib = dry.lib()
    pred = DiffusionLabelPredictor(m, S, seed=11, use_graph=False, guidance=1.5)
    assert pred.sampler.guidance == 1.5
    out = pred(sampler_trace._label_inputs(r, 2, 10))
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import LOSS_KEY_ORDER, LOSS_KEY_WIDTHS
    assert [tuple(out[k].shape) for k in LOSS_KEY_ORDER] == [(2, 10, w) for w in LOSS_KEY_WIDTHS]
    assert lib.calls.count("ib_cfg_combine") == S
    pred.predict_trial(sampler_trace._label_inputs(r, 2, 20), hop=4)
    assert pred._trial[1].guidance == 1.5 and lib.calls.count("ib_cfg_combine") == 2 * S
    ens = DiffusionLabelPredictor(m, S, seed=11, use_graph=False, guidance=1.5, eta=1.0, num_samples=3)
    ens.predict_trial_ensemble(sampler_trace._label_inputs(r, 2, 20), hop=4)
    assert ens._trial_ens[1].guidance == 1.5 and lib.calls.count("ib_cfg_combine") == 3 * S
    assert DiffusionLabelPredictor(m, S).sampler.guidance == 0.0
