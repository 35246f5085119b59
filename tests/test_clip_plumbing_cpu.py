"""Host side of the x0 clip without a GPU: the schedule's tables and rank, the eighth header and the build lists, the
binding's checks, the launch sequence of a clipped step in dry-run traces (off: today's sequence, entry for entry; on: one
more entry between the forward and the update of each of the eight update rows and of the guided step), the capture
signature, the command line's refusals and the checkpoint round trip of column_range."""
import argparse
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import clip_restatement as CR
from tools import sampler_trace

BF = torch.bfloat16
NAMES = ["ib_column_range", "ib_x0_clip_dynamic", "ib_x0_clip_range"]
T, D, C = sampler_trace.SMALL["T"], sampler_trace.SMALL["D"], sampler_trace.COND_COLS
S = sampler_trace.S
INF = float("inf")


@pytest.fixture()
def dry():
    from inferbiomechanics_amd import hip
    hip.set_dry_run(True)
    yield hip
    hip.set_dry_run(False)


# ---------------------------------------------------------------------------------------------------------------------
# 1. schedule: the step table, the per-column tables, the rank
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spacing,steps", [("time", 10), ("time", 100), ("logsnr", 7), ("logsnr", 20)])
def test_x0_coefficients(spacing, steps):
    from inferbiomechanics_amd.diffusion import schedule as sc
    c = sc.x0_coefficients(1000, steps, spacing)
    assert c.dtype == torch.float64 and tuple(c.shape) == (steps, 4)
    ab = sc.alphas_cumprod(1000)[sc.sample_timesteps(1000, steps, spacing)]
    for s in (0, steps // 2, steps - 1):
        a, b = math.sqrt(float(ab[s])), math.sqrt(1.0 - float(ab[s]))
        assert np.allclose(c[s].numpy(), [1.0 / a, b / a, a, 1.0 / b], rtol=1e-14, atol=0.0)
    ia, sa, a, is_ = c.unbind(dim=1)
    assert torch.allclose(ia * a, torch.ones(steps, dtype=torch.float64), rtol=4e-16, atol=0.0)          # before the cast
    assert torch.allclose(sa * is_ * a, torch.ones(steps, dtype=torch.float64), rtol=4e-16, atol=0.0)
    # the data prediction these coefficients state is the one the second-order table's history states
    five = sc.dpmpp_coefficients(1000, steps, spacing)
    assert torch.allclose(five[:, 3], ia, rtol=1e-15) and torch.allclose(five[:, 4], -sa, rtol=1e-15)


def test_clip_rank():
    from inferbiomechanics_amd.diffusion.schedule import clip_rank
    assert clip_rank(0.995, 200) == 199
    assert [clip_rank(1.0, n) for n in (1, 2, 255, 60000)] == [1, 2, 255, 60000]
    assert clip_rank(1e-9, 1000) == 1 and clip_rank(0.5, 1) == 1 and clip_rank(0.5, 10) == 5 and clip_rank(0.51, 10) == 6
    for bad in (0.0, -0.1, 1.0000001, float("nan")):
        with pytest.raises(ValueError):
            clip_rank(bad, 10)
    with pytest.raises(ValueError):
        clip_rank(0.5, 0)


def test_clip_tables():
    from inferbiomechanics_amd.diffusion.schedule import clip_tables
    m, h, ih, b = clip_tables([-1.0, -INF, 2.0, 0.0, -INF, 1.0], [3.0, 5.0, 2.0, INF, INF, 1.5])
    assert b.tolist() == [True, False, False, False, False, True], "infinite on either side and lo == hi are not bounded"
    assert all(v.dtype == torch.float64 for v in (m, h, ih))
    assert (m[0], h[0], ih[0]) == (1.0, 2.0, 0.5) and (m[5], h[5], ih[5]) == (1.25, 0.25, 4.0)
    assert torch.isfinite(m).all() and torch.isfinite(h).all() and torch.isfinite(ih).all()
    assert np.array_equal(CR.bounded([-1.0, -INF, 2.0, 0.0, -INF, 1.0], [3.0, 5.0, 2.0, INF, INF, 1.5]), b.numpy())
    with pytest.raises(ValueError, match="lo > hi"):
        clip_tables([0.0, 2.0], [1.0, 1.0])
    with pytest.raises(ValueError):
        clip_tables([0.0], [1.0, 2.0])
    with pytest.raises(ValueError, match="NaN"):
        clip_tables([float("nan")], [1.0])


def test_x0clip_record_and_set_clip():
    from inferbiomechanics_amd.diffusion.sampler import X0Clip
    from inferbiomechanics_amd.diffusion.schedule import DiffusionTables, x0_coefficients
    q = X0Clip(torch.tensor([-1.0, 0.0]), [1.0, INF], mode="dynamic", quantile=0.9)
    assert q.lo == (-1.0, 0.0) and q.hi == (1.0, INF) and hash(q) == hash(X0Clip([-1.0, 0.0], [1.0, INF], "dynamic", 0.9))
    assert X0Clip([0.0], [1.0]).mode == "range" and X0Clip([0.0], [1.0]).quantile == 0.995
    for bad in (dict(mode="clamp"), dict(quantile=0.0), dict(quantile=1.5)):
        with pytest.raises(ValueError):
            X0Clip([0.0], [1.0], **bad)
    with pytest.raises(ValueError):
        X0Clip([2.0], [1.0])
    tabs = DiffusionTables("cpu", num_sample_steps=10)
    before = {k: v.data_ptr() for k, v in vars(tabs).items() if isinstance(v, torch.Tensor)}
    assert tabs.clip is None and not tabs.clip_serves(10, "time", q.lo, q.hi)
    tabs.set_clip(q.lo, q.hi)
    assert {k: v.data_ptr() for k, v in vars(tabs).items() if isinstance(v, torch.Tensor)} == before, "no other table moves"
    assert tabs.clip_serves(10, "time", q.lo, q.hi) and not tabs.clip_serves(20, "time", q.lo, q.hi)
    assert not tabs.clip_serves(10, "time", q.lo, (1.0, 2.0))
    assert torch.equal(tabs.clip["coef"], x0_coefficients(1000, 10).to(torch.float32)) and tabs.clip["bounded"].tolist() == [True, False]
    assert all(tabs.clip[k].dtype == torch.float32 and tuple(tabs.clip[k].shape) == (2,) for k in ("lo", "hi", "m", "h", "ih"))
    tabs.set_clip(None, None)
    assert tabs.clip is None


# ---------------------------------------------------------------------------------------------------------------------
# 2. the header, the build lists, the binding
# ---------------------------------------------------------------------------------------------------------------------
def test_eighth_header_is_parsed_into_its_own_table_and_built():
    from inferbiomechanics_amd import hip
    assert os.path.basename(hip.CLIP_HEADER_PATH) == "ib_hip_clip.h" and os.path.exists(hip.CLIP_HEADER_PATH)
    assert hip.clip_decls() == NAMES == sorted(hip._CLIP_SIGS)
    others = [t for t in hip._HEADERS if t is not hip._CLIP_SIGS]
    assert len(others) == 7 and hip._CLIP_SIGS in hip._HEADERS
    text = open(hip.CLIP_HEADER_PATH).read()
    for n in NAMES:
        assert len(re.findall(rf"\bint {n}\(", text)) == 1
        assert all(n not in t for t in others), "no name collides with another header's"
        res, args = hip._sig(n)
        assert res is hip._c.c_int and args[-1] is hip._vp and args[-2] is hip._c.c_int and hip._is_launch(n)
    rng, dyn = hip._sig("ib_x0_clip_range")[1], hip._sig("ib_x0_clip_dynamic")[1]
    assert rng == [hip._vp] * 6 + [hip._i64, hip._i32, hip._vp] + [hip._i64] * 4 + [hip._c.c_int, hip._vp]
    assert dyn == rng[:9] + [hip._vp] * 3 + [hip._i64] + rng[9:], "the same operands, then m, h, ih and k"
    mk = open(os.path.join(os.path.dirname(hip.__file__), "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, flags=re.M).group(1).split()
    hdrs = re.search(r"^HDRS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "clip.hip" in srcs and "../../include/ib_hip_clip.h" in hdrs
    for path in (hip.LIB_PATH, hip.AB_LIB_PATH):
        if not os.path.exists(path):
            pytest.fail(f"{path} is not built")
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        assert set(NAMES) <= {line.split()[-1] for line in out.splitlines() if line.strip()}, path
    lib = hip.lib()
    # argument errors are reported before anything is launched (IB_E_ARG = -1)
    assert lib.ib_x0_clip_range(None, None, None, None, None, None, 4, 0, None, 1, 2, 4, 8, 0, None) == -1
    assert lib.ib_x0_clip_dynamic(None, None, None, None, None, None, 4, 0, None, None, None, None, 1, 1, 2, 4, 8, 0, None) == -1
    assert lib.ib_column_range(None, 1, 1, 4, 8, None, 1, None, 0, None) == -1


def test_binding_checks(dry):
    hip, lib = dry, dry.lib()
    x, eps = torch.zeros(2, 3, 8), torch.zeros(2, 3, 8)
    mask, ctr = torch.zeros(3, 8, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32)
    col = lambda: torch.zeros(6)
    lo, hi, m, h, ih, coef = col(), col(), col(), col(), col(), torch.zeros(5, 4)
    hip.x0_clip_range(x, eps, mask, lo, hi, coef, step_dev=ctr, D=6)
    assert lib.args[-1] == ("ib_x0_clip_range", (x.data_ptr(), eps.data_ptr(), mask.data_ptr(), lo.data_ptr(), hi.data_ptr(),
                                                 coef.data_ptr(), 5, 0, ctr.data_ptr(), 2, 3, 6, 8, hip.F32, 0))
    hip.x0_clip_dynamic(x, eps, None, lo, hi, coef, m, h, ih, 18, step=2, D=6)
    assert lib.args[-1] == ("ib_x0_clip_dynamic", (x.data_ptr(), eps.data_ptr(), None, lo.data_ptr(), hi.data_ptr(),
                                                   coef.data_ptr(), 5, 2, None, m.data_ptr(), h.data_ptr(), ih.data_ptr(), 18,
                                                   2, 3, 6, 8, hip.F32, 0))
    table = torch.zeros(4, 24, dtype=BF)
    out = hip.column_range(table, 3, 6)
    name, a = lib.args[-1]
    assert name == "ib_column_range" and a[:5] == (table.data_ptr(), 4, 3, 6, 24) and a[6] == 1 and a[8] == hip.BF16
    assert tuple(out.shape) == (6, 2) and out.dtype == torch.float32
    for bad in (lambda: hip.x0_clip_range(x, eps[:1], mask, lo, hi, coef, D=6),
                lambda: hip.x0_clip_range(x, eps, mask[:2], lo, hi, coef, D=6),
                lambda: hip.x0_clip_range(x, eps, mask, lo[:5], hi, coef, D=6),
                lambda: hip.x0_clip_range(x, eps, mask, lo, hi, coef[:, :2], D=6),
                lambda: hip.x0_clip_range(x, eps, mask, lo, hi, coef, D=9),
                lambda: hip.x0_clip_range(x, eps.to(BF), mask, lo, hi, coef, D=6),
                lambda: hip.x0_clip_dynamic(x, eps, mask, lo, hi, coef, m, h, ih[:3], 1, D=6),
                lambda: hip.x0_clip_dynamic(x, eps, mask, lo, hi, coef, m, h, ih, 0, D=6),
                lambda: hip.x0_clip_dynamic(x, eps, mask, lo, hi, coef, m, h, ih, 19, D=6),
                lambda: hip.column_range(table, 5, 6), lambda: hip.column_range(table[:, :20], 3, 6),
                lambda: hip.column_range(table, 3, 6, out=torch.zeros(6, 3))):
        with pytest.raises(hip.HipError):
            bad()
    assert len(lib.calls) == 3


# ---------------------------------------------------------------------------------------------------------------------
# 3. the launch sequence and the signature
# ---------------------------------------------------------------------------------------------------------------------
UPDATES = {"ib_ddim_step", "ib_ddim_cond_step", "ib_ddim_step_noise", "ib_ddim_cond_step_noise", "ib_dpmpp_step",
           "ib_dpmpp_cond_step", "ib_sde_dpmpp_step", "ib_stitch_ddim_step", "ib_stitch_ddim_step_noise",
           "ib_stitch_dpmpp_step"}


def bounds(mode, quantile=0.995):
    from inferbiomechanics_amd.diffusion.sampler import X0Clip
    lo, hi = [-0.5] * D, [0.5] * D
    lo[25], hi[25] = -INF, INF
    return X0Clip(lo, hi, mode=mode, quantile=quantile)


def traced(hip, make, call):
    """the names of one sample() call of a fresh sampler (eager: S steps of launches), and the sampler"""
    lib = hip.lib()
    smp = make()
    lib.calls.clear()
    call(smp)
    return list(lib.calls), smp


def rows():
    """the eight rows of the update table: (name, expected update entry, constructor, call)"""
    from inferbiomechanics_amd.diffusion import sampler as mod
    r = sampler_trace.Run()
    model = r.model(BF, **sampler_trace.SMALL)
    mask = torch.zeros(T, D, dtype=torch.bool)
    mask[:, :20] = True
    cols = mask[0].clone()
    g = torch.Generator().manual_seed(2)
    z, obs = torch.randn(3, T, D, generator=g), torch.randn(3, T, D, generator=g)
    zt, obst = torch.randn(2, 17, D, generator=g), torch.randn(2, 17, D, generator=g)
    flat = lambda **kw: (lambda **c: mod.ConditionalDDIMSampler(model, S, use_graph=False, seed=5, **kw, **c),
                         lambda s: s.sample(z, obs, mask))
    free = lambda **kw: (lambda **c: mod.DDIMSampler(model, S, use_graph=False, seed=5, **kw, **c), lambda s: s.sample(z))
    st = lambda **kw: (lambda **c: mod.StitchedDDIMSampler(model, S, hop=3, use_graph=False, **kw, **c),
                       lambda s: s.sample(zt, obst, cols))
    sto = lambda **kw: (lambda **c: mod.StochasticStitchedSampler(model, S, hop=3, use_graph=False, seed=5, **kw, **c),
                        lambda s: s.sample(zt, obst, cols))
    return [("flat 1 eta0", "ib_ddim_cond_step", *flat()), ("flat 1 eta0 free", "ib_ddim_step", *free()),
            ("flat 1 eta>0", "ib_ddim_cond_step_noise", *flat(eta=0.5)),
            ("flat 2 eta0", "ib_dpmpp_cond_step", *flat(solver="dpmpp2m", spacing="logsnr")),
            ("flat 2 eta>0", "ib_sde_dpmpp_step", *flat(solver="dpmpp2m_sde", spacing="logsnr", eta=0.5)),
            ("stitched 1 eta0", "ib_stitch_ddim_step", *st()),
            ("stitched 1 eta>0", "ib_stitch_ddim_step_noise", *sto(eta=0.5)),
            ("stitched 2 eta0", "ib_stitch_dpmpp_step", *st(solver="dpmpp2m", spacing="logsnr")),
            ("stitched 2 eta>0", "ib_sde_dpmpp_step", *sto(eta=0.5, solver="dpmpp2m_sde", spacing="logsnr"))]


def test_off_is_todays_sequence_and_on_adds_one_entry_before_every_update(dry):
    for name, update, make, call in rows():
        off, plain = traced(dry, make, call)
        none, _ = traced(dry, lambda: make(x0_clip=None), call)
        assert none == off and not any("x0_clip" in n for n in off), name
        assert off.count(update) == S and sum(n in UPDATES for n in off) == S, name
        for mode, entry in (("range", "ib_x0_clip_range"), ("dynamic", "ib_x0_clip_dynamic")):
            on, smp = traced(dry, lambda: make(x0_clip=bounds(mode)), call)
            assert [n for n in on if n != entry] == off, f"{name}: nothing else changes"
            where = [i for i, n in enumerate(on) if n == entry]
            assert len(where) == S and all(on[i + 1] == update for i in where), f"{name}: one entry, right before the update"
            assert "x0_clip" in smp._sig and mode in smp._sig and "x0_clip" not in plain._sig, name
            assert len(smp._sig) == len(plain._sig) + 9, "the mark, the mode, the rank and six table addresses"
        empty, smp = traced(dry, lambda: make(x0_clip=bounds("range").__class__([-INF] * D, [INF] * D)), call)
        assert empty == off and "x0_clip" in smp._sig, f"{name}: no bounded column, nothing to launch"


def test_guided_step_clips_after_the_combine_over_the_first_half(dry):
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler
    r = sampler_trace.Run()
    model = r.model(BF, cond_cols=C, **sampler_trace.SMALL)
    model.cond_drop = 0.1
    mask = torch.zeros(T, D, dtype=torch.bool)
    mask[:, :C] = True
    g = torch.Generator().manual_seed(2)
    z, obs = torch.randn(3, T, D, generator=g), torch.randn(3, T, D, generator=g)
    make = lambda **c: ConditionalDDIMSampler(model, S, use_graph=False, observations="clean", guidance=1.5, **c)
    call = lambda s: s.sample(z, obs, mask)
    off, _ = traced(dry, make, call)
    on, smp = traced(dry, lambda: make(x0_clip=bounds("dynamic", 0.9)), call)
    assert [n for n in on if n != "ib_x0_clip_dynamic"] == off
    where = [i for i, n in enumerate(on) if n == "ib_x0_clip_dynamic"]
    assert len(where) == S
    for i in where:
        assert on[i - 1] == "ib_cfg_combine" and on[i + 1] == "ib_ddim_cond_step" and on[i + 2] == "ib_cfg_mirror"
    lib = dry.lib()
    a = [a for n, a in lib.args if n == "ib_x0_clip_dynamic"][0]
    xin, eps = smp._bufs["xin"], smp._bufs["eps"]
    assert a[0] == xin.data_ptr() and a[1] == eps.data_ptr() and a[13:17] == (3, T, D, xin.shape[2]), "B windows, not 2B"
    assert a[2] == smp._bufs["mask"].data_ptr() and a[8] == smp._bufs["ctr"].data_ptr()
    from inferbiomechanics_amd.diffusion.schedule import clip_rank
    n = T * (D - C - 1)                                                # the free columns but the unbounded one
    assert a[12] == clip_rank(0.9, n) and smp._sig[-1] == xin.data_ptr(), "the guided entries stay last"


def test_signature_follows_the_bounds_the_mode_and_the_mask(dry):
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler, X0Clip
    r = sampler_trace.Run()
    model = r.model(BF, **sampler_trace.SMALL)
    g = torch.Generator().manual_seed(2)
    z, obs = torch.randn(3, T, D, generator=g), torch.randn(3, T, D, generator=g)
    mask = torch.zeros(T, D, dtype=torch.bool)
    mask[:, :20] = True
    smp = ConditionalDDIMSampler(model, S, use_graph=False, x0_clip=bounds("dynamic", 0.5))
    smp.sample(z, obs, mask)
    first = smp._sig
    smp.sample(z, obs, mask)
    assert smp._sig == first, "the same call again: the same signature"
    mask2 = mask.clone()
    mask2[:, 20:30] = True
    smp.sample(z, obs, mask2)
    assert smp._sig != first, "another mask, another rank: the captured launch bakes it in"
    smp.x0_clip = bounds("range")
    smp.sample(z, obs, mask2)
    assert "range" in smp._sig
    with pytest.raises(ValueError, match="x0_clip"):
        ConditionalDDIMSampler(model, S, x0_clip=X0Clip([0.0] * 3, [1.0] * 3)).sample(z, obs, mask)
    with pytest.raises(ValueError, match="x0_clip"):
        ConditionalDDIMSampler(model, S, x0_clip=([0.0] * D, [1.0] * D))


# ---------------------------------------------------------------------------------------------------------------------
# 4. the command line and the checkpoint
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_flags_and_refusals():
    from inferbiomechanics_amd.cli._common import checked_x0_clip
    from inferbiomechanics_amd.cli.analyze import AnalyzeCommand
    from inferbiomechanics_amd.cli.train import TrainCommand, check_record_range
    from inferbiomechanics_amd.cli.visualize import VisualizeCommand
    parser = argparse.ArgumentParser()
    sub = parser.add_subparsers(dest="command")
    for cmd in (TrainCommand(), AnalyzeCommand(), VisualizeCommand()):
        cmd.register_subcommand(sub)
    rng = torch.stack([-torch.arange(1, 45, dtype=torch.float32), 2.0 * torch.arange(1, 45, dtype=torch.float32)], dim=1)
    with_range, without = argparse.Namespace(column_range=rng), argparse.Namespace(column_range=None)
    for command in ("analyze", "visualize"):
        parse = lambda *a: parser.parse_args([command, "--model-type", "diffusion-transformer"] + list(a))
        d = parse()
        assert (d.x0_clip, d.x0_clip_quantile, d.x0_clip_margin) == ("off", 0.995, 0.0)
        assert checked_x0_clip(d, without) is None and checked_x0_clip(d, with_range) is None
        q = checked_x0_clip(parse("--x0-clip", "dynamic", "--x0-clip-quantile", "0.9"), with_range)
        assert (q.mode, q.quantile, len(q.lo)) == ("dynamic", 0.9, 30) and q.lo[0] == -15.0 and q.hi[-1] == 88.0
        q = checked_x0_clip(parse("--x0-clip", "range", "--x0-clip-margin", "0.5"), with_range)
        assert q.mode == "range" and q.lo[-1] == -44.0 - 0.5 * 66.0 and q.hi[-1] == 88.0 + 0.5 * 66.0
        with pytest.raises(SystemExit, match="--record-range"):
            checked_x0_clip(parse("--x0-clip", "range"), without)
        for bad in ("0", "1.5", "-0.2"):
            with pytest.raises(SystemExit, match="--x0-clip-quantile"):
                checked_x0_clip(parse("--x0-clip", "dynamic", "--x0-clip-quantile", bad), with_range)
        with pytest.raises(SystemExit, match="--x0-clip-margin"):
            checked_x0_clip(parse("--x0-clip", "range", "--x0-clip-margin", "-1"), with_range)
        with pytest.raises(SystemExit):
            parse("--x0-clip", "clamp")
    train = lambda *a: parser.parse_args(["train"] + list(a))
    assert train().record_range is False
    check_record_range(train())
    check_record_range(train("--model-type", "diffusion-mlp", "--record-range", "--window-cache", "hbm"))
    for bad in (("--record-range", "--window-cache", "hbm"), ("--model-type", "diffusion-mlp", "--record-range"),
                ("--model-type", "diffusion-mlp", "--record-range", "--window-cache", "hbm", "--eager")):
        with pytest.raises(SystemExit, match="--record-range"):
            check_record_range(train(*bad))


def test_checkpoint_carries_column_range_only_when_recorded(tmp_path):
    from inferbiomechanics_amd.cli.abstract_command import AbstractCommand
    from inferbiomechanics_amd.cli.train import save_checkpoint
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionMLP

    class Opt:
        def state_dict(self):
            return {}

    model = DiffusionMLP(30, [32], temb_dim=16, temb_hidden=24)
    assert model.column_range is None
    plain = torch.load(save_checkpoint(str(tmp_path / "a"), 0, 1, model, Opt()), map_location="cpu")
    assert "column_range" not in plain
    rng = torch.stack([-torch.arange(30, dtype=torch.float32), torch.arange(30, dtype=torch.float32)], dim=1)
    model.column_range = rng
    ckpt = torch.load(save_checkpoint(str(tmp_path / "b"), 0, 1, model, Opt()), map_location="cpu")
    assert torch.equal(ckpt["column_range"], rng) and ckpt["column_range"].dtype == torch.float32
    # a resumed run: the loaded model holds the checkpoint's record and the next checkpoint keeps it
    fresh = DiffusionMLP(30, [32], temb_dim=16, temb_hidden=24)
    AbstractCommand().load_latest_checkpoint(fresh, checkpoint_dir=str(tmp_path / "b"))
    assert torch.equal(fresh.column_range, rng)
    again = torch.load(save_checkpoint(str(tmp_path / "c"), 1, 1, fresh, Opt()), map_location="cpu")
    assert torch.equal(again["column_range"], rng)
    AbstractCommand().load_latest_checkpoint(fresh, checkpoint_dir=str(tmp_path / "a"))
    assert fresh.column_range is None, "a checkpoint without the key resets it"


def test_train_record_range_end_to_end_in_dry_run(dry, tmp_path):
    """`train --record-range`: one ib_column_range pass over the window cache, the key in every checkpoint; a resumed run
    keeps the checkpoint's record and does not read the cache again; without the flag neither the launch nor the key"""
    import glob
    from inferbiomechanics_amd.main import main
    base = ['--no-wandb', '--synthetic-windows', '24', '--batch-size', '8', '--data-loading-workers', '0', '--model-type',
            'diffusion-mlp', '--feat-dim', '24', '--hidden-dims', '32', '32', '--stride', '1', '--history-len', '6',
            '--compute-dtype', 'bf16', '--seed', '7', '--window-cache', str(tmp_path / "motion.npy")]
    lib = dry.lib()
    latest = lambda d: torch.load(sorted(glob.glob(str(tmp_path / d / "diffusion-mlp" / "*.pt")), key=os.path.getmtime)[-1],
                                  map_location="cpu")
    assert main(['train', '--epochs', '1', '--checkpoint-dir', str(tmp_path / "plain")] + base)
    assert "ib_column_range" not in lib.calls and "column_range" not in latest("plain")
    assert main(['train', '--epochs', '1', '--record-range', '--checkpoint-dir', str(tmp_path / "rec")] + base)
    assert lib.calls.count("ib_column_range") == 1
    first = latest("rec")["column_range"]
    assert tuple(first.shape) == (24, 2) and first.dtype == torch.float32
    lib.calls.clear()
    assert main(['train', '--epochs', '2', '--record-range', '--checkpoint-dir', str(tmp_path / "rec")] + base)
    assert "ib_column_range" not in lib.calls, "the resumed run keeps the checkpoint's record"
    assert torch.equal(latest("rec")["column_range"].view(torch.int32), first.view(torch.int32))
