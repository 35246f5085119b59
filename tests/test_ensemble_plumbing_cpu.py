"""Host side of the ensemble order statistics without a GPU: the seventh header and the Makefile lists, the refusals of
ib_ensemble_order through its C-ABI argument path, the plotting positions (diffusion/ensemble.py), the restatement
(tests/ensemble_restatement.py) against its float64 reference and against what can be derived for a calibrated Gaussian
ensemble, the predictor's and the command line's plumbing in dry-run mode, and the kernels' register budget."""
import argparse
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import ensemble_restatement as ER
from tools import sampler_trace

NAME = "ib_ensemble_order"
OK, ARG, DTYPE, UNSUPPORTED = 0, -1, -2, -5
F32, BF16, BAD = 0, 1, 7
S = sampler_trace.S

_buf = ctypes.create_string_buffer(1 << 12)
P = ctypes.cast(_buf, ctypes.c_void_p).value // 64 * 64 + 64          # aligned, non-null, alive for the whole module


@pytest.fixture()
def dry():
    from inferbiomechanics_amd import hip
    hip.set_dry_run(True)
    yield hip
    hip.set_dry_run(False)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the header, the build lists, the exports
# ---------------------------------------------------------------------------------------------------------------------
def test_seventh_header_is_parsed_into_its_own_table_and_built():
    from inferbiomechanics_amd import hip
    assert os.path.basename(hip.ENSEMBLE_HEADER_PATH) == "ib_hip_ensemble.h" and os.path.exists(hip.ENSEMBLE_HEADER_PATH)
    assert hip.ensemble_symbols() == [NAME] == sorted(hip._ENSEMBLE_SIGS)
    assert all(NAME not in t for t in hip._TABLES), "the other six tables keep their names"
    assert len(hip._SIGS) == 127
    include = os.path.dirname(hip.ENSEMBLE_HEADER_PATH)
    count = sum(len(re.findall(rf"\bint {NAME}\(", open(os.path.join(include, f)).read())) for f in os.listdir(include))
    assert count == 1, "the symbol is declared once across all headers"
    res, args = hip._sig(NAME)
    vp, i64, i32, f32, ci = hip._vp, hip._i64, hip._i32, hip._f32, hip._c.c_int
    assert res is ci and hip._is_launch(NAME)
    assert args == [vp] * 8 + [i64] * 6 + [i32, f32] * 3 + [ci, vp]
    assert hip.ENSEMBLE_KMAX == 64
    mk = open(os.path.join(os.path.dirname(hip.__file__), "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, flags=re.M).group(1).split()
    hdrs = re.search(r"^HDRS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "ensemble.hip" in srcs and "../../include/ib_hip_ensemble.h" in hdrs


def test_both_builds_export_the_symbol():
    import subprocess
    from inferbiomechanics_amd import hip
    for path in (hip.LIB_PATH, hip.AB_LIB_PATH):
        if not os.path.exists(path):
            pytest.fail(f"{path} is not built")
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        assert NAME in {line.split()[-1] for line in out.splitlines() if line.strip()}, path


# ---------------------------------------------------------------------------------------------------------------------
# 2. refusals: every call carries a defect, so nothing is launched
# ---------------------------------------------------------------------------------------------------------------------
VALID = dict(x=P, y=P, q_lo=P, q_med=P, q_hi=P, crps=P, rank=P, inside=P, B=2, K=8, rows=3, ld=16, c0=6, w=10,
             i_lo=0, f_lo=0.25, i_med=3, f_med=0.5, i_hi=7, f_hi=0.0, dtype=F32, stream=None)
_SCORE = ("y", "crps", "rank", "inside")
CASES = (
    [({k: None}, ARG) for k in ("x", "q_lo", "q_med", "q_hi")]
    + [({k: None}, ARG) for k in _SCORE]                                               # one of the four missing
    + [({k: None for k in _SCORE if k != keep}, ARG) for keep in _SCORE]               # one of the four alone
    + [({"y": None, "crps": None}, ARG)]
    + [(d, ARG) for d in (dict(B=0), dict(B=-1), dict(rows=0), dict(w=0), dict(w=-2), dict(K=0), dict(K=-1), dict(c0=-1),
                          dict(c0=7), dict(w=11), dict(c0=16, w=1), dict(ld=15))]
    + [({k: v}, ARG) for k in ("i_lo", "i_med", "i_hi") for v in (-1, 8, 64)]
    + [(dict(K=1, i_lo=0, i_med=0, i_hi=1), ARG), (dict(K=65, i_hi=65), ARG)]
    + [(d, DTYPE) for d in (dict(dtype=BAD), dict(dtype=2), dict(dtype=-1), dict(dtype=BAD, K=65))]
    + [(d, UNSUPPORTED) for d in (dict(K=65), dict(K=65, i_hi=64), dict(K=1000, dtype=BF16))]
    # two defects: arguments are refused before the dtype, the dtype before the member limit
    + [(d, ARG) for d in (dict(x=None, dtype=BAD), dict(B=0, dtype=BAD), dict(i_med=9, dtype=BAD), dict(y=None, dtype=BAD),
                          dict(w=0, K=65), dict(x=None, K=65))]
)


def _id(case):
    return "+".join(f"{k}={v}" for k, v in case[0].items()) + f"->{case[1]}"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_refusal(case):
    from inferbiomechanics_amd import hip
    defects, code = case
    args = dict(VALID)
    assert set(defects) <= set(args)
    args.update(defects)
    assert len(args) == len(hip._ENSEMBLE_SIGS[NAME][1])
    assert getattr(hip.lib(), NAME)(*args.values()) == code


def test_quantiles_alone_is_a_valid_call_shape(dry):
    """y, crps, rank, inside all NULL passes the argument checks (dry run: the call is recorded, nothing is launched)"""
    args = dict(VALID, **{k: None for k in _SCORE})
    assert getattr(dry.lib(), NAME)(*args.values()) == OK


# ---------------------------------------------------------------------------------------------------------------------
# 3. the plotting positions
# ---------------------------------------------------------------------------------------------------------------------
def test_quantile_position_and_coverage():
    from inferbiomechanics_amd.diffusion.ensemble import calibrated_coverage, interval_levels, quantile_position
    assert [quantile_position(q, 9) for q in (0.1, 0.5, 0.9)] == [(0, 0.0), (4, 0.0), (8, 0.0)]
    assert quantile_position(0.1, 8) == (0, 0.0), "clipped: eight members have no 10 % quantile"
    assert quantile_position(0.9, 8) == (7, 0.0)
    for K in (2, 4, 8, 64):
        assert quantile_position(0.5, K) == (K // 2 - 1, 0.5)
    assert quantile_position(0.5, 1) == (0, 0.0) and quantile_position(0.0, 5) == (0, 0.0) and quantile_position(1.0, 5) == (4, 0.0)
    for K in range(1, 70):
        for q in np.linspace(0, 1, 41):
            i, f = quantile_position(float(q), K)
            assert 0 <= i <= K - 1 and 0.0 <= f <= 1.0 and (i < K - 1 or f == 0.0) and float(np.float32(f)) == f
    assert interval_levels(0.8) == ((1 - 0.8) / 2, 0.5, (1 + 0.8) / 2)
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan"), "x", None):
        with pytest.raises(ValueError):
            interval_levels(bad)
    assert calibrated_coverage(0.8, 9) == 0.8 and calibrated_coverage(0.8, 8) == 7 / 9
    assert calibrated_coverage(0.5, 3) == 0.5 and calibrated_coverage(0.9, 2) == 1 / 3
    assert calibrated_coverage(0.8, 1) == 0.0, "one member is no interval"
    with pytest.raises(ValueError):
        quantile_position(0.5, 0)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the restatement
# ---------------------------------------------------------------------------------------------------------------------
def _pos(L, K):
    from inferbiomechanics_amd.diffusion.ensemble import interval_levels, quantile_position
    return [quantile_position(q, K) for q in interval_levels(L)]


@pytest.mark.parametrize("K", [1, 2, 3, 5, 8, 9, 17, 33, 64])
def test_restatement_against_the_float64_reference(K):
    rng = np.random.default_rng(100 + K)
    n = 4000
    m = (rng.standard_normal((K, n)) * rng.choice([1e-3, 1.0, 50.0], size=n)).astype(np.float32)
    m[:, :200] = np.round(m[:, :200])                                  # repeated values
    y = (rng.standard_normal(n) * 2).astype(np.float32)
    y[:100] = m[0, :100]                                               # the truth equal to a member
    pos = _pos(0.8, K)
    got, ref = ER.restate(m, pos, y), ER.reference(m, pos, y)
    assert np.array_equal(got["rank"], ref["rank"]) and got["rank"].max() <= K
    for k in ("lo", "median", "hi"):
        s = np.abs(np.sort(m.astype(np.float64), axis=0))
        assert np.all(np.abs(got[k] - ref[k]) <= 6 * ER.U * s.max(axis=0)), k   # three roundings, of values up to 2 max |s|
    bound = ER.crps_bound(m, y)
    err = np.abs(got["crps"].astype(np.float64) - ref["crps"])
    print(f"K = {K}: worst CRPS error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert np.all(err <= bound)
    if K > 1:
        wgt = np.abs(2.0 * np.arange(K) - K + 1)[:, None]
        gb = (K + 2) * ER.U * (wgt * np.abs(np.sort(m.astype(np.float64), axis=0))).sum(axis=0)
        assert np.all(np.abs(got["G"].astype(np.float64) - ref["G"]) <= gb), "G = sum_{i<j} (s_j - s_i)"
    # where no position is clipped the quantiles are numpy's type 6
    if K >= 9:
        from inferbiomechanics_amd.diffusion.ensemble import interval_levels
        for k, q in zip(("lo", "median", "hi"), interval_levels(0.8)):
            want = np.quantile(m.astype(np.float64), q, axis=0, method="weibull")
            scale = np.abs(m).max(axis=0).astype(np.float64)
            assert np.all(np.abs(ref[k] - want) <= 1e-6 * scale), k


def test_a_calibrated_gaussian_ensemble_scores_what_it_must():
    """y and K = 9 members iid N(0, 1): coverage of the 80 % interval is 0.8, the rank is uniform on 0 .. 9, the mean fair CRPS
    is 1 / sqrt(pi).  Measured with this seed: coverage 0.7999, every rank bin within 1.4 standard errors, mean CRPS 0.56466
    against 0.56419 (its standard error is 0.0010)."""
    N, K, L = 200_000, 9, 0.8
    rng = np.random.default_rng(20141)
    m = rng.standard_normal((K, N)).astype(np.float32)
    y = rng.standard_normal(N).astype(np.float32)
    pos = _pos(L, K)
    assert pos == [(0, 0.0), (4, 0.0), (8, 0.0)]
    got = ER.restate(m, pos, y)
    cov = float(got["inside"].mean())
    print(f"coverage {cov:.4f}")
    assert abs(cov - L) <= 5 * math.sqrt(0.16 / N)
    hist = np.bincount(got["rank"], minlength=K + 1)
    assert hist.sum() == N and len(hist) == K + 1
    se = math.sqrt(0.1 * 0.9 / N)
    print("rank bins, in standard errors:", np.round((hist / N - 0.1) / se, 2).tolist())
    assert np.all(np.abs(hist / N - 0.1) <= 5 * se)
    ref = ER.reference(m, pos, y)["crps"]
    mean = float(got["crps"].astype(np.float64).mean())
    print(f"mean CRPS {mean:.5f}, 1 / sqrt(pi) {1 / math.sqrt(math.pi):.5f}")
    assert abs(mean - 1 / math.sqrt(math.pi)) <= 5 * float(ref.std(ddof=1)) / math.sqrt(N)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the binding, the predictor and the command line in dry-run mode
# ---------------------------------------------------------------------------------------------------------------------
def test_binding_checks(dry):
    hip, lib = dry, dry.lib()
    B, K, rows, ld = 2, 8, 3, 16
    x = torch.zeros(B, K, rows, ld, dtype=torch.bfloat16)
    truth = torch.zeros(B, rows, 10)
    out = hip.ensemble_order(x, (6, 10), 0.8, truth)
    assert sorted(out) == ["crps", "hi", "inside", "lo", "median", "rank"]
    assert all(tuple(t.shape) == (B, rows, 10) and t.is_contiguous() for t in out.values())
    assert [out[k].dtype for k in ("lo", "median", "hi", "crps", "rank", "inside")] == [torch.float32] * 4 + [torch.uint8] * 2
    name, a = lib.args[-1]
    assert name == NAME
    assert a == (x.data_ptr(), truth.data_ptr(), out["lo"].data_ptr(), out["median"].data_ptr(), out["hi"].data_ptr(),
                 out["crps"].data_ptr(), out["rank"].data_ptr(), out["inside"].data_ptr(), B, K, rows, ld, 6, 10,
                 0, 0.0, 3, 0.5, 7, 0.0, hip.BF16, 0)
    out = hip.ensemble_order(x.float(), (0, 16), 0.5)
    assert sorted(out) == ["hi", "lo", "median"] and lib.args[-1][1][1] is None and lib.args[-1][1][5:8] == (None, None, None)
    assert lib.args[-1][1][14:20] == (1, 0.25, 3, 0.5, 5, 0.75) and lib.args[-1][1][20] == hip.F32
    for bad in (lambda: hip.ensemble_order(x[:, :, :, :8], (0, 8), 0.8), lambda: hip.ensemble_order(x[0], (0, 8), 0.8),
                lambda: hip.ensemble_order(x, (6, 11), 0.8), lambda: hip.ensemble_order(x, (-1, 4), 0.8),
                lambda: hip.ensemble_order(x, (0, 0), 0.8), lambda: hip.ensemble_order(x, 5, 0.8),
                lambda: hip.ensemble_order(x, (6, 10), 0.8, truth.double()),
                lambda: hip.ensemble_order(x, (6, 10), 0.8, torch.zeros(B, rows, 9)),
                lambda: hip.ensemble_order(x, (6, 10), 0.8, torch.zeros(B, 10, rows).transpose(1, 2)),
                lambda: hip.ensemble_order(x.to(torch.float16), (6, 10), 0.8)):
        with pytest.raises(hip.HipError):
            bad()
    with pytest.raises(hip.HipError, match="at most 64"):
        hip.ensemble_order(torch.zeros(1, 65, 2, 4), (0, 4), 0.8)
    for L in (0.0, 1.0):
        with pytest.raises(ValueError):
            hip.ensemble_order(x, (6, 10), L)
    assert len(lib.calls) == 2, "a refused call does not reach the library"


def _labels(n, frames):
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import LOSS_KEY_ORDER, LOSS_KEY_WIDTHS
    g = torch.Generator().manual_seed(3)
    return {k: torch.randn(n, frames, w, generator=g) for k, w in zip(LOSS_KEY_ORDER, LOSS_KEY_WIDTHS)}


def test_predictor_paths(dry):
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import LOSS_KEY_ORDER, LOSS_KEY_WIDTHS
    from inferbiomechanics_amd.models.DiffusionLabelPredictor import DiffusionLabelPredictor
    r = sampler_trace.Run()
    lib = dry.lib()
    m = r.model(torch.bfloat16, **sampler_trace.LABELS)
    D = sampler_trace.LABELS["D"]
    with pytest.raises(ValueError, match="num_samples >= 2"):
        DiffusionLabelPredictor(m, S, eta=1.0, num_samples=1, interval=0.5)
    for L in (0.0, 1.0, -1, 2):
        with pytest.raises(ValueError):
            DiffusionLabelPredictor(m, S, eta=1.0, num_samples=3, interval=L)

    def run(interval, path, labels):
        pred = DiffusionLabelPredictor(m, S, seed=11, use_graph=False, eta=1.0, num_samples=3, interval=interval)
        lib.calls.clear()
        lib.args.clear()
        if path == "call":
            out = pred(sampler_trace._label_inputs(r, 2, 10), _labels(2, 10) if labels else None, draw=1)
        else:
            out = pred.predict_trial_ensemble(sampler_trace._label_inputs(r, 2, 20), hop=4, draw=1,
                                              labels=_labels(2, 20) if labels else None)
        return pred, out, list(lib.calls), list(lib.args)

    for path, frames in (("call", 10), ("trial", 20)):
        off, _, plain, _ = run(None, path, True)
        assert NAME not in plain and plain.count("ib_ensemble_stats") == 1
        assert off.last_interval is None and off.last_crps is None and off.last_rank is None and off.last_inside is None
        for labels in (True, False):
            pred, out, names, args = run(0.5, path, labels)
            at = names.index("ib_ensemble_stats")
            assert names.count(NAME) == 1 and names[at + 1] == NAME and names[:at + 1] + names[at + 2:] == plain, \
                "one launch, right after the statistics; everything else is the call without the interval"
            a = dict(args)[NAME]
            assert a[8:14] == (2, 3, frames, D, D - 30, 30) and a[14:20] == (0, 0.0, 1, 0.0, 2, 0.0) and a[20] == dry.BF16
            assert a[0] == dict(args)["ib_ensemble_stats"][0], "the members the statistics were taken of"
            assert (a[1] is None) == (not labels) and all((v is None) == (not labels) for v in a[5:8])
            shapes = [(2, frames, w) for w in LOSS_KEY_WIDTHS]
            assert sorted(pred.last_interval) == ["hi", "lo", "median"]
            for part in pred.last_interval.values():
                assert [tuple(part[k].shape) for k in LOSS_KEY_ORDER] == shapes
                assert all(part[k].dtype == torch.float32 for k in LOSS_KEY_ORDER)
            if labels:
                for d, dt in ((pred.last_crps, torch.float32), (pred.last_rank, torch.uint8), (pred.last_inside, torch.uint8)):
                    assert [tuple(d[k].shape) for k in LOSS_KEY_ORDER] == shapes and all(d[k].dtype == dt for k in LOSS_KEY_ORDER)
            else:
                assert pred.last_crps is None and pred.last_rank is None and pred.last_inside is None
            assert [tuple(out[k].shape) for k in LOSS_KEY_ORDER] == shapes and pred.last_std is not None
    # a scored call followed by an unscored one does not keep the old score
    pred = DiffusionLabelPredictor(m, S, seed=11, use_graph=False, eta=1.0, num_samples=3, interval=0.5)
    pred(sampler_trace._label_inputs(r, 2, 10), _labels(2, 10))
    assert pred.last_crps is not None
    pred(sampler_trace._label_inputs(r, 2, 10))
    assert pred.last_crps is None and pred.last_interval is not None


def test_command_line_flag_and_refusals():
    from inferbiomechanics_amd.cli._common import checked_interval
    from inferbiomechanics_amd.cli.analyze import AnalyzeCommand
    from inferbiomechanics_amd.cli.visualize import VisualizeCommand
    for cmd, word in ((AnalyzeCommand(), "analyze"), (VisualizeCommand(), "visualize")):
        parser = argparse.ArgumentParser()
        cmd.register_subcommand(parser.add_subparsers(dest="command"))
        a = parser.parse_args([word])
        assert a.interval is None and checked_interval(a, 1) is None and checked_interval(a, 8) is None
        a = parser.parse_args([word, "--interval", "0.8"])
        assert checked_interval(a, 2) == 0.8 and checked_interval(a, 8) == 0.8
        for K in (1, 0):
            with pytest.raises(SystemExit, match="--num-samples >= 2"):
                checked_interval(a, K)
        for bad in ("0", "1", "-0.5", "1.5"):
            with pytest.raises(SystemExit, match="--interval"):
                checked_interval(parser.parse_args([word, "--interval", bad]), 8)


def test_analyze_reaches_the_order_statistics(dry, tmp_path, capsys):
    from inferbiomechanics_amd.main import main
    ck = str(tmp_path / "ck")
    base = ['--no-wandb', '--checkpoint-dir', ck, '--data-loading-workers', '0', '--model-type', 'diffusion-mlp',
            '--hidden-dims', '32', '32', '--synthetic-windows', '2']
    assert main(['train', '--feat-dim', '177', '--epochs', '1', '--max-steps', '1', '--batch-size', '4'] + base[:-2]
                + ['--synthetic-windows', '8'])
    lib = dry.lib()
    lib.calls.clear()
    capsys.readouterr()
    assert main(['analyze', '--sample-steps', '5', '--sample-eta', '1', '--num-samples', '3', '--interval', '0.5'] + base)
    assert lib.calls.count(NAME) == 2 * 2 == lib.calls.count("ib_ensemble_stats"), "two splits, two windows each"
    out = capsys.readouterr().out
    assert out.count("Ensemble calibration (") == 2 and out.count("Rank histogram (") == 2
    assert "3 samples per window, level 0.5): cop: coverage " in out and "(calibrated ensemble: 0.5000)" in out
    lib.calls.clear()
    assert main(['analyze', '--sample-steps', '5', '--sample-eta', '1', '--num-samples', '3'] + base)
    assert NAME not in lib.calls and "Ensemble calibration" not in capsys.readouterr().out
    with pytest.raises(SystemExit, match="--num-samples >= 2"):
        main(['analyze', '--sample-steps', '5', '--interval', '0.5'] + base)
    with pytest.raises(SystemExit, match="--interval"):
        main(['analyze', '--sample-steps', '5', '--num-samples', '3', '--interval', '1.0'] + base)


def test_visualize_prints_the_interval_width_next_to_the_std(dry, tmp_path, capsys):
    from inferbiomechanics_amd.main import main
    tr = ["visualize", "--synthetic-windows", "60", "--checkpoint-dir", str(tmp_path / "ck"), "--sample-steps", "4",
          "--model-type", "diffusion-transformer", "--trial-frames", "25", "--trial-hop", "4", "--num-frames", "1",
          "--sample-eta", "1", "--num-samples", "3"]
    fig = r"(?:-?\d+\.\d+|nan|inf|-inf)"           # a dry run computes nothing: only the layout of the figures is checked
    std = rf"^trial 0 +{{}}: mean std over 3 samples stitched {fig}, per-window {fig}"
    lib = dry.lib()
    capsys.readouterr()
    assert main(tr)
    plain = [l for l in capsys.readouterr().out.splitlines() if "mean std over" in l]
    assert len(plain) == 4 and all(re.match(std.format(n) + "$", l) for n, l in zip(("cop", "force", "torque", "wrench"), plain))
    assert NAME not in lib.calls
    lib.calls.clear()
    assert main(tr + ["--interval", "0.5"])
    lines = [l for l in capsys.readouterr().out.splitlines() if "mean std over" in l]
    assert len(lines) == 4
    for n, l in zip(("cop", "force", "torque", "wrench"), lines):
        assert re.match(std.format(n) + rf"; mean width of the 0\.5 interval stitched {fig}, per-window {fig}$", l), l
    assert lib.calls.count(NAME) == 2 == lib.calls.count("ib_ensemble_stats"), "the stitched trial and its disjoint windows"
    with pytest.raises(SystemExit, match="--num-samples >= 2"):
        main(tr[:-2] + ["--interval", "0.5"])


# ---------------------------------------------------------------------------------------------------------------------
# 6. the kernels' registers
# ---------------------------------------------------------------------------------------------------------------------
def test_kernel_resources_no_scratch_no_spill():
    from tools import kernel_resources as kr
    if kr.hipcc() is None:
        pytest.skip("hipcc not installed")
    rows = kr.resources("ensemble.hip")
    forms = sorted(re.search(r"ensemble_order_kernelI(f|DF16b)Li(\d+)E", r["mangled"]).groups() for r in rows)
    assert forms == sorted((ty, str(kp)) for ty in ("f", "DF16b") for kp in (1, 2, 4, 8, 16, 32, 64)), \
        "fp32 / bf16 x every padded size"
    for r in rows:
        print(f"{r['kernel']}: {r['vgpr']} VGPRs, {r['occupancy']} waves per SIMD")
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["lds"] == 0, r
