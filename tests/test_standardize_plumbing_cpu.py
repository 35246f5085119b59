"""Host side of the per-column standardisation without a GPU: the ninth header and the build lists, the argument checks of
the three entries, the binding's marshalling for both geometries, inv_scale against the header's rule, the checkpoint round
trip of column_stats, the command line's refusals, a dry-run `train --standardize` from start to resume, and the launch
sequence of a predictor whose denoiser carries statistics (one ib_column_affine before the sampler's launches, one after)."""
import argparse
import glob
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import standardize_restatement as SR

BF = torch.bfloat16
NAMES = ["ib_column_affine", "ib_column_moments_accum", "ib_column_moments_finalize"]


@pytest.fixture()
def dry():
    from inferbiomechanics_amd import hip
    hip.set_dry_run(True)
    yield hip
    hip.set_dry_run(False)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the header, the build lists, the argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_ninth_header_has_its_own_table_and_is_built():
    from inferbiomechanics_amd import hip
    assert os.path.basename(hip.STANDARDIZE_HEADER_PATH) == "ib_hip_standardize.h" and os.path.exists(hip.STANDARDIZE_HEADER_PATH)
    assert hip.standardize_decls() == NAMES == sorted(hip._STANDARDIZE_SIGS)
    assert len(hip._TABLES) == 6 and len(hip._HEADERS) == 8, "the tables other tests pin are as they were"
    assert all(t is not hip._STANDARDIZE_SIGS for t in hip._HEADERS)
    text = open(hip.STANDARDIZE_HEADER_PATH).read()
    for n in NAMES:
        assert len(re.findall(rf"\bint {n}\(", text)) == 1
        assert all(n not in t for t in hip._HEADERS), "no name collides with another header's"
        res, args = hip._sig(n)
        assert res is hip._c.c_int and args[-1] is hip._vp and hip._is_launch(n)
    i64, vp, ci = hip._i64, hip._vp, hip._c.c_int
    assert hip._sig("ib_column_moments_accum")[1] == [vp] + [i64] * 4 + [vp, vp, i64, ci, vp]
    assert hip._sig("ib_column_moments_finalize")[1] == [vp] + [i64] * 3 + [vp, hip._f32] + [vp] * 4
    assert hip._sig("ib_column_affine")[1] == [vp, ci, i64, i64, vp, ci, i64, i64, vp, vp] + [i64] * 4 + [ci, vp]
    assert len(hip._ALL_SIGS) == sum(len(t) for t in hip._HEADERS) + 3
    mk = open(os.path.join(os.path.dirname(hip.__file__), "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, flags=re.M).group(1).split()
    hdrs = re.search(r"^HDRS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "standardize.hip" in srcs and "../../include/ib_hip_standardize.h" in hdrs
    assert "$(SRCS:%.hip=build/%.o)" in mk and "$(SRCS:%.hip=build_ab/%.o)" in mk, "one list serves both builds"
    for path in (hip.LIB_PATH, hip.AB_LIB_PATH):
        if not os.path.exists(path):
            pytest.fail(f"{path} is not built")
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        assert set(NAMES) <= {line.split()[-1] for line in out.splitlines() if line.strip()}, path


def test_argument_errors_come_before_any_launch():
    """IB_E_ARG = -1, IB_E_DTYPE = -2; the pointers are never dereferenced on the host, any non-null value stands for one"""
    from inferbiomechanics_amd import hip
    lib = hip.lib()
    P = lambda on=True: 4096 if on else None
    acc = lambda nulls=(), n=4, T=3, D=6, pitch=24, G=8, dtype=1: lib.ib_column_moments_accum(
        P(0 not in nulls), n, T, D, pitch, P(1 not in nulls), P(2 not in nulls), G, dtype, None)
    for i in range(3):
        assert acc(nulls=(i,)) == -1, i
    assert acc(pitch=17) == -1, "pitch < T D"
    assert acc(G=0) == -1 and acc(G=-3) == -1 and acc(n=0) == -1 and acc(T=0) == -1 and acc(D=0) == -1
    assert acc(dtype=7) == -2
    fin = lambda nulls=(), G=8, D=6, count=12, min_std=1e-6: lib.ib_column_moments_finalize(
        P(0 not in nulls), G, D, count, P(1 not in nulls), min_std, P(2 not in nulls), P(3 not in nulls), P(4 not in nulls), None)
    for i in range(5):
        assert fin(nulls=(i,)) == -1, i
    assert fin(count=0) == -1 and fin(count=-1) == -1 and fin(G=0) == -1 and fin(D=0) == -1 and fin(min_std=-1.0) == -1

    def aff(nulls=(), sdt=1, ddt=0, swin=48, srow=8, dwin=48, drow=8, N=2, T=6, c0=0, w=8, mode=0, same=False):
        src = P(0 not in nulls)
        return lib.ib_column_affine(src, sdt, swin, srow, src if same else (8192 if 1 not in nulls else None), ddt, dwin, drow,
                                    P(2 not in nulls), P(3 not in nulls), N, T, c0, w, mode, None)
    for i in range(4):
        assert aff(nulls=(i,)) == -1, i                                 # a = NULL is an error in mode 0 only
    assert aff(w=0) == -1 and aff(w=-8) == -1 and aff(c0=-1) == -1 and aff(N=0) == -1 and aff(T=0) == -1
    assert aff(mode=2) == -1 and aff(mode=-1) == -1
    assert aff(c0=4, w=8) == -1 and aff(swin=40) == -1 and aff(dwin=47) == -1, "a window does not fit its row or its pitch"
    assert aff(same=True) == -1 and aff(same=True, ddt=1, drow=16, dwin=96) == -1, "in place: equal dtype and strides"
    assert aff(sdt=5) == -2 and aff(ddt=9) == -2


# ---------------------------------------------------------------------------------------------------------------------
# 2. the binding
# ---------------------------------------------------------------------------------------------------------------------
def test_wrappers_marshal_both_geometries(dry):
    hip, lib = dry, dry.lib()
    table = torch.zeros(4, 24, dtype=BF)
    shift = torch.zeros(6)
    acc = hip.column_moments_acc(6, "cpu", 16)
    assert tuple(acc.shape) == (16, 6, 2) and acc.dtype == torch.float64 and not acc.any()
    assert hip.column_moments(table, 3, 6, shift, acc) is acc
    assert lib.args[-1] == ("ib_column_moments_accum", (table.data_ptr(), 4, 3, 6, 24, shift.data_ptr(), acc.data_ptr(), 16,
                                                        hip.BF16, 0))
    hip.column_moments(table[1:3], 3, 6, shift, acc)                    # a chunk: rows of the same table
    assert lib.args[-1][1][:5] == (table[1:3].data_ptr(), 2, 3, 6, 24)
    mean, scale, inv = hip.column_moments_finalize(acc, 12, shift, min_std=1e-3)
    name, a = lib.args[-1]
    assert name == "ib_column_moments_finalize" and a[:5] == (acc.data_ptr(), 16, 6, 12, shift.data_ptr())
    assert a[5] == 1e-3 and a[6:] == (mean.data_ptr(), scale.data_ptr(), inv.data_ptr(), 0)
    assert all(t.dtype == torch.float32 and tuple(t.shape) == (6,) for t in (mean, scale, inv))
    # a cache table: win = pitch, row = D; fp32 source rows [n, T D] into a pitched bf16 table
    src = torch.zeros(4, 18)
    hip.column_affine(src, table, mean, inv, mode=hip.STANDARDIZE, window=3)
    assert lib.args[-1] == ("ib_column_affine", (src.data_ptr(), hip.F32, 18, 6, table.data_ptr(), hip.BF16, 24, 6,
                                                 mean.data_ptr(), inv.data_ptr(), 4, 3, 0, 6, 0, 0))
    hip.column_affine(table, table, mean, inv, window=3)                # in place; mode 0 is the default
    assert lib.args[-1][1][:8] == (table.data_ptr(), hip.BF16, 24, 6, table.data_ptr(), hip.BF16, 24, 6)
    # a sampler state [B, T, ld]: win = T ld, row = ld; a column window; de-standardising without a mean
    x, out = torch.zeros(2, 5, 8, dtype=BF), torch.zeros(2, 5, 6)
    hip.column_affine(x, out, None, scale, cols=(2, 3), mode=hip.DESTANDARDIZE)
    assert lib.args[-1] == ("ib_column_affine", (x.data_ptr(), hip.BF16, 40, 8, out.data_ptr(), hip.F32, 30, 6, None,
                                                 scale.data_ptr(), 2, 5, 2, 3, 1, 0))
    n = len(lib.calls)
    for bad in (lambda: hip.column_moments(table, 5, 6, shift, acc), lambda: hip.column_moments(table, 3, 6, shift[:5], acc),
                lambda: hip.column_moments(table, 3, 6, shift, acc.float()), lambda: hip.column_moments(table, 3, 6, shift, acc[:, :5]),
                lambda: hip.column_moments(table[:, :20], 3, 6, shift, acc),
                lambda: hip.column_moments_finalize(acc, 0, shift), lambda: hip.column_moments_finalize(acc, 5, shift, -1.0),
                lambda: hip.column_moments_finalize(acc, 5, shift[:3]),
                lambda: hip.column_affine(src, table, mean, inv), lambda: hip.column_affine(src, table, None, inv, window=3),
                lambda: hip.column_affine(src, table, mean, inv, window=4), lambda: hip.column_affine(src, table, mean, inv[:5], window=3),
                lambda: hip.column_affine(src[:3], table, mean, inv, window=3), lambda: hip.column_affine(x, out, mean, inv, cols=(4, 3)),
                lambda: hip.column_affine(x, out, mean, inv, cols=(0, 0)), lambda: hip.column_affine(x, out, mean, inv, mode=2),
                lambda: hip.column_affine(x, x.view(2, 40), mean, inv, window=5), lambda: hip.column_affine(x, out[:, :4], mean, inv),
                lambda: hip.column_affine(x, torch.zeros(2, 5, 4), mean, inv)):
        with pytest.raises(hip.HipError):
            bad()
    assert len(lib.calls) == n, "a refused call launches nothing"


def test_inv_scale_is_the_headers_rule():
    from inferbiomechanics_amd import hip
    g = torch.Generator().manual_seed(1)
    scale = torch.cat([10.0 ** (torch.rand(4000, generator=g) * 12 - 6), torch.tensor([1.0, 3.0, 1e-6, 0.1, 1024.0])])
    inv = hip.inv_scale(scale)
    assert inv.dtype == torch.float32 and inv.device == scale.device
    assert np.array_equal(SR.bits(inv.numpy()), SR.bits(SR.inv_rule(scale.numpy())))
    exact = [(1.0 / np.float64(np.float32(s))).astype(np.float32) for s in (3.0, 0.1)]
    assert inv[-4].item() == exact[0] and inv[-2].item() == exact[1] and inv[-1].item() == 1.0 / 1024
    s, i = SR.finalize_rule(np.array([0.0, 5e-7, 2e-6, 3.0], np.float32), 1e-6)
    assert s.tolist() == [1.0, 1.0, np.float32(2e-6), 3.0] and i[0] == 1.0 and i[3] == np.float32(1.0 / 3.0)
    with pytest.raises(hip.HipError):
        hip.inv_scale(scale.double())


def test_restatement_rounds_as_torch_does():
    g = torch.Generator().manual_seed(2)
    v = torch.cat([torch.randn(5000, generator=g) * 100, torch.tensor([1.00390625, 1.01171875, -1.00390625, 0.0, 3.0e38])])
    assert np.array_equal(SR.bits(SR.bf16_round(v.numpy())), SR.bits(v.to(BF).float().numpy())), "ties go to even"
    x, a, b = (torch.randn(64, 7, generator=g).numpy() for _ in range(3))
    assert np.array_equal(SR.affine(x, a[0], b[0], 0), ((x - a[0]).astype(np.float32) * b[0]).astype(np.float32))
    fused = SR.affine(x, a[0], b[0], 1)
    exact = x.astype(np.float64) * b[0].astype(np.float64) + a[0].astype(np.float64)     # the fma, up to one float64 rounding
    assert np.abs(fused - exact).max() <= 0.5001 * np.abs(SR.ulp32(exact)).max() and np.array_equal(SR.affine(x, None, b[0], 1), x * b[0])
    mean, sd = SR.moments_ref(np.array([[1.0, 5.0], [3.0, 5.0]]))
    assert mean.tolist() == [2.0, 5.0] and sd.tolist() == [1.0, 0.0]


# ---------------------------------------------------------------------------------------------------------------------
# 3. the checkpoint and the command line
# ---------------------------------------------------------------------------------------------------------------------
def test_checkpoint_carries_column_stats_only_when_set(tmp_path):
    from inferbiomechanics_amd.cli.abstract_command import AbstractCommand
    from inferbiomechanics_amd.cli.train import save_checkpoint
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionMLP, DiffusionTransformer

    class Opt:
        def state_dict(self):
            return {}

    model = DiffusionMLP(30, [32], temb_dim=16, temb_hidden=24)
    assert model.column_stats is None and DiffusionTransformer(40, 8, d_model=64, num_heads=4, dim_feedforward=64,
                                                              num_layers=1).column_stats is None
    plain = torch.load(save_checkpoint(str(tmp_path / "a"), 0, 1, model, Opt()), map_location="cpu")
    assert "column_stats" not in plain
    stats = torch.stack([torch.arange(30, dtype=torch.float32) - 7.0, torch.arange(1, 31, dtype=torch.float32) / 8], dim=1)
    model.column_stats = stats.double()                                # whatever it is held as, the file holds fp32
    ckpt = torch.load(save_checkpoint(str(tmp_path / "b"), 0, 1, model, Opt()), map_location="cpu")
    assert torch.equal(ckpt["column_stats"], stats) and ckpt["column_stats"].dtype == torch.float32
    assert tuple(ckpt["column_stats"].shape) == (30, 2) and "column_range" not in ckpt
    fresh = DiffusionMLP(30, [32], temb_dim=16, temb_hidden=24)
    AbstractCommand().load_latest_checkpoint(fresh, checkpoint_dir=str(tmp_path / "b"))
    assert torch.equal(fresh.column_stats, stats) and fresh.column_stats.dtype == torch.float32
    again = torch.load(save_checkpoint(str(tmp_path / "c"), 1, 1, fresh, Opt()), map_location="cpu")
    assert torch.equal(again["column_stats"], stats)
    AbstractCommand().load_latest_checkpoint(fresh, checkpoint_dir=str(tmp_path / "a"))
    assert fresh.column_stats is None, "an older checkpoint loads as before: no statistics"


def parser():
    from inferbiomechanics_amd.cli.train import TrainCommand
    p = argparse.ArgumentParser()
    TrainCommand().register_subcommand(p.add_subparsers(dest="command"))
    return p


def test_cli_flag_and_refusals():
    from inferbiomechanics_amd.cli.train import check_standardize
    train = lambda *a: parser().parse_args(["train"] + list(a))
    assert train().standardize is False
    check_standardize(train())
    check_standardize(train(), have_stats=False)
    ok = train("--model-type", "diffusion-mlp", "--standardize", "--window-cache", "hbm")
    check_standardize(ok)
    check_standardize(ok, have_stats=False)
    with pytest.raises(SystemExit, match="--standardize"):
        check_standardize(train("--standardize", "--window-cache", "hbm"))          # a regression model type
    for new_run in (("--model-type", "diffusion-mlp", "--standardize"),
                    ("--model-type", "diffusion-transformer", "--standardize", "--window-cache", "hbm", "--eager")):
        check_standardize(train(*new_run))                              # the model type is fine ...
        with pytest.raises(SystemExit, match="--window-cache"):
            check_standardize(train(*new_run), have_stats=False)        # ... but there is nothing to take the statistics from
        check_standardize(train(*new_run), have_stats=True)             # a resumed run has them: --eager is fine
    sub = [a for a in parser()._subparsers._group_actions[0].choices["train"]._actions if "--standardize" in a.option_strings][0]
    assert "--record-range" in sub.help and "sampler" in sub.help


BASE = ['--no-wandb', '--synthetic-windows', '24', '--batch-size', '8', '--data-loading-workers', '0', '--model-type',
        'diffusion-mlp', '--feat-dim', '24', '--hidden-dims', '32', '32', '--stride', '1', '--history-len', '6',
        '--compute-dtype', 'bf16', '--seed', '7']


def latest(tmp_path, d):
    return torch.load(sorted(glob.glob(str(tmp_path / d / "diffusion-mlp" / "*.pt")), key=os.path.getmtime)[-1], map_location="cpu")


def test_train_standardize_end_to_end_in_dry_run(dry, tmp_path):
    """a new run: two passes over the cache's source (moments, then the affine into the table), the key in the checkpoint;
    a resumed run: pass 2 alone with the checkpoint's statistics; the dev loop's windows go through the affine; the two
    mismatched resumes are refused; without the flag neither a launch nor the key"""
    from inferbiomechanics_amd.main import main
    lib = dry.lib()
    cache = ['--window-cache', str(tmp_path / "motion.npy")]
    assert main(['train', '--epochs', '1', '--checkpoint-dir', str(tmp_path / "plain")] + BASE + cache)
    assert not any(n in lib.calls for n in NAMES) and "column_stats" not in latest(tmp_path, "plain")
    lib.calls.clear()
    assert main(['train', '--epochs', '1', '--standardize', '--checkpoint-dir', str(tmp_path / "std")] + BASE + cache)
    assert lib.calls.count("ib_column_moments_accum") == 1 and lib.calls.count("ib_column_moments_finalize") == 1
    build = [n for n in lib.calls if n in NAMES][:3]
    assert build == ["ib_column_moments_accum", "ib_column_moments_finalize", "ib_column_affine"], "pass 1, finalize, pass 2"
    dev_windows = lib.calls.count("ib_column_affine") - 1
    assert dev_windows >= 1, "every dev batch is standardised on the device"
    first = latest(tmp_path, "std")["column_stats"]
    assert tuple(first.shape) == (24, 2) and first.dtype == torch.float32
    lib.calls.clear()
    assert main(['train', '--epochs', '2', '--standardize', '--checkpoint-dir', str(tmp_path / "std")] + BASE + cache)
    assert "ib_column_moments_accum" not in lib.calls and "ib_column_moments_finalize" not in lib.calls, "the checkpoint's statistics"
    assert lib.calls.count("ib_column_affine") == 1 + dev_windows
    assert torch.equal(latest(tmp_path, "std")["column_stats"].view(torch.int32), first.view(torch.int32))
    with pytest.raises(SystemExit, match="--standardize"):
        main(['train', '--epochs', '3', '--checkpoint-dir', str(tmp_path / "std")] + BASE + cache)
    with pytest.raises(SystemExit, match="--standardize"):
        main(['train', '--epochs', '3', '--standardize', '--checkpoint-dir', str(tmp_path / "plain")] + BASE + cache)
    with pytest.raises(SystemExit, match="--window-cache"):
        main(['train', '--epochs', '1', '--standardize', '--checkpoint-dir', str(tmp_path / "none")] + BASE)
    # with --record-range the range is taken after the table was standardised
    lib.calls.clear()
    del lib.args[:]
    assert main(['train', '--epochs', '1', '--standardize', '--record-range', '--checkpoint-dir', str(tmp_path / "both")]
                + BASE + ['--window-cache', 'hbm'])
    names = [n for n in lib.calls if n in NAMES + ["ib_column_range"]]
    assert names[:4] == ["ib_column_moments_accum", "ib_column_moments_finalize", "ib_column_affine", "ib_column_range"]
    table_pass = [a for n, a in lib.args if n == "ib_column_affine"][0]
    assert table_pass[0] == table_pass[4] and table_pass[1] == table_pass[5] == dry.BF16, "the synthetic table, in place"
    both = latest(tmp_path, "both")
    assert "column_stats" in both and "column_range" in both
    # a resumed run may be eager: its windows go through the affine, nothing is accumulated
    lib.calls.clear()
    assert main(['train', '--epochs', '3', '--standardize', '--eager', '--max-steps', '2', '--checkpoint-dir', str(tmp_path / "std")] + BASE)
    assert "ib_column_moments_accum" not in lib.calls and lib.calls.count("ib_column_affine") >= 2


# ---------------------------------------------------------------------------------------------------------------------
# 4. the predictor
# ---------------------------------------------------------------------------------------------------------------------
def windows(n):
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import SyntheticWindowDataset
    ds = SyntheticWindowDataset(n, 50, 5)
    items = [ds[i] for i in range(n)]
    return ({k: torch.stack([it[0][k] for it in items]) for k in items[0][0]},
            {k: torch.stack([it[1][k] for it in items]) for k in items[0][1]})


def test_predictor_brackets_the_sampler_with_one_affine_each_side(dry):
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionMLP
    from inferbiomechanics_amd.models.DiffusionLabelPredictor import DiffusionLabelPredictor
    inputs, labels = windows(3)
    model = DiffusionMLP(177, [32, 32], temb_dim=16, temb_hidden=24, compute_dtype=BF)
    lib = dry.lib()
    stats = torch.stack([torch.linspace(-2, 2, 177), torch.linspace(0.5, 3, 177)], dim=1)
    for kw in (dict(), dict(eta=1.0, num_samples=3, interval=0.8)):
        pred = DiffusionLabelPredictor(model, 5, seed=3, **kw)
        model.column_stats = None
        lib.calls.clear()
        pred(inputs, labels)
        off = list(lib.calls)
        assert "ib_column_affine" not in off, "no statistics, nothing launched"
        model.column_stats = stats                                     # read per call: the same predictor
        lib.calls.clear()
        del lib.args[:]
        out = pred(inputs, labels)
        on = list(lib.calls)
        assert [n for n in on if n != "ib_column_affine"] == off, "nothing else changes"
        where = [i for i, n in enumerate(on) if n == "ib_column_affine"]
        K = kw.get("num_samples", 1)
        tail = 0 if K == 1 else 2                                      # ib_ensemble_stats and ib_ensemble_order follow
        assert where == [0, len(on) - 1 - tail], "one before the sampler's first launch, one after its last"
        a_in, a_out = [a for n, a in lib.args if n == "ib_column_affine"]
        assert a_in[1] == a_in[5] == dry.F32 and a_in[2:4] == a_in[6:8] == (10 * 177, 177) and a_in[10:] == (3, 10, 0, 177, 0, 0)
        assert a_out[1] == dry.BF16 and a_out[5] == dry.F32 and a_out[6:8] == (10 * 177, 177), "de-standardised into fp32"
        assert a_out[10:] == (3 * K, 10, 0, 177, 1, 0) and a_out[8] == a_in[8] and a_out[9] != a_in[9], "mean; scale, not inv"
        assert all(v.dtype == torch.float32 for v in out.values())
        if K > 1:
            stat_call = [a for n, a in lib.args if n == "ib_ensemble_stats"][0]
            order_call = [a for n, a in lib.args if n == "ib_ensemble_order"][0]
            assert stat_call[0] == order_call[0] == a_out[4] and stat_call[-2] == dry.F32, "they read the raw-unit tensor"
    model.column_stats = torch.zeros(5, 2)
    with pytest.raises(ValueError, match="column_stats"):
        DiffusionLabelPredictor(model, 5)(inputs)
