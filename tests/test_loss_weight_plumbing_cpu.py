"""Host side of the loss weighting by noise level without a GPU: LossWeight.weights against the closed form, the band rule at
every edge, the refusals, the fourteenth header and the build, the binding's table, the trainer's loss seam in dry-run traces
(off: the launches as ever, name for name; on: exactly the weighted pair), the state-dict round trip, the command line, and
the new kernels' registers."""
import argparse
import os
import re
import subprocess

import numpy as np
import pytest
import torch

NAMES = ["ib_loss_level_buckets", "ib_mse_loss_weighted_finalize", "ib_mse_loss_weighted_partial", "ib_mse_loss_weighted_workspace"]
NB = 8
PLAIN_SEAM = {"ib_mse_loss_partial", "ib_mse_loss_finalize", "ib_mse_loss_partial_cond", "ib_mse_loss_finalize_cond"}
WEIGHTED_SEAM = {"ib_mse_loss_weighted_partial", "ib_mse_loss_weighted_finalize"}


@pytest.fixture()
def dry():
    from inferbiomechanics_amd import hip
    hip.set_dry_run(True)
    yield hip
    hip.set_dry_run(False)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the weights
# ---------------------------------------------------------------------------------------------------------------------
def test_weights_match_the_closed_form():
    from inferbiomechanics_amd.diffusion.schedule import alphas_cumprod
    from inferbiomechanics_amd.loss_weight import LossWeight
    ab = alphas_cumprod(1000).numpy()
    assert ab.dtype == np.float64
    snr = ab / (1.0 - ab)
    assert snr[0] > 9e3 and snr[-1] < 5e-5, "the linear schedule: SNR from about 1e4 to about 4e-5"
    for gamma in (1.0, 5.0, 20.0):
        lw = LossWeight("min_snr", gamma=gamma)
        w64 = lw.weights64(ab)
        assert w64.dtype == np.float64 and np.array_equal(w64, np.minimum(1.0, gamma / snr))
        # the paper's form for eps-prediction, min(snr, gamma) / snr: the same number up to one rounding of the division
        np.testing.assert_allclose(w64, np.minimum(snr, gamma) / snr, rtol=4e-16, atol=0)
        assert np.all(w64[snr <= gamma] == 1.0) and np.all(w64[snr > gamma] < 1.0)
        assert np.all(np.diff(w64) >= 0), "SNR falls with t: the weights do not increase with SNR"
        order = np.argsort(snr)
        assert np.all(np.diff(w64[order]) <= 0)
        w = lw.weights(ab)
        assert w.dtype == np.float32 and np.array_equal(w, w64.astype(np.float32)), "cast to fp32 once"
        assert np.all(w > 0)
    # gamma = 5 on the product's schedule: hand-checked ends
    w = LossWeight("min_snr").weights64(ab)
    assert w[0] == 5.0 * (1.0 - ab[0]) / ab[0] or abs(w[0] - 5.0 * (1.0 - ab[0]) / ab[0]) <= 1e-18
    assert abs(w[0] - 5.0 * 1e-4 / (1.0 - 1e-4)) <= 1e-15 and w[-1] == 1.0
    assert np.array_equal(LossWeight("uniform").weights(ab), np.ones(1000, dtype=np.float32))
    tab = np.linspace(0.0, 2.0, 1000)
    assert np.array_equal(LossWeight("table", table=tab).weights(ab), tab.astype(np.float32))
    assert np.array_equal(LossWeight("table", table=torch.from_numpy(tab)).weights(torch.from_numpy(ab)), tab.astype(np.float32))


def test_level_band_at_every_edge():
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.loss_weight import LEVEL_BUCKETS, band_edges, level_band
    assert LEVEL_BUCKETS == NB == hip.LOSS_LEVEL_BUCKETS
    text = open(hip.LOSSWEIGHT_HEADER_PATH).read()
    assert re.search(r"^#define IB_LOSS_LEVEL_BUCKETS 8$", text, flags=re.M)
    if os.path.exists(hip.LIB_PATH):
        assert hip.loss_level_buckets() == NB
    for n in (7, 50, 1000):
        all_t = np.arange(n)
        k = level_band(all_t, n)
        assert np.array_equal(k, [t * NB // n for t in range(n)]) and k.min() == 0 and k.max() == (n - 1) * NB // n
        assert np.all(np.diff(k) >= 0)
        edges = band_edges(n)
        assert edges[0][0] == 0 and edges[-1][1] == n and all(a[1] == b[0] for a, b in zip(edges, edges[1:]))
        for band, (lo, hi) in enumerate(edges):
            assert np.array_equal(all_t[k == band], np.arange(lo, hi)), (n, band)
            if hi > lo:
                assert level_band(lo, n) == band == level_band(hi - 1, n)
                assert lo == 0 or level_band(lo - 1, n) < band
                assert hi == n or level_band(hi, n) > band
        assert level_band(-5, n) == 0 and level_band(n, n) == k[-1] == level_band(1 << 40, n), "the kernel's clamp"
    assert band_edges(1000) == [(125 * k, 125 * (k + 1)) for k in range(NB)]
    assert band_edges(50) == [(0, 7), (7, 13), (13, 19), (19, 25), (25, 32), (32, 38), (38, 44), (44, 50)]
    assert [hi - lo for lo, hi in band_edges(7)] == [1, 1, 1, 1, 1, 1, 1, 0], "fewer levels than bands: an empty band"
    with pytest.raises(ValueError):
        level_band(0, 0)


def test_bad_values_are_refused():
    from inferbiomechanics_amd.engine import HipTrainer
    from inferbiomechanics_amd.loss_weight import LossWeight
    for bad in (0.0, -1.0, float("nan"), float("inf"), "much", None):
        with pytest.raises(ValueError, match="gamma"):
            LossWeight("min_snr", gamma=bad)
    for kind in ("snr", "min-snr", "", None):
        with pytest.raises(ValueError, match="kind"):
            LossWeight(kind)
    with pytest.raises(ValueError, match="table"):
        LossWeight("table")
    with pytest.raises(ValueError, match="table"):
        LossWeight("uniform", table=np.ones(4))
    for bad in (np.ones((2, 2)), np.zeros(0), np.array([1.0, -0.5]), np.array([1.0, np.nan]), np.array([np.inf])):
        with pytest.raises(ValueError, match="table"):
            LossWeight("table", table=bad)
    with pytest.raises(ValueError, match="999 entries, the model 1000"):
        HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, loss_weight=LossWeight("table", table=np.ones(999)))
    with pytest.raises(ValueError, match="999"):
        LossWeight("table", table=np.ones(999)).weights(np.full(1000, 0.5))
    with pytest.raises(ValueError, match="loss_weight"):
        HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, loss_weight="min_snr")
    with pytest.raises(ValueError, match="alpha_bar"):
        LossWeight("min_snr").weights(np.array([1.0, 0.5]))


# ---------------------------------------------------------------------------------------------------------------------
# 2. the header, the build, the binding
# ---------------------------------------------------------------------------------------------------------------------
def test_fourteenth_header_has_its_own_table_and_is_built():
    from inferbiomechanics_amd import hip
    assert os.path.basename(hip.LOSSWEIGHT_HEADER_PATH) == "ib_hip_lossweight.h" and os.path.exists(hip.LOSSWEIGHT_HEADER_PATH)
    assert hip.lossweight_decls() == NAMES == sorted(hip._LOSSWEIGHT_SIGS)
    text = open(hip.LOSSWEIGHT_HEADER_PATH).read()
    for n in NAMES:
        assert len(re.findall(rf"\b(?:int|size_t) {n}\(", text)) == 1
        assert hip._sig(n) == hip._LOSSWEIGHT_SIGS[n]
        for table in (hip._SIGS, hip._STITCH_SIGS, hip._HEAD_SIGS, hip._SDE_SIGS, hip._CFG_SIGS, hip._RESAMPLE_SIGS,
                      hip._ENSEMBLE_SIGS, hip._CLIP_SIGS, hip._STANDARDIZE_SIGS, hip._SCHED_SIGS, hip._DECAY_SIGS,
                      hip._SWEEP_SIGS, hip._GRADNORM_SIGS):
            assert n not in table, "the new table is disjoint from the other thirteen"
        assert n not in hip._EXPORTS
    assert len(hip._SYMBOLS) == len(hip._EXPORTS) + 4 and len(hip._SIGS) == 127
    assert hip._is_launch("ib_mse_loss_weighted_partial") and hip._is_launch("ib_mse_loss_weighted_finalize")
    assert not hip._is_launch("ib_mse_loss_weighted_workspace") and not hip._is_launch("ib_loss_level_buckets")
    c, vp, i64 = hip._c, hip._vp, hip._i64
    assert hip._sig("ib_mse_loss_weighted_partial") == (c.c_int, [vp, i64, vp, vp, i64, vp, vp, c.c_int, i64, vp, hip._sz, i64,
                                                                  i64, i64, c.c_int, vp])
    assert hip._sig("ib_mse_loss_weighted_finalize") == (c.c_int, [vp, hip._sz, vp, i64, c.c_int, vp, vp, i64, i64, vp])
    assert hip._sig("ib_mse_loss_weighted_workspace") == (hip._sz, [i64]) and hip._sig("ib_loss_level_buckets") == (c.c_int, [])
    here = os.path.dirname(hip.__file__)
    mk = open(os.path.join(here, "csrc", "Makefile")).read()
    assert "loss_weight.hip" in re.search(r"^SRCS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert re.search(r"^build/loss_weight\.o build_ab/loss_weight\.o: \.\./\.\./include/ib_hip_lossweight\.h$", mk, flags=re.M)
    assert mk.index("\nall:") < mk.index("ib_hip_lossweight.h"), "the default goal stays `all`"
    src = open(os.path.join(here, "csrc", "loss_weight.hip")).read()
    assert "ib_hip_lossweight.h" in src and "atomic" not in src.lower()
    loss = open(os.path.join(here, "csrc", "loss.hip")).read()
    assert "weighted" not in loss and "lossweight" not in loss, "csrc/loss.hip stays as it was"
    for path in (hip.LIB_PATH, hip.AB_LIB_PATH):
        if not os.path.exists(path):
            pytest.fail(f"{path} is not built")
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        assert set(NAMES) <= {line.split()[-1] for line in out.splitlines() if line.strip()}, path
    root = os.path.dirname(here)
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "ib_hip_lossweight.h" in open(os.path.join(root, doc)).read(), doc
    assert "lossweight_decls" in open(os.path.join(root, "__graft_entry__.py")).read(), "build() checks the header's exports"


def test_workspace_and_host_argument_checks():
    """the checks that run before any launch, on the live library without a GPU: every refused call returns its code"""
    from inferbiomechanics_amd import hip
    lib = hip.lib()
    ws = lib.ib_mse_loss_weighted_workspace
    parts = lambda n: int(lib.ib_mse_loss_workspace(n)) // 4
    for n in (1, 2047, 2048, 2049, 44 * 96, 1024 * 2048, 1024 * 2048 + 1, 1 << 33):
        assert ws(n) == parts(n) * (2 + NB) * 4, n
    assert ws(0) == 0 and ws(-1) == 0 and ws(1024 * 2048 + 1) == 1024 * 40
    assert lib.ib_loss_level_buckets() == NB
    p = 4096                                     # never dereferenced: every call below is refused before a launch
    E_ARG = lib.ib_mse_loss_partial_cond(None, 44, None, None, 44, None, 0, 96, 44, 0, 0, None)
    E_WS = lib.ib_mse_loss_partial_cond(p, 44, p, None, 44, None, 0, 96, 44, 1, 0, None)
    assert E_ARG < 0 and E_WS < 0 and E_ARG != E_WS
    bytes_ = ws(96 * 44)

    def partial(pred=p, target=p, t=p, tab=p, levels=50, rpw=12, wsp=p, wsb=bytes_, rows=96, cols=44, C=0, dtype=0, ldp=44):
        return lib.ib_mse_loss_weighted_partial(pred, ldp, target, None, 0, t, tab, levels, rpw, wsp, wsb, rows, cols, C, dtype,
                                                None)
    assert partial(rpw=7) == E_ARG and partial(rpw=0) == E_ARG and partial(rpw=-12) == E_ARG
    assert partial(levels=0) == E_ARG and partial(levels=-1) == E_ARG
    assert partial(C=44) == E_ARG and partial(C=45) == E_ARG and partial(C=-1) == E_ARG
    assert partial(t=None) == E_ARG and partial(tab=None) == E_ARG and partial(pred=None) == E_ARG and partial(target=None) == E_ARG
    assert partial(rows=0) == E_ARG and partial(cols=0) == E_ARG and partial(ldp=43) == E_ARG
    assert partial(wsp=None) == E_WS and partial(wsb=bytes_ - 1) == E_WS
    assert partial(dtype=5) < 0 and partial(dtype=5) not in (E_ARG, E_WS)

    def final(wsp=p, wsb=bytes_, t=p, nw=8, levels=50, res=p, n_launch=96 * 44, n_mean=96 * 30):
        return lib.ib_mse_loss_weighted_finalize(wsp, wsb, t, nw, levels, res, None, n_launch, n_mean, None)
    assert final(wsp=None) == E_ARG and final(t=None) == E_ARG and final(res=None) == E_ARG
    assert final(nw=0) == E_ARG and final(levels=0) == E_ARG and final(n_launch=0) == E_ARG
    assert final(n_mean=0) == E_ARG and final(n_mean=96 * 44 + 1) == E_ARG
    assert final(wsb=bytes_ - 1) == E_WS


def test_binding_marshals_and_refuses(dry):
    lib = dry.lib()
    rows, D, T, n_levels = 24, 44, 12, 50
    pred_full = torch.zeros(rows, 48)
    pred, target = pred_full[:, :D], torch.zeros(rows, D)
    dfull = torch.zeros(rows, 48)
    t, wtab = torch.zeros(2, dtype=torch.int64), torch.ones(n_levels)
    ws = torch.zeros(dry.mse_loss_weighted_workspace_bytes(rows * D), dtype=torch.uint8)
    res, accum = torch.zeros(64), torch.zeros(2 + 2 * NB, dtype=torch.float64)
    assert ws.numel() == (2 + NB) * 4
    dry.mse_loss_weighted_partial(pred, target, ws, t, wtab, T, cond_cols=14, dpred=dfull[:, :D])
    assert lib.args[-1] == ("ib_mse_loss_weighted_partial",
                            (pred.data_ptr(), 48, target.data_ptr(), dfull.data_ptr(), 48, t.data_ptr(), wtab.data_ptr(), n_levels,
                             T, ws.data_ptr(), ws.numel(), rows, D, 14, 0, 0))
    dry.mse_loss_weighted_partial(pred, target, ws, t, wtab, T)
    assert lib.args[-1][1][3:5] == (None, 0) and lib.args[-1][1][13] == 0
    dry.mse_loss_weighted_finalize(ws, res, t, n_levels, rows * D, rows * 30, accum=accum)
    assert lib.args[-1] == ("ib_mse_loss_weighted_finalize",
                            (ws.data_ptr(), ws.numel(), t.data_ptr(), 2, n_levels, res.data_ptr(), accum.data_ptr(), rows * D,
                             rows * 30, 0))
    dry.mse_loss_weighted_finalize(ws, res, t, n_levels, rows * D, rows * D)
    assert lib.args[-1][1][6] is None
    n = len(lib.calls)
    for bad in (lambda: dry.mse_loss_weighted_partial(pred, target, ws, t, wtab, 7),
                lambda: dry.mse_loss_weighted_partial(pred, target, ws, t, wtab, 0),
                lambda: dry.mse_loss_weighted_partial(pred, target, ws, t, wtab, T, cond_cols=D),
                lambda: dry.mse_loss_weighted_partial(pred, target, ws, t, wtab, T, cond_cols=-1),
                lambda: dry.mse_loss_weighted_partial(pred, target, ws, t[:1], wtab, T),
                lambda: dry.mse_loss_weighted_partial(pred, target, ws, t.int(), wtab, T),
                lambda: dry.mse_loss_weighted_partial(pred, target, ws, t, wtab.double(), T),
                lambda: dry.mse_loss_weighted_partial(pred, target, ws, t, wtab[:0], T),
                lambda: dry.mse_loss_weighted_partial(pred, target, ws, t, wtab[::2], T),
                lambda: dry.mse_loss_weighted_partial(pred, target[:-1], ws, t, wtab, T),
                lambda: dry.mse_loss_weighted_partial(pred, target, ws[:-1], t, wtab, T),
                lambda: dry.mse_loss_weighted_partial(pred, target, ws, t, wtab, T, dpred=torch.zeros(rows, D + 1)),
                lambda: dry.mse_loss_weighted_partial(target.view(-1), target, ws, t, wtab, T),
                lambda: dry.mse_loss_weighted_finalize(ws, res[:17], t, n_levels, rows * D, rows * D),
                lambda: dry.mse_loss_weighted_finalize(ws, res, t, 0, rows * D, rows * D),
                lambda: dry.mse_loss_weighted_finalize(ws, res, t, n_levels, rows * D, rows * D + 1),
                lambda: dry.mse_loss_weighted_finalize(ws, res, t, n_levels, rows * D, 0),
                lambda: dry.mse_loss_weighted_finalize(ws, res, t, n_levels, rows * D, rows * D, accum=accum.float()),
                lambda: dry.mse_loss_weighted_finalize(ws, res, t, n_levels, rows * D, rows * D, accum=accum[:17])):
        with pytest.raises(dry.HipError):
            bad()
    assert len(lib.calls) == n, "a refused call launches nothing"


# ---------------------------------------------------------------------------------------------------------------------
# 3. the trainer
# ---------------------------------------------------------------------------------------------------------------------
def _mlp(dtype=torch.float32):
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionMLP
    torch.manual_seed(0)
    return DiffusionMLP(30, [32, 48], temb_dim=16, temb_hidden=24, compute_dtype=dtype)


def _chain_mlp():
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionMLP
    torch.manual_seed(0)
    return DiffusionMLP(48, [128, 128], temb_dim=32, temb_hidden=128, compute_dtype=torch.bfloat16)


def _transformer():
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    torch.manual_seed(0)
    return DiffusionTransformer(48, 32, d_model=512, num_heads=4, dim_feedforward=1024, num_layers=3, compute_dtype=torch.bfloat16)


def _batch(B=3, T=7, D=30, dt=torch.float32):
    g = torch.Generator().manual_seed(1)
    return (torch.randn(B, T, D, generator=g).to(dt), torch.randint(0, 1000, (B,), generator=g), torch.randn(B, T, D, generator=g).to(dt))


MODELS = {"mlp": (_mlp, lambda: _batch()), "chain_mlp": (_chain_mlp, lambda: _batch(6, 16, 48, torch.bfloat16)),
          "transformer": (_transformer, lambda: _batch(128, 32, 48, torch.bfloat16))}


def _step_calls(hip, tr, batch):
    lib = hip.lib()
    lib.calls.clear()
    del lib.args[:]
    tr.step(batch)
    return list(lib.calls), list(lib.args)


@pytest.mark.parametrize("model", sorted(MODELS))
def test_off_is_the_trainer_without_the_argument(dry, model):
    from inferbiomechanics_amd.engine import HipTrainer
    mk, mb = MODELS[model]
    batch = mb()
    for C in (0, 14):
        want, _ = _step_calls(dry, HipTrainer(mk(), "diffusion", "adam", 1e-3, use_graph=False, cond_cols=C), batch)
        tr = HipTrainer(mk(), "diffusion", "adam", 1e-3, use_graph=False, cond_cols=C, loss_weight=None)
        got, _ = _step_calls(dry, tr, batch)
        assert got == want, "name for name"
        assert tr.loss_weight is None and tr.level_table is None and tr.level_accum is None
        assert not WEIGHTED_SEAM & set(want)
        if model == "chain_mlp" and C == 0:
            assert "ib_mlp_chain_train" in want and not PLAIN_SEAM & set(want)
        else:
            assert (PLAIN_SEAM & set(want)) == ({"ib_mse_loss_partial_cond", "ib_mse_loss_finalize_cond"} if C else
                                                {"ib_mse_loss_partial", "ib_mse_loss_finalize"})
        with pytest.raises(dry.HipError, match="without a loss_weight"):
            tr.level_loss()


@pytest.mark.parametrize("model", sorted(MODELS))
def test_on_replaces_exactly_the_loss_seam(dry, model):
    from inferbiomechanics_amd.diffusion.schedule import alphas_cumprod
    from inferbiomechanics_amd.engine import HipTrainer
    from inferbiomechanics_amd.loss_weight import LossWeight
    from inferbiomechanics_amd._tuning import tuning as TU
    mk, mb = MODELS[model]
    batch = mb()
    B, T, D = batch[0].shape
    swap = {"ib_mse_loss_partial": "ib_mse_loss_weighted_partial", "ib_mse_loss_partial_cond": "ib_mse_loss_weighted_partial",
            "ib_mse_loss_finalize": "ib_mse_loss_weighted_finalize", "ib_mse_loss_finalize_cond": "ib_mse_loss_weighted_finalize"}
    for C in (0, 14):
        if model == "chain_mlp":
            TU.no_chain = True                   # the yardstick of a weighted MLP step is the per-op step
        try:
            plain = HipTrainer(mk(), "diffusion", "adam", 1e-3, use_graph=False, cond_cols=C)
            want, _ = _step_calls(dry, plain, batch)
        finally:
            if model == "chain_mlp":
                del TU.no_chain
        lw = LossWeight("min_snr", gamma=5.0)
        tr = HipTrainer(mk(), "diffusion", "adam", 1e-3, use_graph=False, cond_cols=C, loss_weight=lw)
        if model == "chain_mlp":
            assert tr.plan.chain_ok(D) and not tr.plan.chain_ok(D, 0, weighted=True)
        assert tr.level_table.dtype == torch.float32 and tr.level_table.numel() == 1000
        assert np.array_equal(tr.level_table.numpy(), lw.weights(alphas_cumprod(1000)))
        assert tr.level_accum.dtype == torch.float64 and tr.level_accum.numel() == 2 + 2 * NB
        for _ in range(2):
            got, args = _step_calls(dry, tr, batch)
            assert got == [swap.get(n, n) for n in want], "every other launch is the unweighted step's, in its order"
            assert got.count("ib_mse_loss_weighted_partial") == 1 == got.count("ib_mse_loss_weighted_finalize")
            assert not PLAIN_SEAM & set(got) and "ib_mlp_chain_train" not in got
            a = [x for n, x in args if n == "ib_mse_loss_weighted_partial"][0]
            f = [x for n, x in args if n == "ib_mse_loss_weighted_finalize"][0]
            t_ptr = a[5]
            assert a[6] == tr.level_table.data_ptr() and a[7:9] == (1000, T) and a[11:14] == (B * T, D, C) and a[3] is not None
            assert f[2] == t_ptr and f[3:5] == (B, 1000) and f[5] == tr.result.data_ptr() and f[6] == tr.level_accum.data_ptr()
            assert f[7:9] == (B * T * D, B * T * (D - C)) and f[0] == a[9] and f[1] == a[10]
        rep = tr.level_loss(reset=True)          # a dry run computes nothing: the shape of the report
        assert rep["steps"] == 2 and rep["windows"] == [0] * NB and len(rep["bands"]) == NB
        assert [(lo, hi) for lo, hi, _ in rep["bands"]] == [(125 * k, 125 * (k + 1)) for k in range(NB)]
        assert all(m is None for _, _, m in rep["bands"]) and tr.level_loss()["steps"] == 0


def test_on_combines_with_the_other_options(dry):
    from inferbiomechanics_amd.engine import HipTrainer
    from inferbiomechanics_amd.loss_weight import LossWeight
    from inferbiomechanics_amd.lr_schedule import LrSchedule
    kw = dict(cond_cols=14, cond_drop=0.1, ema_decay=0.999, weight_decay=0.1, max_grad_norm=0.5,
              lr_schedule=LrSchedule("cosine", 5, 15, 0.1))
    plain, _ = _step_calls(dry, HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, **kw), _batch())
    tr = HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, loss_weight=LossWeight("uniform"), **kw)
    got, _ = _step_calls(dry, tr, _batch())
    assert [n.replace("_weighted", "").replace("partial", "partial_cond").replace("finalize", "finalize_cond")
            if "weighted" in n else n for n in got] == plain
    assert "ib_q_sample_cond_drop" in got and got[-2:] == ["ib_grad_sumsq", "ib_optim_step_gradnorm"]
    with pytest.raises(ValueError, match="diffusion"):
        from inferbiomechanics_amd.models.FeedForwardRegressionBaseline import FeedForwardBaseline
        HipTrainer(FeedForwardBaseline(23, 2, 50, "all_frames", "sigmoid", 5, 10), "regression", "adam", 1e-3,
                   args=argparse.Namespace(predict_grf_components=list(range(6)), predict_cop_components=list(range(6)),
                                           predict_moment_components=list(range(6)), predict_wrench_components=list(range(12))),
                   loss_weight=LossWeight("uniform"))


def test_a_step_that_raises_is_not_counted(dry):
    from inferbiomechanics_amd.engine import HipTrainer
    from inferbiomechanics_amd.loss_weight import LossWeight
    tr = HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, cond_cols=30, loss_weight=LossWeight("uniform"))
    with pytest.raises(ValueError, match="cond_cols"):
        tr.step(_batch())                        # 30 columns: nothing is left to score, refused before any launch
    assert tr.level_loss(reset=False)["steps"] == 0 and tr.steps_done == 0


def test_trainer_state_dict_round_trip_of_the_weight(dry):
    from inferbiomechanics_amd.engine import HipTrainer
    from inferbiomechanics_amd.loss_weight import LossWeight
    mk = lambda **kw: HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, **kw)
    tr = mk(loss_weight=LossWeight("min_snr", gamma=5.0))
    for _ in range(3):
        tr.step(_batch())
    sd = tr.optimizer_state_dict()
    assert sd["loss_weight"] == {"kind": "min_snr", "gamma": 5.0, "table": None} and sd["step"] == 3
    again = mk(loss_weight=LossWeight("min_snr", gamma=5))
    again.load_optimizer_state_dict(sd)
    assert again.steps_done == 3
    tab = np.linspace(0.5, 1.5, 1000)
    for other in (dict(), dict(loss_weight=LossWeight("min_snr", gamma=4.0)), dict(loss_weight=LossWeight("uniform")),
                  dict(loss_weight=LossWeight("table", table=tab))):
        t2 = mk(**other)
        with pytest.raises(dry.HipError, match=r"the checkpoint's loss weighting \(min_snr\(gamma=5\)\) differs from this "
                                               r"trainer's \((none|min_snr\(gamma=4\)|uniform|table\[1000\])\)"):
            t2.load_optimizer_state_dict(sd)
        assert t2.steps_done == 0, "nothing was loaded"
    plain_sd = mk().optimizer_state_dict()
    assert plain_sd["loss_weight"] is None
    with pytest.raises(dry.HipError, match=r"loss weighting \(none\) differs from this trainer's \(min_snr\(gamma=5\)\)"):
        again.load_optimizer_state_dict(plain_sd)
    old = {k: v for k, v in plain_sd.items() if k != "loss_weight"}            # an older checkpoint: no weighting
    mk().load_optimizer_state_dict(old)
    with pytest.raises(dry.HipError, match=r"loss weighting \(none\) differs"):
        again.load_optimizer_state_dict(old)
    # a table travels with the checkpoint, value for value; uniform ignores gamma
    tt = mk(loss_weight=LossWeight("table", table=tab))
    tsd = tt.optimizer_state_dict()
    assert tsd["loss_weight"]["kind"] == "table" and tsd["loss_weight"]["table"] == tab.tolist()
    mk(loss_weight=LossWeight("table", table=tab.copy())).load_optimizer_state_dict(tsd)
    with pytest.raises(dry.HipError, match="loss weighting"):
        mk(loss_weight=LossWeight("table", table=tab + 1e-9)).load_optimizer_state_dict(tsd)
    mk(loss_weight=LossWeight("uniform", gamma=3.0)).load_optimizer_state_dict(mk(loss_weight=LossWeight("uniform")).optimizer_state_dict())
    assert LossWeight.from_fields(tsd["loss_weight"]) == LossWeight("table", table=tab) and LossWeight.from_fields(None) is None
    # torch.optim's grammar is as it was
    assert tr.torch_optimizer_state_dict()["param_groups"] == mk().torch_optimizer_state_dict()["param_groups"]


# ---------------------------------------------------------------------------------------------------------------------
# 4. the command line
# ---------------------------------------------------------------------------------------------------------------------
def _train(*a):
    from inferbiomechanics_amd.cli.train import TrainCommand
    p = argparse.ArgumentParser()
    TrainCommand().register_subcommand(p.add_subparsers(dest="command"))
    return p.parse_args(["train"] + list(a))


DIFF = ("--model-type", "diffusion-mlp")


def test_cli_flags_defaults_and_refusals():
    from inferbiomechanics_amd.cli.train import resolve_loss_weight
    from inferbiomechanics_amd.loss_weight import LossWeight
    a = _train()
    assert a.loss_weight == "off" and a.min_snr_gamma == 5.0
    assert resolve_loss_weight(_train()) is None and resolve_loss_weight(_train("--eager")) is None
    assert resolve_loss_weight(_train(*DIFF, "--loss-weight", "off", "--eager")) is None
    assert resolve_loss_weight(_train(*DIFF, "--loss-weight", "min-snr")) == LossWeight("min_snr", gamma=5.0)
    assert resolve_loss_weight(_train(*DIFF, "--loss-weight", "min-snr", "--min-snr-gamma", "1.5")) == LossWeight("min_snr", gamma=1.5)
    assert resolve_loss_weight(_train(*DIFF, "--loss-weight", "uniform")) == LossWeight("uniform")
    with pytest.raises(SystemExit, match="--loss-weight needs the fused trainer"):
        resolve_loss_weight(_train(*DIFF, "--loss-weight", "min-snr", "--eager"))
    with pytest.raises(SystemExit, match="--loss-weight needs the fused trainer"):
        resolve_loss_weight(_train(*DIFF, "--loss-weight", "uniform", "--eager"))
    for bad in ("0", "-1", "nan", "inf"):
        with pytest.raises(SystemExit, match="--min-snr-gamma"):
            resolve_loss_weight(_train(*DIFF, "--loss-weight", "min-snr", "--min-snr-gamma", bad))
    with pytest.raises(SystemExit, match="diffusion model type"):
        resolve_loss_weight(_train("--model-type", "feedforward", "--loss-weight", "min-snr"))
    with pytest.raises(SystemExit):
        _train("--loss-weight", "snr")           # argparse: not one of the choices


BASE = ['--no-wandb', '--synthetic-windows', '24', '--batch-size', '8', '--data-loading-workers', '0', '--model-type',
        'diffusion-mlp', '--feat-dim', '24', '--hidden-dims', '32', '32', '--stride', '1', '--history-len', '6', '--seed', '7']


def test_train_with_loss_weight_in_dry_run(dry, tmp_path, capsys):
    """a weighted run from start to resume: refused with --eager before anything is written, every step the weighted pair, the
    report lines printed, the value saved, a resume with another value refused, with the same value accepted"""
    from inferbiomechanics_amd.cli.train import TrainCommand
    ck = str(tmp_path / "ck")
    common = BASE + ['--checkpoint-dir', ck, '--window-cache', 'hbm', '--report-every', '2']
    with pytest.raises(SystemExit, match="--loss-weight needs the fused trainer"):
        TrainCommand().run(_train(*common, '--epochs', '1', '--loss-weight', 'min-snr', '--eager'))
    assert not os.path.exists(ck)
    lib = dry.lib()
    lib.calls.clear()
    assert TrainCommand().run(_train(*common, '--epochs', '1', '--loss-weight', 'min-snr', '--min-snr-gamma', '4'))
    steps = lib.calls.count("ib_mse_loss_weighted_partial")
    assert steps == 3 == lib.calls.count("ib_mse_loss_weighted_finalize") and not PLAIN_SEAM & set(lib.calls)
    out = capsys.readouterr().out
    assert "Loss weighting by noise level: min_snr(gamma=4)" in out
    assert "unweighted eps-MSE" in out and "eps-MSE per noise-level band: t 0-124 " in out
    with pytest.raises(SystemExit, match="Resume with the same --loss-weight / --min-snr-gamma"):
        TrainCommand().run(_train(*common, '--epochs', '2'))
    with pytest.raises(SystemExit, match="Resume with the same --loss-weight / --min-snr-gamma"):
        TrainCommand().run(_train(*common, '--epochs', '2', '--loss-weight', 'min-snr'))
    lib.calls.clear()
    assert TrainCommand().run(_train(*common, '--epochs', '2', '--loss-weight', 'min-snr', '--min-snr-gamma', '4'))
    assert lib.calls.count("ib_mse_loss_weighted_partial") == 3, "one more epoch"


def test_format_level_report():
    from inferbiomechanics_amd.cli.train import format_level_report
    rep = {"bands": [(0, 1, 0.5), (1, 2, None), (2, 2, None), (2, 4, 1.25)]}
    assert format_level_report(rep) == "t 0-0 0.5  t 1-1 -  t 2-3 1.25"


# ---------------------------------------------------------------------------------------------------------------------
# 5. the kernels' registers
# ---------------------------------------------------------------------------------------------------------------------
def test_weighted_kernels_use_no_scratch():
    """the band accumulators stay in registers: no form of the new kernels spills or touches scratch (compile only)"""
    from tools import kernel_resources as kr
    if kr.hipcc() is None:
        pytest.skip("hipcc not installed")
    rows = {k["kernel"]: k for k in kr.resources("loss_weight.hip")}
    forms = ["mse_weighted_partial_kernel<float,4>", "mse_weighted_partial_kernel<float,1>",
             "mse_weighted_partial_kernel<bf16,4>", "mse_weighted_partial_kernel<bf16,1>", "mse_weighted_final_kernel"]
    assert sorted(rows) == sorted(forms)
    for name in forms:
        k = rows[name]
        assert not k["scratch"] and not k["vgpr_spill"] and not k["sgpr_spill"], k
        assert k["occupancy"] >= 4, k
