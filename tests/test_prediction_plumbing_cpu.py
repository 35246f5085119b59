"""Host side of x0- and v-prediction without a GPU: the tables against closed forms written here, the float64 restatements'
round trips, the fifteenth header and the build, the binding's table and marshalling, the refusals of the live library before
any launch, the trainer's and the samplers' launches in dry-run traces (eps: the launches as ever, name for name; v / x0:
exactly the loss seam and one launch per sampler step differ), the checkpoint round trips, the command line."""
import argparse
import os
import re
import subprocess

import numpy as np
import pytest
import torch

NAMES = ["ib_mse_loss_pred_partial", "ib_pred_to_eps"]
NB = 8
PLAIN_SEAM = {"ib_mse_loss_partial", "ib_mse_loss_finalize", "ib_mse_loss_partial_cond", "ib_mse_loss_finalize_cond"}
KINDS = ("eps", "x0", "v")


@pytest.fixture()
def dry():
    from inferbiomechanics_amd import hip
    hip.set_dry_run(True)
    yield hip
    hip.set_dry_run(False)


def _ab(n=1000):
    from inferbiomechanics_amd.diffusion.schedule import alphas_cumprod
    ab = alphas_cumprod(n).numpy()
    assert ab.dtype == np.float64
    return ab


# ---------------------------------------------------------------------------------------------------------------------
# 1. the tables and the restatements
# ---------------------------------------------------------------------------------------------------------------------
def test_eps_units_match_the_closed_form():
    from inferbiomechanics_amd import prediction as P
    assert P.KINDS == KINDS
    ab = _ab()
    assert np.array_equal(P.eps_units64(ab, "eps"), np.ones(1000))
    assert np.array_equal(P.eps_units64(ab, "x0"), ab / (1.0 - ab))
    assert np.array_equal(P.eps_units64(ab, "v"), ab)
    for kind in KINDS:
        u = P.eps_units(ab, kind)
        assert u.dtype == np.float32 and np.array_equal(u, P.eps_units64(ab, kind).astype(np.float32)), "cast to fp32 once"
        assert np.array_equal(P.eps_units64(torch.from_numpy(ab), kind), P.eps_units64(ab, kind))
    for bad in ("noise", "", None, "V"):
        with pytest.raises(ValueError, match="prediction"):
            P.eps_units64(ab, bad)
    for bad in (np.array([1.0, 0.5]), np.array([0.0]), np.ones((2, 2)) * 0.5, np.zeros(0)):
        with pytest.raises(ValueError, match="alpha_bar"):
            P.eps_units64(bad, "v")


def test_min_snr_per_prediction_kind():
    from inferbiomechanics_amd.loss_weight import LossWeight
    ab = _ab()
    snr = ab / (1.0 - ab)
    for gamma in (1.0, 5.0, 20.0):
        lw = LossWeight("min_snr", gamma=gamma)
        w_eps, w_x0, w_v = (lw.weights64(ab, k) for k in KINDS)
        assert np.array_equal(w_eps, lw.weights64(ab)), "the default argument is eps, as before"
        assert np.array_equal(w_eps, np.minimum(1.0, gamma / snr))
        assert np.array_equal(w_x0, np.minimum(snr, gamma))
        assert np.array_equal(w_v, np.minimum(snr, gamma) / (snr + 1.0))
        # the three forms weight the same x0 error: w_x0 = snr w_eps, w_v = ab w_eps, to a few float64 roundings
        np.testing.assert_allclose(w_x0, snr * w_eps, rtol=4e-16, atol=0)
        np.testing.assert_allclose(w_v, ab * w_eps, rtol=1e-15, atol=0)
        for k in KINDS:
            w = lw.weights(ab, k)
            assert w.dtype == np.float32 and np.array_equal(w, lw.weights64(ab, k).astype(np.float32))
    tab = np.linspace(0.0, 2.0, 1000)
    for k in KINDS:                                 # uniform and table weight the target's own squared error: unchanged
        assert np.array_equal(LossWeight("uniform").weights(ab, k), np.ones(1000, dtype=np.float32))
        assert np.array_equal(LossWeight("table", table=tab).weights(ab, k), tab.astype(np.float32))
    with pytest.raises(ValueError, match="prediction"):
        LossWeight("min_snr").weights(ab, "noise")


def test_restatement_round_trips():
    from inferbiomechanics_amd import prediction as P
    ab = _ab()
    g = np.random.default_rng(0)
    t = np.array([0, 1, 124, 125, 500, 998, 999])
    x0, eps = g.standard_normal((7, 5, 6)), g.standard_normal((7, 5, 6))
    a, s = np.sqrt(ab[t])[:, None, None], np.sqrt(1.0 - ab[t])[:, None, None]
    xt = a * x0 + s * eps
    assert np.array_equal(P.target64(x0, eps, ab[t], "eps"), eps) and np.array_equal(P.target64(x0, eps, ab[t], "x0"), x0)
    assert np.array_equal(P.target64(x0, eps, ab[t], "v"), a * eps - s * x0)
    for kind in KINDS:
        o = P.target64(x0, eps, ab[t], kind)
        # x0 at level 0 divides by sigma = 0.01: the error of x_t, 1e-16, is multiplied by 100
        np.testing.assert_allclose(P.pred_to_eps64(xt, o, ab[t], kind), eps, rtol=0, atol=1e-13)
    # the implied noise error of an output error q is sqrt(u) q, up to sign
    q = g.standard_normal((7, 5, 6))
    for kind in KINDS:
        o = P.target64(x0, eps, ab[t], kind)
        d = P.pred_to_eps64(xt, o + q, ab[t], kind) - P.pred_to_eps64(xt, o, ab[t], kind)
        u = P.eps_units64(ab, kind)[t][:, None, None]
        np.testing.assert_allclose(d * d, u * q * q, rtol=1e-9, atol=1e-12)


def test_inv_sqrt_table_is_made_on_demand():
    from inferbiomechanics_amd.diffusion.schedule import DiffusionTables
    tabs = DiffusionTables("cpu", 1000)
    assert tabs._inv_sqrt_1mab is None, "an eps model allocates nothing"
    inv = tabs.inv_sqrt_1mab
    assert inv.dtype == torch.float32 and inv is tabs.inv_sqrt_1mab
    assert np.array_equal(inv.numpy(), (1.0 / np.sqrt(1.0 - _ab())).astype(np.float32)), "float64, cast once"


# ---------------------------------------------------------------------------------------------------------------------
# 2. the header, the build, the binding
# ---------------------------------------------------------------------------------------------------------------------
def test_fifteenth_header_has_its_own_table_and_is_built():
    from inferbiomechanics_amd import hip
    assert os.path.basename(hip.PREDICT_HEADER_PATH) == "ib_hip_predict.h" and os.path.exists(hip.PREDICT_HEADER_PATH)
    assert hip.predict_decls() == NAMES == sorted(hip._PREDICT_SIGS)
    text = open(hip.PREDICT_HEADER_PATH).read()
    for n in NAMES:
        assert len(re.findall(rf"\bint {n}\(", text)) == 1
        assert hip._sig(n) == hip._PREDICT_SIGS[n]
        for table in (hip._SIGS, hip._STITCH_SIGS, hip._HEAD_SIGS, hip._SDE_SIGS, hip._CFG_SIGS, hip._RESAMPLE_SIGS,
                      hip._ENSEMBLE_SIGS, hip._CLIP_SIGS, hip._STANDARDIZE_SIGS, hip._SCHED_SIGS, hip._DECAY_SIGS,
                      hip._SWEEP_SIGS, hip._GRADNORM_SIGS, hip._LOSSWEIGHT_SIGS):
            assert n not in table, "the new table is disjoint from the other fourteen"
        assert n not in hip._SYMBOLS and hip._is_launch(n)
    assert len(hip._DECLARED) == len(hip._SYMBOLS) + 2 and len(hip._SIGS) == 127 and len(hip._HEADERS) == 8
    assert len(hip._SYMBOLS) == len(hip._EXPORTS) + 4
    c, vp, i64 = hip._c, hip._vp, hip._i64
    assert hip._sig("ib_mse_loss_pred_partial") == (c.c_int, [vp, i64, vp, vp, vp, i64, vp, vp, vp, vp, vp, c.c_int, i64, vp,
                                                              hip._sz, i64, i64, i64, c.c_int, c.c_int, vp])
    assert hip._sig("ib_pred_to_eps") == (c.c_int, [vp, vp, vp, vp, vp, vp, c.c_int, c.c_int, i64, i64, i64, i64, c.c_int, vp])
    assert [int(re.search(rf"^#define IB_PRED_{k} (\d)$", text, flags=re.M).group(1)) for k in ("EPS", "X0", "V")] == [0, 1, 2]
    assert hip.PRED_KINDS == {"eps": 0, "x0": 1, "v": 2}
    here = os.path.dirname(hip.__file__)
    mk = open(os.path.join(here, "csrc", "Makefile")).read()
    assert "predict.hip" in re.search(r"^SRCS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert re.search(r"^build/predict\.o build_ab/predict\.o: \.\./\.\./include/ib_hip_predict\.h", mk, flags=re.M)
    assert mk.index("\nall:") < mk.index("ib_hip_predict.h"), "the default goal stays `all`"
    src = open(os.path.join(here, "csrc", "predict.hip")).read()
    assert "ib_hip_predict.h" in src and "atomic" not in src.lower() and "fp contract(off)" in src
    for name in ("loss.hip", "loss_weight.hip"):
        other = open(os.path.join(here, "csrc", name)).read()
        assert "ib_hip_predict" not in other and "pred_partial" not in other, f"csrc/{name} stays as it was"
    for path in (hip.LIB_PATH, hip.AB_LIB_PATH):
        if not os.path.exists(path):
            pytest.fail(f"{path} is not built")
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        assert set(NAMES) <= {line.split()[-1] for line in out.splitlines() if line.strip()}, path
    root = os.path.dirname(here)
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "ib_hip_predict.h" in open(os.path.join(root, doc)).read(), doc
    assert "predict_decls" in open(os.path.join(root, "__graft_entry__.py")).read(), "build() checks the header's exports"


def test_host_argument_checks_of_the_live_library():
    """the checks that run before any launch, on the live library without a GPU: every refused call returns its code"""
    from inferbiomechanics_amd import hip
    lib = hip.lib()
    p = 4096                                     # never dereferenced: every call below is refused before a launch
    E_ARG = lib.ib_mse_loss_partial_cond(None, 44, None, None, 44, None, 0, 96, 44, 0, 0, None)
    E_WS = lib.ib_mse_loss_partial_cond(p, 44, p, None, 44, None, 0, 96, 44, 1, 0, None)
    assert E_ARG < 0 and E_WS < 0 and E_ARG != E_WS
    bytes_ = lib.ib_mse_loss_weighted_workspace(96 * 44)

    def partial(pred=p, x0=p, eps=p, t=p, wtab=p, utab=p, sa=p, sb=p, levels=50, rpw=12, wsp=p, wsb=bytes_, rows=96, cols=44,
                C=0, kind=2, dtype=0, ldp=44, dpred=None, ldd=0):
        return lib.ib_mse_loss_pred_partial(pred, ldp, x0, eps, dpred, ldd, t, wtab, utab, sa, sb, levels, rpw, wsp, wsb, rows,
                                            cols, C, kind, dtype, None)
    for null in ("pred", "x0", "eps", "t", "wtab", "utab", "sa", "sb"):
        assert partial(**{null: None}) == E_ARG, null
    assert partial(kind=3) == E_ARG and partial(kind=-1) == E_ARG
    assert partial(rpw=7) == E_ARG and partial(rpw=0) == E_ARG and partial(rpw=-12) == E_ARG
    assert partial(levels=0) == E_ARG and partial(levels=-1) == E_ARG
    assert partial(C=44) == E_ARG and partial(C=45) == E_ARG and partial(C=-1) == E_ARG
    assert partial(rows=0) == E_ARG and partial(cols=0) == E_ARG and partial(ldp=43) == E_ARG
    assert partial(dpred=p, ldd=43) == E_ARG
    assert partial(wsp=None) == E_WS and partial(wsb=bytes_ - 1) == E_WS
    for kind in (0, 1, 2):
        assert partial(kind=kind, dtype=5) < 0 and partial(kind=kind, dtype=5) not in (E_ARG, E_WS)

    def convert(x=p, out=p, t=p, sa=p, sb=p, inv=p, levels=50, kind=2, B=3, T=5, D=44, ld=48, dtype=0):
        return lib.ib_pred_to_eps(x, out, t, sa, sb, inv, levels, kind, B, T, D, ld, dtype, None)
    for null in ("x", "out", "t", "sa", "sb", "inv"):
        assert convert(**{null: None}) == E_ARG, null
    assert convert(kind=0) == E_ARG, "eps: the caller launches nothing"
    assert convert(kind=3) == E_ARG and convert(kind=-1) == E_ARG
    assert convert(levels=0) == E_ARG and convert(B=0) == E_ARG and convert(T=0) == E_ARG and convert(D=0) == E_ARG
    assert convert(D=49) == E_ARG and convert(B=1 << 40, T=1 << 20, ld=1 << 10, D=8) == E_ARG
    for kind in (1, 2):
        assert convert(kind=kind, dtype=5) < 0 and convert(kind=kind, dtype=5) not in (E_ARG, E_WS)


def test_binding_marshals_and_refuses(dry):
    lib = dry.lib()
    rows, D, T, n_levels = 24, 44, 12, 50
    pred_full, dfull = torch.zeros(rows, 48), torch.zeros(rows, 48)
    pred, x0, eps = pred_full[:, :D], torch.zeros(rows, D), torch.zeros(rows, D)
    t = torch.zeros(2, dtype=torch.int64)
    wtab, utab, sa, sb, inv = (torch.ones(n_levels) for _ in range(5))
    ws = torch.zeros(dry.mse_loss_weighted_workspace_bytes(rows * D), dtype=torch.uint8)
    for kind, code in (("eps", 0), ("x0", 1), ("v", 2)):
        dry.mse_loss_pred_partial(pred, x0, eps, ws, t, wtab, utab, sa, sb, T, kind, cond_cols=14, dpred=dfull[:, :D])
        assert lib.args[-1] == ("ib_mse_loss_pred_partial",
                                (pred.data_ptr(), 48, x0.data_ptr(), eps.data_ptr(), dfull.data_ptr(), 48, t.data_ptr(),
                                 wtab.data_ptr(), utab.data_ptr(), sa.data_ptr(), sb.data_ptr(), n_levels, T, ws.data_ptr(),
                                 ws.numel(), rows, D, 14, code, 0, 0))
    dry.mse_loss_pred_partial(pred, x0, eps, ws, t, wtab, utab, sa, sb, T, "v")
    assert lib.args[-1][1][4:6] == (None, 0) and lib.args[-1][1][17] == 0
    B, Tw, ld = 3, 5, 48
    x, out, tw = torch.zeros(B, Tw, ld), torch.zeros(B, Tw, ld), torch.zeros(B, dtype=torch.int64)
    for kind, code in (("x0", 1), ("v", 2)):
        assert dry.pred_to_eps(x, out, tw, sa, sb, inv, kind, D=44) is out
        assert lib.args[-1] == ("ib_pred_to_eps", (x.data_ptr(), out.data_ptr(), tw.data_ptr(), sa.data_ptr(), sb.data_ptr(),
                                                   inv.data_ptr(), n_levels, code, B, Tw, 44, ld, 0, 0))
    dry.pred_to_eps(x.bfloat16(), out.bfloat16(), tw, sa, sb, inv, "v")
    assert lib.args[-1][1][10:13] == (ld, ld, 1)
    n = len(lib.calls)
    for bad in (lambda: dry.mse_loss_pred_partial(pred, x0, eps, ws, t, wtab, utab, sa, sb, 7, "v"),
                lambda: dry.mse_loss_pred_partial(pred, x0, eps, ws, t, wtab, utab, sa, sb, T, "noise"),
                lambda: dry.mse_loss_pred_partial(pred, x0, eps, ws, t, wtab, utab, sa, sb, T, 2),
                lambda: dry.mse_loss_pred_partial(pred, x0, eps, ws, t, wtab, utab, sa, sb, T, "v", cond_cols=D),
                lambda: dry.mse_loss_pred_partial(pred, x0[:-1], eps, ws, t, wtab, utab, sa, sb, T, "v"),
                lambda: dry.mse_loss_pred_partial(pred, x0, eps.double(), ws, t, wtab, utab, sa, sb, T, "v"),
                lambda: dry.mse_loss_pred_partial(pred, x0, eps, ws, t[:1], wtab, utab, sa, sb, T, "v"),
                lambda: dry.mse_loss_pred_partial(pred, x0, eps, ws, t, wtab, utab[:-1], sa, sb, T, "v"),
                lambda: dry.mse_loss_pred_partial(pred, x0, eps, ws, t, wtab, utab, sa.double(), sb, T, "v"),
                lambda: dry.mse_loss_pred_partial(pred, x0, eps, ws, t, wtab, utab, sa, sb[::2], T, "v"),
                lambda: dry.mse_loss_pred_partial(pred, x0, eps, ws[:-1], t, wtab, utab, sa, sb, T, "v"),
                lambda: dry.mse_loss_pred_partial(pred, x0, eps, ws, t, wtab, utab, sa, sb, T, "v", dpred=torch.zeros(rows, D + 1)),
                lambda: dry.pred_to_eps(x, out, tw, sa, sb, inv, "eps"),
                lambda: dry.pred_to_eps(x, out, tw, sa, sb, inv, "noise"),
                lambda: dry.pred_to_eps(x, out[:2], tw, sa, sb, inv, "v"),
                lambda: dry.pred_to_eps(x, out.bfloat16(), tw, sa, sb, inv, "v"),
                lambda: dry.pred_to_eps(x[:, :, :44], out[:, :, :44], tw, sa, sb, inv, "v"),
                lambda: dry.pred_to_eps(x, out, tw[:2], sa, sb, inv, "v"),
                lambda: dry.pred_to_eps(x, out, tw.int(), sa, sb, inv, "v"),
                lambda: dry.pred_to_eps(x, out, tw, sa, sb, inv[:-1], "x0"),
                lambda: dry.pred_to_eps(x, out, tw, sa, sb, inv, "v", D=49),
                lambda: dry.pred_to_eps(x, out, tw, sa, sb, inv, "v", D=0)):
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
def test_eps_is_the_trainer_without_the_argument(dry, model):
    from inferbiomechanics_amd.engine import HipTrainer
    mk, mb = MODELS[model]
    batch = mb()
    for C in (0, 14):
        want, wargs = _step_calls(dry, HipTrainer(mk(), "diffusion", "adam", 1e-3, use_graph=False, cond_cols=C), batch)
        m = mk()
        tr = HipTrainer(m, "diffusion", "adam", 1e-3, use_graph=False, cond_cols=C, prediction="eps")
        got, _ = _step_calls(dry, tr, batch)
        assert got == want, "name for name"
        assert "ib_mse_loss_pred_partial" not in got and "ib_mse_loss_weighted_finalize" not in got
        assert tr.prediction == "eps" == m.prediction and tr.units_table is None and tr.level_table is None
        assert tr.level_accum is None and m.tables(torch.device("cpu"))._inv_sqrt_1mab is None, "nothing is allocated"
        assert "prediction" not in tr.optimizer_state_dict()
        assert not any(e[0] == "prediction" for e in tr._sig)
        with pytest.raises(dry.HipError, match="without a loss_weight"):
            tr.level_loss()


@pytest.mark.parametrize("kind", ["x0", "v"])
@pytest.mark.parametrize("model", sorted(MODELS))
def test_x0_and_v_replace_exactly_the_loss_seam(dry, model, kind):
    from inferbiomechanics_amd.engine import HipTrainer
    from inferbiomechanics_amd.loss_weight import LossWeight
    from inferbiomechanics_amd import prediction as P
    from inferbiomechanics_amd._tuning import tuning as TU
    mk, mb = MODELS[model]
    batch = mb()
    B, T, D = batch[0].shape
    swap = {"ib_mse_loss_partial": "ib_mse_loss_pred_partial", "ib_mse_loss_partial_cond": "ib_mse_loss_pred_partial",
            "ib_mse_loss_weighted_partial": "ib_mse_loss_pred_partial",
            "ib_mse_loss_finalize": "ib_mse_loss_weighted_finalize", "ib_mse_loss_finalize_cond": "ib_mse_loss_weighted_finalize"}
    for C in (0, 14):
        for lw in (None, LossWeight("min_snr", gamma=5.0)):
            if model == "chain_mlp":
                TU.no_chain = True                   # the yardstick of an x0 / v MLP step is the per-op step
            try:
                plain = HipTrainer(mk(), "diffusion", "adam", 1e-3, use_graph=False, cond_cols=C, loss_weight=lw)
                want, _ = _step_calls(dry, plain, batch)
            finally:
                if model == "chain_mlp":
                    del TU.no_chain
            m = mk()
            tr = HipTrainer(m, "diffusion", "adam", 1e-3, use_graph=False, cond_cols=C, loss_weight=lw, prediction=kind)
            assert m.prediction == kind, "the samplers read the model"
            if model == "chain_mlp":
                assert tr.plan.chain_ok(D) and not tr.plan.chain_ok(D, 0, weighted=True)
            tabs = m.tables(torch.device("cpu"))
            ab = _ab()
            assert np.array_equal(tr.units_table.numpy(), P.eps_units(ab, kind))
            assert np.array_equal(tr.level_table.numpy(), np.ones(1000, dtype=np.float32) if lw is None else lw.weights(ab, kind))
            assert tr.level_accum.dtype == torch.float64 and tr.level_accum.numel() == 2 + 2 * NB
            for _ in range(2):
                got, args = _step_calls(dry, tr, batch)
                assert got == [swap.get(n, n) for n in want], "every other launch is the eps step's, in its order"
                assert got.count("ib_mse_loss_pred_partial") == 1 == got.count("ib_mse_loss_weighted_finalize")
                assert not PLAIN_SEAM & set(got) and "ib_mlp_chain_train" not in got
                assert "ib_mse_loss_weighted_partial" not in got
                a = [x for n, x in args if n == "ib_mse_loss_pred_partial"][0]
                f = [x for n, x in args if n == "ib_mse_loss_weighted_finalize"][0]
                q = [x for n, x in args if n.startswith("ib_q_sample")][0]
                assert a[2:4] == q[0:2], "x0 and eps are the buffers the forward noising read"
                assert a[7:11] == (tr.level_table.data_ptr(), tr.units_table.data_ptr(), tabs.sqrt_ab.data_ptr(),
                                   tabs.sqrt_1mab.data_ptr())
                assert a[11:13] == (1000, T) and a[15:19] == (B * T, D, C, P.KINDS.index(kind)) and a[4] is not None
                assert f[2] == a[6] and f[3:5] == (B, 1000) and f[5] == tr.result.data_ptr() and f[6] == tr.level_accum.data_ptr()
                assert f[7:9] == (B * T * D, B * T * (D - C)) and f[0] == a[13] and f[1] == a[14]
            assert ("prediction", kind) in tr._sig, "the capture signature includes the kind"
            rep = tr.level_loss(reset=True)          # kept with and without a loss_weight; a dry run computes nothing
            assert rep["steps"] == 2 and rep["windows"] == [0] * NB and len(rep["bands"]) == NB
            assert tr.level_loss()["steps"] == 0


def test_bad_values_are_refused():
    from inferbiomechanics_amd.engine import HipTrainer
    for bad in ("noise", "", None, "V", 2):
        with pytest.raises(ValueError, match="prediction"):
            HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, prediction=bad)
    m = _mlp()
    m.prediction = "x0"
    for other in ("eps", "v"):
        with pytest.raises(ValueError, match="the model predicts 'x0'"):
            HipTrainer(m, "diffusion", "adam", 1e-3, use_graph=False, prediction=other)
    with pytest.raises(ValueError, match="diffusion"):
        from inferbiomechanics_amd.models.FeedForwardRegressionBaseline import FeedForwardBaseline
        HipTrainer(FeedForwardBaseline(23, 2, 50, "all_frames", "sigmoid", 5, 10), "regression", "adam", 1e-3,
                   args=argparse.Namespace(predict_grf_components=list(range(6)), predict_cop_components=list(range(6)),
                                           predict_moment_components=list(range(6)), predict_wrench_components=list(range(12))),
                   prediction="v")


def test_trainer_state_dict_round_trip_of_the_kind(dry):
    from inferbiomechanics_amd.engine import HipTrainer
    mk = lambda **kw: HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, **kw)
    tr = mk(prediction="v")
    for _ in range(3):
        tr.step(_batch())
    sd = tr.optimizer_state_dict()
    assert sd["prediction"] == "v" and sd["step"] == 3 and sd["loss_weight"] is None
    again = mk(prediction="v")
    again.load_optimizer_state_dict(sd)
    assert again.steps_done == 3
    for other in ("eps", "x0"):
        t2 = mk(prediction=other)
        with pytest.raises(dry.HipError, match=rf"the checkpoint's prediction \(v\) differs from this trainer's \({other}\)"):
            t2.load_optimizer_state_dict(sd)
        assert t2.steps_done == 0, "nothing was loaded"
    plain_sd = mk().optimizer_state_dict()
    assert "prediction" not in plain_sd, "an eps trainer's payload is what it was"
    with pytest.raises(dry.HipError, match=r"the checkpoint's prediction \(eps\) differs from this trainer's \(v\)"):
        again.load_optimizer_state_dict(plain_sd)
    mk().load_optimizer_state_dict(plain_sd)
    assert tr.torch_optimizer_state_dict()["param_groups"] == mk().torch_optimizer_state_dict()["param_groups"]


# ---------------------------------------------------------------------------------------------------------------------
# 4. the samplers
# ---------------------------------------------------------------------------------------------------------------------
def _sampler_runs():
    """(name, make(model), call(sampler)) over the four classes, pitched (bf16) and unpitched (fp32) states, a guided loop
    and a clipped one"""
    from inferbiomechanics_amd.diffusion import sampler as S
    T, D, F = 8, 44, 17
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g)
    mask = torch.zeros(T, D, dtype=torch.bool)
    mask[:, :14] = True
    cols = mask[0].clone()
    x, o, z, q = r(3, T, D), r(3, T, D), r(2, F, D), r(2, F, D)
    clip = S.X0Clip((-3.0,) * D, (3.0,) * D, "range")
    return [("ddim", lambda m: S.DDIMSampler(m, 4, use_graph=False), lambda s: s.sample(x)),
            ("ddim_eta", lambda m: S.DDIMSampler(m, 4, use_graph=False, eta=0.5, seed=1), lambda s: s.sample(x)),
            ("dpmpp2m", lambda m: S.DDIMSampler(m, 4, use_graph=False, solver="dpmpp2m", spacing="logsnr"), lambda s: s.sample(x)),
            ("cond", lambda m: S.ConditionalDDIMSampler(m, 4, use_graph=False), lambda s: s.sample(x, o, mask)),
            ("cond_clip", lambda m: S.ConditionalDDIMSampler(m, 4, use_graph=False, x0_clip=clip), lambda s: s.sample(x, o, mask)),
            ("cond_guided", lambda m: S.ConditionalDDIMSampler(m, 4, use_graph=False, observations="clean", guidance=1.5),
             lambda s: s.sample(x, o, mask)),
            ("stitched", lambda m: S.StitchedDDIMSampler(m, 4, hop=3, use_graph=False), lambda s: s.sample(z, q, cols)),
            ("stitched_sde", lambda m: S.StochasticStitchedSampler(m, 4, eta=0.5, hop=3, seed=1, use_graph=False),
             lambda s: s.sample(z, q, cols))]


def _sampler_model(dtype, kind=None):
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    torch.manual_seed(0)
    m = DiffusionTransformer(44, 8, d_model=64, num_heads=4, dim_feedforward=128, num_layers=2, compute_dtype=dtype)
    m.cond_cols, m.cond_drop = 14, 0.1
    if kind is not None:
        m.prediction = kind
    return m


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("which", range(8), ids=[r[0] for r in _sampler_runs()])
def test_samplers_add_one_launch_per_step(dry, which, dtype):
    name, make, call = _sampler_runs()[which]
    lib = dry.lib()

    def run(kind):
        m = _sampler_model(dtype, kind)
        lib.calls.clear()
        del lib.args[:]
        s = make(m)
        call(s)
        return m, s, list(lib.calls), list(lib.args)
    _, s0, plain, _ = run(None)
    _, s1, eps, _ = run("eps")
    assert eps == plain and "ib_pred_to_eps" not in plain and len(s1._sig) == len(s0._sig)
    assert not any(e == "prediction" for e in s1._sig)
    for kind in ("x0", "v"):
        m, s, got, args = run(kind)
        assert [n for n in got if n != "ib_pred_to_eps"] == plain, "every other launch is the eps loop's, in its order"
        assert got.count("ib_pred_to_eps") == 4, "one per step"
        i = s._sig.index("prediction")
        assert s._sig[i + 1] == kind, "the kind is part of the capture signature"
        tabs = m.tables(torch.device("cpu"))
        for k, n in enumerate(got):
            if n != "ib_pred_to_eps":
                continue
            # directly behind the forward (the guided step: behind the combination), before the clip and the update
            step = ("ib_ddim_", "ib_dpmpp_", "ib_stitch_", "ib_sde_")
            before, after = got[k - 1], got[k + 1]
            if name == "cond_guided":
                assert before == "ib_cfg_combine"
            else:
                assert not before.startswith(step + ("ib_x0_clip", "ib_counter", "ib_cfg")), (name, before)
            assert after == "ib_x0_clip_range" if name == "cond_clip" else after.startswith(step), (name, after)
            a = args[k][1]
            B = s._bufs["x"].shape[0]
            assert a[0] == s._bufs["x"].data_ptr() and a[2] == s._bufs["t"].data_ptr()
            assert a[3:6] == (tabs.sqrt_ab.data_ptr(), tabs.sqrt_1mab.data_ptr(), tabs.inv_sqrt_1mab.data_ptr())
            assert a[6:8] == (1000, {"x0": 1, "v": 2}[kind]) and a[8:11] == (B, 8, 44) and a[11] == s._bufs["x"].shape[2]
            if "eps" in s._bufs:
                assert a[1] == s._bufs["eps"].data_ptr(), "the first half of the noise buffer in a guided step"


def test_label_predictor_reads_the_model(dry):
    from tools import sampler_trace
    from inferbiomechanics_amd.models.DiffusionLabelPredictor import DiffusionLabelPredictor
    lib = dry.lib()
    r = sampler_trace.Run()

    def run(kind):
        m = r.model(torch.bfloat16, **sampler_trace.LABELS)
        if kind:
            m.prediction = kind
        m.column_stats = torch.stack([torch.zeros(177), torch.ones(177)], dim=1)
        pred = DiffusionLabelPredictor(m, 4, seed=11, use_graph=False)
        lib.calls.clear()
        pred(sampler_trace._label_inputs(r, 2, 10))
        return list(lib.calls)
    plain, v = run(None), run("v")
    assert [n for n in v if n != "ib_pred_to_eps"] == plain and v.count("ib_pred_to_eps") == 4


# ---------------------------------------------------------------------------------------------------------------------
# 5. the command line and the checkpoint
# ---------------------------------------------------------------------------------------------------------------------
def _train(*a):
    from inferbiomechanics_amd.cli.train import TrainCommand
    p = argparse.ArgumentParser()
    TrainCommand().register_subcommand(p.add_subparsers(dest="command"))
    return p.parse_args(["train"] + list(a))


DIFF = ("--model-type", "diffusion-mlp")


def test_cli_flag_default_and_refusals():
    from inferbiomechanics_amd.cli.train import resolve_prediction
    assert _train().prediction == "eps"
    assert resolve_prediction(_train()) == "eps" and resolve_prediction(_train("--eager")) == "eps"
    assert resolve_prediction(_train("--model-type", "feedforward")) == "eps"
    assert resolve_prediction(_train(*DIFF, "--prediction", "eps", "--eager")) == "eps"
    assert resolve_prediction(_train(*DIFF, "--prediction", "v")) == "v"
    assert resolve_prediction(_train(*DIFF, "--prediction", "x0")) == "x0"
    for kind in ("x0", "v"):
        with pytest.raises(SystemExit, match="--prediction needs the fused trainer"):
            resolve_prediction(_train(*DIFF, "--prediction", kind, "--eager"))
        with pytest.raises(SystemExit, match="diffusion model type"):
            resolve_prediction(_train("--model-type", "feedforward", "--prediction", kind))
    with pytest.raises(SystemExit):
        _train("--prediction", "noise")          # argparse: not one of the choices


BASE = ['--no-wandb', '--synthetic-windows', '24', '--batch-size', '8', '--data-loading-workers', '0', '--model-type',
        'diffusion-mlp', '--feat-dim', '24', '--hidden-dims', '32', '32', '--stride', '1', '--history-len', '6', '--seed', '7']


def test_train_with_prediction_in_dry_run(dry, tmp_path, capsys):
    """a v run from start to resume: refused with --eager before anything is written, every step the new loss launch, the
    dev-set evaluation converted, the kind saved in the checkpoint only when not eps and restored into the model, a resume
    with another value refused, with the same value accepted"""
    from inferbiomechanics_amd.cli.abstract_command import AbstractCommand
    from inferbiomechanics_amd.cli.train import TrainCommand
    ck = str(tmp_path / "ck")
    common = BASE + ['--checkpoint-dir', ck, '--window-cache', 'hbm', '--report-every', '2']
    with pytest.raises(SystemExit, match="--prediction needs the fused trainer"):
        TrainCommand().run(_train(*common, '--epochs', '1', '--prediction', 'v', '--eager'))
    assert not os.path.exists(ck)
    lib = dry.lib()
    lib.calls.clear()
    assert TrainCommand().run(_train(*common, '--epochs', '1', '--prediction', 'v'))
    assert lib.calls.count("ib_mse_loss_pred_partial") == 3 == lib.calls.count("ib_mse_loss_weighted_finalize")
    assert not PLAIN_SEAM & set(lib.calls)
    assert lib.calls.count("ib_pred_to_eps") > 0, "the dev-set evaluation converts the output"
    out = capsys.readouterr().out
    assert "The denoiser predicts v" in out and "v-prediction, unweighted" in out and "eps-MSE per noise-level band" in out
    sub = os.path.join(ck, "diffusion-mlp")
    files = sorted(f for f in os.listdir(sub) if f.endswith(".pt"))
    payload = torch.load(os.path.join(sub, files[-1]), map_location="cpu")
    assert payload["prediction"] == "v" and payload["optimizer_state_dict"]["prediction"] == "v"
    m = _mlp_for_ckpt()
    assert m.prediction == "eps"
    AbstractCommand.load_latest_checkpoint(TrainCommand(), m, checkpoint_dir=sub)
    assert m.prediction == "v", "abstract_command restores it"
    for other in ((), ('--prediction', 'x0')):
        with pytest.raises(SystemExit, match="[Rr]esume with the same (--prediction|value)"):
            TrainCommand().run(_train(*common, '--epochs', '2', *other))
    lib.calls.clear()
    assert TrainCommand().run(_train(*common, '--epochs', '2', '--prediction', 'v'))
    assert lib.calls.count("ib_mse_loss_pred_partial") == 3, "one more epoch"
    # an eps run writes no key
    ck2 = str(tmp_path / "ck2")
    assert TrainCommand().run(_train(*BASE, '--checkpoint-dir', ck2, '--window-cache', 'hbm', '--epochs', '1'))
    sub2 = os.path.join(ck2, "diffusion-mlp")
    files = sorted(f for f in os.listdir(sub2) if f.endswith(".pt"))
    payload = torch.load(os.path.join(sub2, files[-1]), map_location="cpu")
    assert "prediction" not in payload and "prediction" not in payload["optimizer_state_dict"]


def _mlp_for_ckpt():
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionMLP
    return DiffusionMLP(24, [32, 32])


# ---------------------------------------------------------------------------------------------------------------------
# 6. the kernels' registers
# ---------------------------------------------------------------------------------------------------------------------
def test_prediction_kernels_use_no_scratch():
    """no form of the new kernels spills or touches scratch (compile only)"""
    from tools import kernel_resources as kr
    if kr.hipcc() is None:
        pytest.skip("hipcc not installed")
    rows = {k["kernel"]: k for k in kr.resources("predict.hip")}
    assert len(rows) == 12 + 8, sorted(rows)
    for name, k in rows.items():
        assert name.startswith(("mse_pred_partial_kernel<", "pred_to_eps_kernel<")), name
        assert not k["scratch"] and not k["vgpr_spill"] and not k["sgpr_spill"], k
        assert k["occupancy"] >= 4, k
