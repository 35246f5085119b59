"""Host side of the velocity loss without a GPU: the two tables against the closed forms written here, the float64
restatement's analytic gradient against autograd, the sixteenth header and the build, the binding's table and marshalling, the
refusals of the live library before any launch, the trainer's loss seam in dry-run traces (off: the launches as ever, name for
name; on: exactly the loss seam differs, under every kind, weight and conditioning), the checkpoint keys, the command line."""
import argparse
import os
import re
import subprocess

import numpy as np
import pytest
import torch

NAMES = ["ib_vel_loss_finalize", "ib_vel_loss_frame_chunk", "ib_vel_loss_partial", "ib_vel_loss_workspace"]
NB = 8
KINDS = ("eps", "x0", "v")
SEAM = {"ib_mse_loss_partial", "ib_mse_loss_finalize", "ib_mse_loss_partial_cond", "ib_mse_loss_finalize_cond",
        "ib_mse_loss_weighted_partial", "ib_mse_loss_weighted_finalize", "ib_mse_loss_pred_partial"}


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
# 1. the tables and the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_levels", [50, 1000])
@pytest.mark.parametrize("gamma", [5.0, float("inf")])
def test_tables_match_the_closed_forms(n_levels, gamma):
    from inferbiomechanics_amd.velocity_loss import VelocityLoss, x0_units64
    ab = _ab(n_levels)
    snr = ab / (1.0 - ab)
    closed = {"eps": np.minimum(1.0, gamma / snr), "x0": np.minimum(snr, gamma), "v": np.minimum(snr, gamma) / (snr + 1.0)}
    units = {"eps": 1.0 / snr, "x0": np.ones(n_levels), "v": 1.0 - ab}
    for lam in (1.0, 0.3):
        vl = VelocityLoss(lam, gamma=gamma)
        for kind in KINDS:
            v64, x64 = vl.tables64(ab, kind)
            assert np.array_equal(v64, lam * closed[kind]), "vtab / lambda is Min-SNR in the form of the kind"
            np.testing.assert_allclose(x64, units[kind], rtol=4e-16, atol=0)
            assert np.array_equal(x64, x0_units64(ab, kind))
            # vtab = lambda m_t c_t^2 with m_t = min(snr, gamma), to a few float64 roundings
            np.testing.assert_allclose(v64, lam * vl.level_weights64(ab) * x64, rtol=1e-15, atol=0)
            v32, x32 = vl.tables(ab, kind)
            assert v32.dtype == x32.dtype == np.float32
            assert np.array_equal(v32, v64.astype(np.float32)) and np.array_equal(x32, x64.astype(np.float32)), "cast once"
            assert np.array_equal(vl.tables64(torch.from_numpy(ab), kind)[0], v64)
    if gamma == float("inf"):
        assert np.array_equal(VelocityLoss(2.0, gamma=gamma).tables64(ab, "eps")[0], np.full(n_levels, 2.0)), \
            "eps, gamma = inf: the plain difference of eps errors"


def test_a_callers_table_replaces_the_rule_and_bad_values_are_refused():
    from inferbiomechanics_amd.velocity_loss import VelocityLoss, x0_units64
    ab = _ab(50)
    tab = np.linspace(0.0, 2.0, 50)
    vl = VelocityLoss(0.5, table=tab)
    for kind in KINDS:
        v64, x64 = vl.tables64(ab, kind)
        np.testing.assert_allclose(v64, 0.5 * tab * x0_units64(ab, kind), rtol=1e-15, atol=0)
    assert np.array_equal(vl.level_weights64(ab), tab)
    with pytest.raises(ValueError, match="50 entries"):
        vl.tables64(_ab(1000), "eps")
    for bad in (0.0, -1.0, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="weight"):
            VelocityLoss(bad)
    for bad in (0.0, -5.0, float("nan"), "x"):
        with pytest.raises(ValueError, match="gamma"):
            VelocityLoss(1.0, gamma=bad)
    for bad in (np.ones((2, 2)), np.zeros(0), np.array([1.0, -1.0]), np.array([np.nan])):
        with pytest.raises(ValueError, match="table"):
            VelocityLoss(1.0, table=bad)
    with pytest.raises(ValueError, match="prediction"):
        VelocityLoss(1.0).tables64(ab, "noise")
    a, b = VelocityLoss(1.0, gamma=5.0), VelocityLoss.from_fields(VelocityLoss(1.0, gamma=5.0).fields())
    assert a == b and a != VelocityLoss(2.0) and a != VelocityLoss(1.0, gamma=float("inf")) and a != VelocityLoss(1.0, table=tab)
    assert VelocityLoss.from_fields(None) is None and vl == VelocityLoss.from_fields(vl.fields())
    assert set(a.fields()) == {"weight", "gamma", "table"}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T", [2, 3, 5])
def test_restatement_gradient_is_its_own_dpred(T, kind):
    from inferbiomechanics_amd.velocity_loss import VelocityLoss, velocity_terms64
    from inferbiomechanics_amd.loss_weight import LossWeight
    from inferbiomechanics_amd.prediction import eps_units64
    n_levels, B, D, C = 50, 6, 7, 3
    ab = _ab(n_levels)
    g = torch.Generator().manual_seed(T)
    r = lambda: torch.randn(B, T, D, generator=g, dtype=torch.float64)
    pred, x0, eps = r().requires_grad_(True), r(), r()
    t = torch.tensor([0, 49, 6, 7, 25, 60])                    # the last one is clamped to 49
    v, x = VelocityLoss(0.7).tables64(ab, kind)
    w, u = LossWeight("min_snr").weights64(ab, kind), eps_units64(ab, kind)
    e = velocity_terms64(pred, x0, eps, t, ab, kind, w, u, v, x, cond_cols=C)
    e["loss"].backward()
    assert torch.equal(e["loss"], e["mse"] + e["vel"])
    ref = e["dpred"].abs().max().item()
    assert (pred.grad - e["dpred"]).abs().max().item() <= 1e-12 * ref
    assert torch.equal(pred.grad[:, :, :C], torch.zeros(B, T, C, dtype=torch.float64)), "conditioning columns are not scored"
    assert torch.equal(e["dn"][:, -1], torch.zeros(B, D, dtype=torch.float64)) and torch.equal(e["dp"][:, 0], e["dn"][:, -1])
    assert torch.equal(e["dp"][:, 1:], e["dn"][:, :-1])
    np.testing.assert_allclose(e["dpred"], e["dm"] + (e["dp"] - e["dn"]) * e["vscale"] * e["v"], rtol=1e-14, atol=0)
    # the sums by hand: no difference crosses a window, the means divide by n and n_v
    tl = t.clamp(0, n_levels - 1)
    a, s = np.sqrt(ab[tl])[:, None, None], np.sqrt(1.0 - ab[tl])[:, None, None]
    target = {"eps": eps, "x0": x0, "v": torch.from_numpy(a) * eps - torch.from_numpy(s) * x0}[kind]
    q = (pred.detach() - target)[:, :, C:].numpy()
    dn = q[:, 1:] - q[:, :-1]
    lv = lambda tab: tab[tl][:, None, None]
    n, n_v = B * T * (D - C), B * (T - 1) * (D - C)
    np.testing.assert_allclose(float(e["mse"].detach()), (lv(w) * q * q).sum() / n, rtol=1e-13)
    np.testing.assert_allclose(float(e["vel"].detach()), (lv(v) * dn * dn).sum() / n_v, rtol=1e-13)
    np.testing.assert_allclose(float(e["eps_mse"]), (lv(u) * q * q).sum() / n, rtol=1e-13)
    np.testing.assert_allclose(float(e["x0_vel"]), (lv(x) * dn * dn).sum() / n_v, rtol=1e-13)
    band = (tl * NB // n_levels).numpy()
    assert e["counts"].tolist() == [int((band == k).sum()) for k in range(NB)]
    for k in range(NB):
        np.testing.assert_allclose(float(e["bands"][k]), (lv(u) * q * q)[band == k].sum(), rtol=1e-13)
        np.testing.assert_allclose(float(e["x0_bands"][k]), (lv(x) * dn * dn)[band == k].sum(), rtol=1e-13)
    with pytest.raises(ValueError, match="at least 2 frames"):
        velocity_terms64(pred[:, :1], x0[:, :1], eps[:, :1], t, ab, kind, w, u, v, x)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the header, the build, the binding
# ---------------------------------------------------------------------------------------------------------------------
def test_sixteenth_header_has_its_own_table_and_is_built():
    from inferbiomechanics_amd import hip
    assert os.path.basename(hip.VELOCITY_HEADER_PATH) == "ib_hip_velocity.h" and os.path.exists(hip.VELOCITY_HEADER_PATH)
    assert hip.velocity_decls() == NAMES == sorted(hip._VELOCITY_SIGS)
    text = open(hip.VELOCITY_HEADER_PATH).read()
    for n in NAMES:
        assert len(re.findall(rf"\b(?:int|size_t) {n}\(", text)) == 1
        assert hip._sig(n) == hip._VELOCITY_SIGS[n]
        for table in (hip._SIGS, hip._STITCH_SIGS, hip._HEAD_SIGS, hip._SDE_SIGS, hip._CFG_SIGS, hip._RESAMPLE_SIGS,
                      hip._ENSEMBLE_SIGS, hip._CLIP_SIGS, hip._STANDARDIZE_SIGS, hip._SCHED_SIGS, hip._DECAY_SIGS,
                      hip._SWEEP_SIGS, hip._GRADNORM_SIGS, hip._LOSSWEIGHT_SIGS, hip._PREDICT_SIGS):
            assert n not in table, "the new table is disjoint from the other fifteen"
        assert n not in hip._DECLARED and n not in hip._SYMBOLS and n not in hip._EXPORTS
    assert hip._is_launch("ib_vel_loss_partial") and hip._is_launch("ib_vel_loss_finalize")
    assert not hip._is_launch("ib_vel_loss_workspace") and not hip._is_launch("ib_vel_loss_frame_chunk"), "host queries"
    assert len(hip._DECLARED) == len(hip._SYMBOLS) + 2 and len(hip._SIGS) == 127 and len(hip._HEADERS) == 8
    c, vp, i64 = hip._c, hip._vp, hip._i64
    pred_sig = hip._sig("ib_mse_loss_pred_partial")[1]
    assert hip._sig("ib_vel_loss_partial") == (c.c_int, pred_sig[:9] + [vp, vp] + pred_sig[9:]), \
        "the arguments of ib_mse_loss_pred_partial plus vtab and xtab"
    assert hip._sig("ib_vel_loss_finalize") == (c.c_int, [vp, hip._sz, vp, c.c_int, vp, vp, i64, i64, i64, i64, vp])
    assert hip._sig("ib_vel_loss_workspace") == (hip._sz, [i64, i64, i64]) and hip._sig("ib_vel_loss_frame_chunk") == (c.c_int, [])
    define = lambda name: int(re.search(rf"^#define {name} \(?(\d+)", text, flags=re.M).group(1))
    assert define("IB_VEL_FRAME_CHUNK") == hip.VEL_FRAME_CHUNK == hip.lib().ib_vel_loss_frame_chunk()
    assert (hip.VEL_R_TOTAL, hip.VEL_R_EPS, hip.VEL_R_BANDS, hip.VEL_R_COUNTS) == (0, 1, 2, 2 + NB), \
        "the first 2 + 2 NB places are laid out as the weighted finalize's result"
    assert (hip.VEL_R_MSE, hip.VEL_R_VEL, hip.VEL_R_X0, hip.VEL_R_X0_BANDS, hip.VEL_RESULT_LEN) == \
        (2 + 2 * NB, 3 + 2 * NB, 4 + 2 * NB, 5 + 2 * NB, 5 + 3 * NB)
    for name, add, nbs in (("IB_VEL_R_MSE", 2, 2), ("IB_VEL_R_VEL", 3, 2), ("IB_VEL_R_X0", 4, 2), ("IB_VEL_R_X0_BANDS", 5, 2),
                           ("IB_VEL_RESULT_LEN", 5, 3)):
        assert re.search(rf"^#define {name} \({add} \+ {nbs} \* IB_LOSS_LEVEL_BUCKETS\)", text, flags=re.M), name
    here = os.path.dirname(hip.__file__)
    mk = open(os.path.join(here, "csrc", "Makefile")).read()
    assert "velocity.hip" in re.search(r"^SRCS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert re.search(r"^build/velocity\.o build_ab/velocity\.o: \.\./\.\./include/ib_hip_velocity\.h", mk, flags=re.M)
    assert mk.index("\nall:") < mk.index("ib_hip_velocity.h"), "the default goal stays `all`"
    src = open(os.path.join(here, "csrc", "velocity.hip")).read()
    assert "ib_hip_velocity.h" in src and "atomic" not in src.lower() and "fp contract(off)" in src
    for name in ("loss.hip", "loss_weight.hip", "predict.hip"):
        other = open(os.path.join(here, "csrc", name)).read()
        assert "ib_hip_velocity" not in other and "vel_loss" not in other, f"csrc/{name} stays as it was"
    for path in (hip.LIB_PATH, hip.AB_LIB_PATH):
        if not os.path.exists(path):
            pytest.fail(f"{path} is not built")
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        assert set(NAMES) <= {line.split()[-1] for line in out.splitlines() if line.strip()}, path
    root = os.path.dirname(here)
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "ib_hip_velocity.h" in open(os.path.join(root, doc)).read(), doc
    assert "velocity_decls" in open(os.path.join(root, "__graft_entry__.py")).read(), "build() checks the header's exports"


def test_workspace_and_chunk_queries():
    from inferbiomechanics_amd import hip
    FC = hip.vel_loss_frame_chunk()
    per = 4 * (4 + 2 * NB)                                     # bytes per workgroup
    assert hip.vel_loss_workspace_bytes(12800, 300, 50) == -(-(256 * -(-50 // FC) * 75) // 256) * per, "the headline shape"
    assert hip.vel_loss_workspace_bytes(4, 3, 2) == per, "one workgroup at least"
    assert hip.vel_loss_workspace_bytes(50 << 24, 300, 50) == 2048 * per, "capped: the kernel strides"
    assert hip.vel_loss_workspace_bytes(12, 43, 3) == hip.vel_loss_workspace_bytes(12, 44, 3), "4-column units at either width"
    for rows, cols, T in ((0, 44, 2), (12, 0, 2), (12, 44, 1), (12, 44, 0), (12, 44, 5), (-12, 44, 2)):
        assert hip.vel_loss_workspace_bytes(rows, cols, T) == 0, (rows, cols, T)


def test_host_argument_checks_of_the_live_library():
    """the checks that run before any launch, on the live library without a GPU: every refused call returns its code"""
    from inferbiomechanics_amd import hip
    lib = hip.lib()
    p = 4096                                     # never dereferenced: every call below is refused before a launch
    E_ARG = lib.ib_mse_loss_partial_cond(None, 44, None, None, 44, None, 0, 96, 44, 0, 0, None)
    E_WS = lib.ib_mse_loss_partial_cond(p, 44, p, None, 44, None, 0, 96, 44, 1, 0, None)
    assert E_ARG < 0 and E_WS < 0 and E_ARG != E_WS
    bytes_ = lib.ib_vel_loss_workspace(96, 44, 12)
    assert bytes_ > 0

    def partial(pred=p, x0=p, eps=p, t=p, wtab=p, utab=p, vtab=p, xtab=p, sa=p, sb=p, levels=50, rpw=12, wsp=p, wsb=bytes_,
                rows=96, cols=44, C=0, kind=2, dtype=0, ldp=44, dpred=None, ldd=0):
        return lib.ib_vel_loss_partial(pred, ldp, x0, eps, dpred, ldd, t, wtab, utab, vtab, xtab, sa, sb, levels, rpw, wsp, wsb,
                                       rows, cols, C, kind, dtype, None)
    for null in ("pred", "x0", "eps", "t", "wtab", "utab", "vtab", "xtab", "sa", "sb"):
        assert partial(**{null: None}) == E_ARG, null
    assert partial(kind=3) == E_ARG and partial(kind=-1) == E_ARG
    assert partial(rpw=1) == E_ARG, "T < 2: no frame difference"
    assert partial(rpw=7) == E_ARG and partial(rpw=0) == E_ARG and partial(rpw=-12) == E_ARG
    assert partial(levels=0) == E_ARG and partial(levels=-1) == E_ARG
    assert partial(C=44) == E_ARG and partial(C=45) == E_ARG and partial(C=-1) == E_ARG
    assert partial(rows=0) == E_ARG and partial(cols=0) == E_ARG and partial(ldp=43) == E_ARG
    assert partial(dpred=p, ldd=43) == E_ARG
    assert partial(wsp=None) == E_WS and partial(wsb=bytes_ - 1) == E_WS
    for kind in (0, 1, 2):
        assert partial(kind=kind, dtype=5) < 0 and partial(kind=kind, dtype=5) not in (E_ARG, E_WS)

    def final(wsp=p, wsb=bytes_, t=p, levels=50, res=p, rows=96, cols=44, C=0, rpw=12):
        return lib.ib_vel_loss_finalize(wsp, wsb, t, levels, res, None, rows, cols, C, rpw, None)
    for null in ("wsp", "t", "res"):
        assert final(**{null: None}) == E_ARG, null
    assert final(levels=0) == E_ARG and final(rpw=1) == E_ARG and final(rpw=7) == E_ARG and final(rows=0) == E_ARG
    assert final(cols=0) == E_ARG and final(C=44) == E_ARG and final(C=-1) == E_ARG
    assert final(wsb=bytes_ - 1) == E_WS


def test_binding_marshals_and_refuses(dry):
    lib = dry.lib()
    rows, D, T, n_levels = 24, 44, 12, 50
    pred_full, dfull = torch.zeros(rows, 48), torch.zeros(rows, 48)
    pred, x0, eps = pred_full[:, :D], torch.zeros(rows, D), torch.zeros(rows, D)
    t = torch.zeros(2, dtype=torch.int64)
    wtab, utab, vtab, xtab, sa, sb = (torch.ones(n_levels) for _ in range(6))
    ws = torch.zeros(dry.vel_loss_workspace_bytes(rows, D, T), dtype=torch.uint8)
    res, acc = torch.zeros(dry.VEL_RESULT_LEN), torch.zeros(dry.VEL_RESULT_LEN, dtype=torch.float64)
    go = lambda *a, **k: dry.vel_loss_partial(*a, **k)
    for kind, code in (("eps", 0), ("x0", 1), ("v", 2)):
        go(pred, x0, eps, ws, t, wtab, utab, vtab, xtab, sa, sb, T, kind, cond_cols=14, dpred=dfull[:, :D])
        assert lib.args[-1] == ("ib_vel_loss_partial",
                                (pred.data_ptr(), 48, x0.data_ptr(), eps.data_ptr(), dfull.data_ptr(), 48, t.data_ptr(),
                                 wtab.data_ptr(), utab.data_ptr(), vtab.data_ptr(), xtab.data_ptr(), sa.data_ptr(),
                                 sb.data_ptr(), n_levels, T, ws.data_ptr(), ws.numel(), rows, D, 14, code, 0, 0))
    go(pred, x0, eps, ws, t, wtab, utab, vtab, xtab, sa, sb, T, "v")
    assert lib.args[-1][1][4:6] == (None, 0) and lib.args[-1][1][19] == 0
    dry.vel_loss_finalize(ws, res, t, n_levels, rows, D, 14, T, accum=acc)
    assert lib.args[-1] == ("ib_vel_loss_finalize", (ws.data_ptr(), ws.numel(), t.data_ptr(), n_levels, res.data_ptr(),
                                                     acc.data_ptr(), rows, D, 14, T, 0))
    dry.vel_loss_finalize(ws, res, t, n_levels, rows, D, 0, T)
    assert lib.args[-1][1][5] is None
    n = len(lib.calls)
    base = (pred, x0, eps, ws, t, wtab, utab, vtab, xtab, sa, sb, T, "v")

    def swap(i, v):
        a = list(base)
        a[i] = v
        return lambda: go(*a)
    for bad in (swap(11, 7), swap(11, 1), swap(12, "noise"), swap(12, 2), swap(1, x0[:-1]), swap(2, eps.double()),
                swap(4, t[:1]), swap(4, t.int()), swap(6, utab[:-1]), swap(7, vtab.double()), swap(8, xtab[::2]),
                swap(9, sa[:-1]), swap(3, ws[:-1]), swap(0, pred.bfloat16()),
                lambda: go(*base, cond_cols=D), lambda: go(*base, dpred=torch.zeros(rows, D + 1)),
                lambda: dry.vel_loss_finalize(ws, res[:-1], t, n_levels, rows, D, 0, T),
                lambda: dry.vel_loss_finalize(ws, res, t, n_levels, rows, D, 0, 1),
                lambda: dry.vel_loss_finalize(ws, res, t[:1], n_levels, rows, D, 0, T),
                lambda: dry.vel_loss_finalize(ws, res, t, n_levels, rows, D, D, T),
                lambda: dry.vel_loss_finalize(ws, res, t, 0, rows, D, 0, T),
                lambda: dry.vel_loss_finalize(ws[:-1], res, t, n_levels, rows, D, 0, T),
                lambda: dry.vel_loss_finalize(ws, res, t, n_levels, rows, D, 0, T, accum=acc.float())):
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
        tr = HipTrainer(mk(), "diffusion", "adam", 1e-3, use_graph=False, cond_cols=C, velocity_loss=None)
        got, _ = _step_calls(dry, tr, batch)
        assert got == want, "name for name"
        assert not any(n.startswith("ib_vel_") for n in got)
        assert tr.velocity_loss is None and tr.vel_table is None and tr.vel_units_table is None
        assert tr.units_table is None and tr.level_table is None and tr.level_accum is None, "nothing is allocated"
        assert "velocity_loss" not in tr.optimizer_state_dict()
        assert not any(e[0] == "velocity_loss" for e in tr._sig)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("model", sorted(MODELS))
def test_on_replaces_exactly_the_loss_seam(dry, model, kind):
    from inferbiomechanics_amd.engine import HipTrainer
    from inferbiomechanics_amd.loss_weight import LossWeight
    from inferbiomechanics_amd.velocity_loss import VelocityLoss
    from inferbiomechanics_amd import prediction as P
    from inferbiomechanics_amd._tuning import tuning as TU
    mk, mb = MODELS[model]
    batch = mb()
    B, T, D = batch[0].shape
    swap = {n: ("ib_vel_loss_finalize" if "finalize" in n else "ib_vel_loss_partial") for n in SEAM}
    ab = _ab()
    for C in (0, 14):
        for lw in (None, LossWeight("min_snr", gamma=5.0)):
            if model == "chain_mlp":
                TU.no_chain = True                   # the yardstick of an MLP step with the term is the per-op step
            try:
                plain = HipTrainer(mk(), "diffusion", "adam", 1e-3, use_graph=False, cond_cols=C, loss_weight=lw, prediction=kind)
                want, _ = _step_calls(dry, plain, batch)
            finally:
                if model == "chain_mlp":
                    del TU.no_chain
            m = mk()
            vl = VelocityLoss(0.25, gamma=3.0)
            tr = HipTrainer(m, "diffusion", "adam", 1e-3, use_graph=False, cond_cols=C, loss_weight=lw, prediction=kind,
                            velocity_loss=vl)
            if model == "chain_mlp":
                assert tr.plan.chain_ok(D) and not tr.plan.chain_ok(D, 0, weighted=True)
            tabs = m.tables(torch.device("cpu"))
            vtab, xtab = vl.tables(ab, kind)
            assert np.array_equal(tr.vel_table.numpy(), vtab) and np.array_equal(tr.vel_units_table.numpy(), xtab)
            assert np.array_equal(tr.units_table.numpy(), P.eps_units(ab, kind))
            assert np.array_equal(tr.level_table.numpy(), np.ones(1000, dtype=np.float32) if lw is None else lw.weights(ab, kind))
            assert tr.level_accum.dtype == torch.float64 and tr.level_accum.numel() == dry.VEL_RESULT_LEN
            for _ in range(2):
                got, args = _step_calls(dry, tr, batch)
                assert got == [swap.get(n, n) for n in want], "every other launch is the step's without the term, in its order"
                assert got.count("ib_vel_loss_partial") == 1 == got.count("ib_vel_loss_finalize")
                assert not SEAM & set(got) and "ib_mlp_chain_train" not in got
                a = [x for n, x in args if n == "ib_vel_loss_partial"][0]
                f = [x for n, x in args if n == "ib_vel_loss_finalize"][0]
                q = [x for n, x in args if n.startswith("ib_q_sample")][0]
                assert a[2:4] == q[0:2], "x0 and eps are the buffers the forward noising read"
                assert a[7:13] == (tr.level_table.data_ptr(), tr.units_table.data_ptr(), tr.vel_table.data_ptr(),
                                   tr.vel_units_table.data_ptr(), tabs.sqrt_ab.data_ptr(), tabs.sqrt_1mab.data_ptr())
                assert a[13:15] == (1000, T) and a[17:21] == (B * T, D, C, P.KINDS.index(kind)) and a[4] is not None
                assert f[0:2] == a[15:17] and f[2] == a[6] and f[3] == 1000 and f[4] == tr.result.data_ptr()
                assert f[5] == tr.level_accum.data_ptr() and f[6:10] == (B * T, D, C, T)
            assert ("velocity_loss", 0.25) in tr._sig, "the capture signature includes the term"
            rep = tr.level_loss(reset=True)          # a dry run computes nothing
            assert rep["steps"] == 2 and rep["windows"] == [0] * NB and len(rep["bands"]) == NB
            assert rep["mse"] == rep["velocity"] == rep["x0_velocity"] == 0.0 and len(rep["x0_velocity_bands"]) == NB
            assert [b[:2] for b in rep["x0_velocity_bands"]] == [b[:2] for b in rep["bands"]]
            assert tr.level_loss()["steps"] == 0


def test_bad_values_are_refused():
    from inferbiomechanics_amd.engine import HipTrainer
    from inferbiomechanics_amd.velocity_loss import VelocityLoss
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    for bad in (0.5, "on", True):
        with pytest.raises(ValueError, match="velocity_loss must be None or a VelocityLoss"):
            HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, velocity_loss=bad)
    with pytest.raises(ValueError, match="50 entries"):
        HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, velocity_loss=VelocityLoss(1.0, table=np.ones(50)))
    with pytest.raises(ValueError, match="diffusion"):
        from inferbiomechanics_amd.models.FeedForwardRegressionBaseline import FeedForwardBaseline
        HipTrainer(FeedForwardBaseline(23, 2, 50, "all_frames", "sigmoid", 5, 10), "regression", "adam", 1e-3,
                   args=argparse.Namespace(predict_grf_components=list(range(6)), predict_cop_components=list(range(6)),
                                           predict_moment_components=list(range(6)), predict_wrench_components=list(range(12))),
                   velocity_loss=VelocityLoss(1.0))
    torch.manual_seed(0)
    one = DiffusionTransformer(8, 1, d_model=32, num_heads=2, dim_feedforward=32, num_layers=1)
    with pytest.raises(ValueError, match="at least 2 frames"):
        HipTrainer(one, "diffusion", "adam", 1e-3, use_graph=False, velocity_loss=VelocityLoss(1.0))


def test_a_window_of_one_frame_is_refused_at_the_first_batch(dry):
    from inferbiomechanics_amd.engine import HipTrainer
    from inferbiomechanics_amd.velocity_loss import VelocityLoss
    tr = HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, velocity_loss=VelocityLoss(1.0))
    lib = dry.lib()
    lib.calls.clear()
    with pytest.raises(ValueError, match="at least 2 frames"):
        tr.step(_batch(T=1))
    assert not any(n.startswith(("ib_vel_", "ib_mse_", "ib_q_sample")) for n in lib.calls), "refused before the step's launches"


def test_trainer_state_dict_round_trip_of_the_term(dry):
    from inferbiomechanics_amd.engine import HipTrainer
    from inferbiomechanics_amd.velocity_loss import VelocityLoss
    mk = lambda **kw: HipTrainer(_mlp(), "diffusion", "adam", 1e-3, use_graph=False, **kw)
    tr = mk(velocity_loss=VelocityLoss(0.5, gamma=4.0), prediction="v")
    for _ in range(3):
        tr.step(_batch())
    sd = tr.optimizer_state_dict()
    assert sd["velocity_loss"] == {"weight": 0.5, "gamma": 4.0, "table": None} and sd["step"] == 3
    again = mk(velocity_loss=VelocityLoss(0.5, gamma=4.0), prediction="v")
    again.load_optimizer_state_dict(sd)
    assert again.steps_done == 3
    for other, shown in ((VelocityLoss(0.25, gamma=4.0), r"velocity\(weight=0\.25, gamma=4\)"),
                         (VelocityLoss(0.5, gamma=5.0), r"velocity\(weight=0\.5, gamma=5\)"), (None, "none")):
        t2 = mk(velocity_loss=other, prediction="v")
        with pytest.raises(dry.HipError, match=rf"the checkpoint's velocity loss \(velocity\(weight=0\.5, gamma=4\)\) differs "
                                                 rf"from this trainer's \({shown}\)"):
            t2.load_optimizer_state_dict(sd)
        assert t2.steps_done == 0, "nothing was loaded"
    plain_sd = mk(prediction="v").optimizer_state_dict()
    assert "velocity_loss" not in plain_sd, "a trainer without the term writes what it wrote"
    with pytest.raises(dry.HipError, match=r"the checkpoint's velocity loss \(none\) differs from this trainer's"):
        again.load_optimizer_state_dict(plain_sd)
    tab = np.linspace(0.0, 1.0, 1000)
    with_table = mk(velocity_loss=VelocityLoss(0.5, table=tab))
    sd_t = with_table.optimizer_state_dict()
    assert sd_t["velocity_loss"]["table"] == tab.tolist()
    mk(velocity_loss=VelocityLoss(0.5, table=tab)).load_optimizer_state_dict(sd_t)
    with pytest.raises(dry.HipError, match="velocity loss"):
        mk(velocity_loss=VelocityLoss(0.5, table=tab[::-1].copy())).load_optimizer_state_dict(sd_t)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the command line
# ---------------------------------------------------------------------------------------------------------------------
def _train(*a):
    from inferbiomechanics_amd.cli.train import TrainCommand
    p = argparse.ArgumentParser()
    TrainCommand().register_subcommand(p.add_subparsers(dest="command"))
    return p.parse_args(["train"] + list(a))


DIFF = ("--model-type", "diffusion-mlp")


def test_cli_flag_default_and_refusals():
    from inferbiomechanics_amd.cli.train import resolve_velocity_loss
    from inferbiomechanics_amd.velocity_loss import VelocityLoss
    assert _train().velocity_loss == 0.0 and _train().velocity_gamma == 5.0
    assert resolve_velocity_loss(_train()) is None and resolve_velocity_loss(_train("--eager")) is None
    assert resolve_velocity_loss(_train("--model-type", "feedforward")) is None
    assert resolve_velocity_loss(_train(*DIFF, "--velocity-loss", "0.5")) == VelocityLoss(0.5, gamma=5.0)
    assert resolve_velocity_loss(_train(*DIFF, "--velocity-loss", "2", "--velocity-gamma", "inf")) == VelocityLoss(2.0, gamma=float("inf"))
    with pytest.raises(SystemExit, match="--velocity-loss needs the fused trainer"):
        resolve_velocity_loss(_train(*DIFF, "--velocity-loss", "0.5", "--eager"))
    with pytest.raises(SystemExit, match="diffusion model type"):
        resolve_velocity_loss(_train("--model-type", "feedforward", "--velocity-loss", "0.5"))
    for bad in (("--velocity-loss", "-1"), ("--velocity-loss", "nan"), ("--velocity-loss", "1", "--velocity-gamma", "0")):
        with pytest.raises(SystemExit, match="--velocity-loss / --velocity-gamma"):
            resolve_velocity_loss(_train(*DIFF, *bad))


BASE = ['--no-wandb', '--synthetic-windows', '24', '--batch-size', '8', '--data-loading-workers', '0', '--model-type',
        'diffusion-mlp', '--feat-dim', '24', '--hidden-dims', '32', '32', '--stride', '1', '--history-len', '6', '--seed', '7']


def test_train_with_the_term_in_dry_run(dry, tmp_path, capsys):
    """a run with the term from start to resume: refused with --eager before anything is written, every step the new loss
    seam, the report lines, the trainer keys in the checkpoint only when on, a resume with another value refused"""
    from inferbiomechanics_amd.cli.train import TrainCommand
    ck = str(tmp_path / "ck")
    common = BASE + ['--checkpoint-dir', ck, '--window-cache', 'hbm', '--report-every', '2']
    with pytest.raises(SystemExit, match="--velocity-loss needs the fused trainer"):
        TrainCommand().run(_train(*common, '--epochs', '1', '--velocity-loss', '0.5', '--eager'))
    assert not os.path.exists(ck)
    lib = dry.lib()
    lib.calls.clear()
    assert TrainCommand().run(_train(*common, '--epochs', '1', '--velocity-loss', '0.5'))
    assert lib.calls.count("ib_vel_loss_partial") == 3 == lib.calls.count("ib_vel_loss_finalize")
    assert not SEAM & set(lib.calls)
    out = capsys.readouterr().out
    assert "Velocity loss on the predicted x0: velocity(weight=0.5, gamma=5)" in out
    assert "velocity term" in out and "x0 velocity error per noise-level band" in out
    sub = os.path.join(ck, "diffusion-mlp")
    files = sorted(f for f in os.listdir(sub) if f.endswith(".pt"))
    payload = torch.load(os.path.join(sub, files[-1]), map_location="cpu")
    assert payload["optimizer_state_dict"]["velocity_loss"] == {"weight": 0.5, "gamma": 5.0, "table": None}
    assert "velocity_loss" not in payload, "the checkpoint format gains only the trainer keys"
    for other in ((), ('--velocity-loss', '0.25'), ('--velocity-loss', '0.5', '--velocity-gamma', '2')):
        with pytest.raises(SystemExit, match="Resume with the same --velocity-loss"):
            TrainCommand().run(_train(*common, '--epochs', '2', *other))
    lib.calls.clear()
    assert TrainCommand().run(_train(*common, '--epochs', '2', '--velocity-loss', '0.5'))
    assert lib.calls.count("ib_vel_loss_partial") == 3, "one more epoch"
    ck2 = str(tmp_path / "ck2")
    assert TrainCommand().run(_train(*BASE, '--checkpoint-dir', ck2, '--window-cache', 'hbm', '--epochs', '1'))
    sub2 = os.path.join(ck2, "diffusion-mlp")
    files = sorted(f for f in os.listdir(sub2) if f.endswith(".pt"))
    payload = torch.load(os.path.join(sub2, files[-1]), map_location="cpu")
    assert "velocity_loss" not in payload["optimizer_state_dict"]


# ---------------------------------------------------------------------------------------------------------------------
# 5. the kernels' registers
# ---------------------------------------------------------------------------------------------------------------------
def test_velocity_kernels_use_no_scratch_and_no_lds_beyond_the_reduction():
    """no form of the new kernels spills or touches scratch; the partial kernel's LDS is its 4 x (4 + 2 NB) reduction scratch
    (compile only)"""
    from tools import kernel_resources as kr
    if kr.hipcc() is None:
        pytest.skip("hipcc not installed")
    rows = {k["kernel"]: k for k in kr.resources("velocity.hip")}
    assert len(rows) == 12 + 1, sorted(rows)
    for name, k in rows.items():
        assert name.startswith("vel_partial_kernel<") or name == "vel_final_kernel", name
        assert not k["scratch"] and not k["vgpr_spill"] and not k["sgpr_spill"], k
        if name != "vel_final_kernel":
            assert k["lds"] == 4 * (4 + 2 * NB) * 4, k
            assert k["occupancy"] >= 2, k
