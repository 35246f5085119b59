"""Host side of solver 'dpmpp2m_sde' (no GPU): the float64 tables against their identities and against the restatement of
tests/sde_restatement.py, the fourth header and its table, the dry-run launches of the sampler classes, the predictor and
the two commands, the table-sharing rule of DiffusionTables.serves, the binding's refusals and the kernel's registers."""
import argparse
import os
import subprocess

import pytest
import torch

from tests import sde_restatement as RS

NAME = "ib_sde_dpmpp_step"
GRIDS = [("time", 10), ("time", 100), ("logsnr", 10), ("logsnr", 20), ("logsnr", 50)]
# final variance / s2 of the solver on x0 ~ N(0, s2), log-SNR grid: (steps, eta, s2) -> (this solver, the first-order eta loop)
FIGURES = {(10, 0.5, 0.25): (1.06184, 0.55491), (10, 0.5, 4.0): (1.09462, 0.55506), (10, 1.0, 0.25): (1.04219, 0.41110),
           (10, 1.0, 4.0): (1.09077, 0.41244), (20, 0.5, 0.25): (1.05035, 0.74502), (20, 0.5, 4.0): (1.04987, 0.74515),
           (20, 1.0, 0.25): (1.07002, 0.62769), (20, 1.0, 4.0): (1.06907, 0.62771)}


@pytest.fixture()
def dry():
    from inferbiomechanics_amd import hip
    hip.set_dry_run(True)
    yield hip
    hip.set_dry_run(False)


def _tr(dt=torch.float32, D=44, T=8):
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    return DiffusionTransformer(D, T, d_model=32, num_heads=4, dim_feedforward=64, num_layers=1, temb_dim=16, temb_hidden=24,
                                compute_dtype=dt)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the tables
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spacing,S", GRIDS)
def test_table_identities(spacing, S):
    from inferbiomechanics_amd.diffusion import schedule as sch
    assert "dpmpp2m_sde" in sch.SOLVERS
    zero = sch.sde_dpmpp_coefficients(1000, S, 0.0, spacing)
    assert zero.dtype == torch.float64 and tuple(zero.shape) == (S, 6)
    assert torch.equal(zero[:, :5], sch.dpmpp_coefficients(1000, S, spacing)) and not zero[:, 5].any()   # bit for bit
    one = sch.sde_dpmpp_coefficients(1000, S, 1.0, spacing)
    first = sch.ddim_coefficients_eta(1000, S, 1.0, spacing)
    assert float((one[0, [0, 1, 5]] - first[0]).abs().max()) <= 1e-12
    rq1 = sch.sde_observation_noise_coefficients(1000, S, 1.0, spacing)
    assert tuple(rq1.shape) == (S, 2)
    assert float((rq1 - sch.observation_noise_coefficients(1000, S, 1.0, spacing)).abs().max()) <= 1e-12
    last = sch.ddim_coefficients(1000, S, spacing)[-1]
    for eta in (0.3, 0.5, 1.0):
        c = sch.sde_dpmpp_coefficients(1000, S, eta, spacing)
        rq = sch.sde_observation_noise_coefficients(1000, S, eta, spacing)
        assert float(((rq[:-1] ** 2).sum(1) - 1).abs().max()) <= 1e-12
        assert rq[-1].tolist() == [0.0, 0.0]
        assert float((c[-1, :2] - last).abs().max()) <= 1e-12 and float(c[-1, 2]) == 0.0 == float(c[-1, 5])
        assert float(c[0, 2]) == 0.0 and bool((c[1:-1, 2] != 0).all()) and bool((c[:-1, 5] > 0).all())
        assert torch.equal(c[:, 3:5], zero[:, 3:5])                    # the history does not depend on eta
    if S > 1:                                                          # at eta < 1 the two (r, q) tables are not the same
        a, b = sch.sde_observation_noise_coefficients(1000, S, 0.5, spacing), sch.observation_noise_coefficients(1000, S, 0.5, spacing)
        assert float((a - b).abs().max()) > 1e-3
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="eta"):
            sch.sde_dpmpp_coefficients(1000, S, bad, spacing)
        with pytest.raises(ValueError, match="eta"):
            sch.sde_observation_noise_coefficients(1000, S, bad, spacing)


@pytest.mark.parametrize("spacing,S", GRIDS)
@pytest.mark.parametrize("eta", [0.5, 1.0])
def test_tables_equal_the_restatement(spacing, S, eta):
    from inferbiomechanics_amd.diffusion import schedule as sch
    ab = RS.alpha_bars()
    ts = sch.sample_timesteps(1000, S, spacing).tolist()
    coef, rq = RS.rows64(ab, ts, eta)
    got, got_rq = sch.sde_dpmpp_coefficients(1000, S, eta, spacing), sch.sde_observation_noise_coefficients(1000, S, eta, spacing)
    want, want_rq = torch.tensor(coef, dtype=torch.float64), torch.tensor(rq, dtype=torch.float64)
    # both are float64 evaluations of the same closed forms from alpha_bar values that agree to an ulp or two; the
    # lambda differences lose at most ~1e-13 relative on the fine 'time' grid, and every entry is O(1) .. O(30)
    assert float(((got - want).abs() / (1 + want.abs())).max()) <= 1e-10
    assert float((got_rq - want_rq).abs().max()) <= 1e-10


@pytest.mark.parametrize("key", sorted(FIGURES))
def test_covariance_recursion_reproduces_the_recorded_figures(key):
    """x0 ~ N(0, s2) with the analytic optimal denoiser eps = k x: the exact covariance recursion of (x, h) over the table
    gives final variance / s2; the recorded figures to 1e-4, from the schedule's table and from the restatement's"""
    from inferbiomechanics_amd.diffusion import schedule as sch
    S, eta, s2 = key
    ab = RS.alpha_bars()
    ts = sch.sample_timesteps(1000, S, "logsnr").tolist()
    ks = RS.gains(ab, ts, s2)
    want, want_first = FIGURES[key]
    mine = RS.final_variance(RS.rows64(ab, ts, eta)[0], ks) / s2
    table = RS.final_variance(sch.sde_dpmpp_coefficients(1000, S, eta, "logsnr").tolist(), ks) / s2
    first = RS.first_order_ratio(ab, ts, eta, s2)
    print(f"S={S} eta={eta} s2={s2}: restatement {mine:.5f}, schedule.py {table:.5f} (recorded {want}); first order {first:.5f} "
          f"(recorded {want_first})")
    assert abs(mine - want) <= 1e-4 and abs(table - want) <= 1e-4
    assert abs(first - want_first) <= 1e-4
    assert abs(table - 1) < abs(first - 1)


def test_time_grid_at_twenty_steps_is_poor():
    """why the docs send the solver to --sample-spacing logsnr: 2.26 at s2 = 0.25 on the 'time' grid"""
    from inferbiomechanics_amd.diffusion import schedule as sch
    ab = RS.alpha_bars()
    ts = sch.sample_timesteps(1000, 20, "time").tolist()
    ratio = RS.final_variance(sch.sde_dpmpp_coefficients(1000, 20, 1.0, "time").tolist(), RS.gains(ab, ts, 0.25)) / 0.25
    assert abs(ratio - 2.26) <= 5e-3


# ---------------------------------------------------------------------------------------------------------------------
# 2. the header
# ---------------------------------------------------------------------------------------------------------------------
def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_fourth_header_has_its_own_table_and_both_builds_export_it():
    from inferbiomechanics_amd import hip
    assert os.path.basename(hip.SDE_HEADER_PATH) == "ib_hip_sde.h" and os.path.exists(hip.SDE_HEADER_PATH)
    assert hip.sde_symbols() == [NAME] and list(hip._SDE_SIGS) == [NAME]
    assert NAME not in hip._SIGS and NAME not in hip._STITCH_SIGS and NAME not in hip._HEAD_SIGS
    assert len(hip._SIGS) == 127
    assert hip.stitch_symbols() == ["ib_stitch_ddim_step", "ib_stitch_ddim_step_noise", "ib_stitch_dpmpp_step"]
    res, args = hip._sig(NAME)
    assert res is hip._c.c_int and len(args) == 27 and args[-1] is hip._vp and args[18] is hip._c.c_uint64
    assert args[10] is hip._i64 and args[11] is hip._i32 and all(a is hip._i64 for a in args[19:25]) and args[25] is hip._c.c_int
    assert hip._is_launch(NAME)
    for path in (hip.LIB_PATH, hip.AB_LIB_PATH):
        if not os.path.exists(path):
            pytest.fail(f"{path} is not built")
        assert NAME in _exports(path), path
    fn = getattr(hip.lib(), NAME)
    assert fn.restype is hip._c.c_int and list(fn.argtypes) == args


def test_a_name_of_another_header_declared_again_in_the_fourth_is_refused():
    import importlib.util
    import io

    from inferbiomechanics_amd import hip
    text = open(hip.SDE_HEADER_PATH).read()

    def load(extra):
        spec = importlib.util.spec_from_file_location("inferbiomechanics_amd._hip_sde_twice", hip.__file__)
        mod = importlib.util.module_from_spec(spec)
        real_open = open

        def fake_open(path, *a, **kw):
            f = real_open(path, *a, **kw)
            if os.path.abspath(str(path)) != os.path.abspath(hip.SDE_HEADER_PATH):
                return f
            f.close()
            return io.StringIO(text.replace("#ifdef __cplusplus\n}", extra + "\n#ifdef __cplusplus\n}"))

        mod.__dict__["open"] = fake_open
        spec.loader.exec_module(mod)
        return mod

    assert load("").sde_symbols() == [NAME]
    with pytest.raises(RuntimeError, match="declared in two headers.*ib_stitch_dpmpp_step"):
        load("int ib_stitch_dpmpp_step(void* x, ib_stream_t stream);")
    with pytest.raises(RuntimeError, match=f"{NAME} is declared twice"):
        load(f"int {NAME}(void* x, ib_stream_t stream);")


# ---------------------------------------------------------------------------------------------------------------------
# 3. dry-run launches
# ---------------------------------------------------------------------------------------------------------------------
OTHERS = ("ib_stitch_ddim_step", "ib_stitch_dpmpp_step", "ib_stitch_ddim_step_noise", "ib_ddim_step", "ib_ddim_cond_step",
          "ib_ddim_step_noise", "ib_ddim_cond_step_noise", "ib_dpmpp_step", "ib_dpmpp_cond_step")


@pytest.mark.parametrize("cond", [False, True])
def test_per_window_samplers_issue_one_launch_per_step(dry, cond):
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion import ConditionalDDIMSampler, DDIMSampler
    B, D, T, S = 3, 44, 8, 5
    m = _tr(torch.bfloat16)
    cls = ConditionalDDIMSampler if cond else DDIMSampler
    s = cls(m, S, eta=0.5, seed=(7 << 32) + 3, solver="dpmpp2m_sde", spacing="logsnr")
    mask = torch.zeros(T, D, dtype=torch.bool)
    mask[::2, :14] = True
    dry.lib().calls.clear()
    dry.lib().args.clear()
    out = s.sample(torch.randn(B, T, D), *((torch.randn(B, T, D), mask) if cond else ()), window_ids=[5, (1 << 32) - 1, 0])
    assert out.shape == (B, T, D)
    calls = dry.lib().calls
    assert calls.count(NAME) == S and calls.count("ib_ddim_cond_init") == (1 if cond else 0)
    assert not [o for o in OTHERS if o in calls]
    b, tabs = s._bufs, m.tables(torch.device("cpu"))
    Dp = b["x"].shape[-1]
    assert Dp % 8 == 0 and Dp >= D and tuple(b["hist"].shape) == (B, T, Dp) and b["hist"].dtype == torch.float32
    start, cover, wn = b["one_window"]
    assert start.tolist() == [0] and cover.tolist() == [[0, 1]] * T and wn[:, 0].tolist() == [1.0] * T and not wn[:, 1:].any()
    p = lambda t: None if t is None else t.data_ptr()
    cnd = [p(b["x0"]), p(b["z"]), p(b["mask"])] if cond else [None, None, None]
    want = [p(b["x"]), p(b["eps"]), p(b["hist"])] + cnd + \
           [p(tabs.sde_coef), p(tabs.obs_coef) if cond else None, p(tabs.sde_obs_noise_coef) if cond else None,
            p(tabs.ddim_t), S, 0, p(b["ctr"]), p(b["t"]), p(start), p(cover), p(wn), p(b["win"]),
            (7 << 32) + 3, B, 1, T, T, D, Dp, hip.BF16, 0]
    got = [a for n, a in dry.lib().args if n == NAME]
    assert len(got) == S
    for a in got:
        assert list(a) == want
    assert b["win"].tolist() == [5, (1 << 32) - 1, 0] and b["t"].numel() == B
    assert tuple(tabs.sde_coef.shape) == (S, 6) and tuple(tabs.sde_obs_noise_coef.shape) == (S, 2)
    assert tabs.ddim_coef_eta is None and tabs.obs_noise_coef is None, "the first-order eta tables are another loop's"
    # the signature of the captured step holds the new tables' pointers
    assert p(tabs.sde_coef) in s._sig and p(tabs.sde_obs_noise_coef) in s._sig


@pytest.mark.parametrize("cond", [False, True])
def test_stitched_sampler_issues_one_launch_per_step(dry, cond):
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion import StochasticStitchedSampler
    N, F, D, T, S = 2, 17, 44, 8, 5
    m = _tr(torch.bfloat16)
    s = StochasticStitchedSampler(m, S, eta=0.5, hop=3, seed=11, spacing="logsnr", solver="dpmpp2m_sde")
    assert s.solver == "dpmpp2m_sde" and s.eta == 0.5
    cols = torch.zeros(D, dtype=torch.bool)
    cols[:14] = True
    dry.lib().calls.clear()
    dry.lib().args.clear()
    out = s.sample(torch.randn(N, F, D), *((torch.randn(N, F, D), cols) if cond else ()), trial_ids=[5, (1 << 32) - 1])
    assert out.shape == (N, F, D)
    calls = dry.lib().calls
    assert calls.count(NAME) == S and not [o for o in OTHERS if o in calls]
    b, lay, tabs = s._bufs, s.layout, m.tables(torch.device("cpu"))
    Dp, W = b["x"].shape[-1], lay["W"]
    assert W == 4 and tuple(b["hist"].shape) == (N * W, T, Dp) and b["hist"].dtype == torch.float32
    p = lambda t: None if t is None else t.data_ptr()
    cnd = [p(b["x0"]), p(b["z"]), p(b["mask"])] if cond else [None, None, None]
    want = [p(b["x"]), p(b["eps"]), p(b["hist"])] + cnd + \
           [p(tabs.sde_coef), p(tabs.obs_coef) if cond else None, p(tabs.sde_obs_noise_coef) if cond else None,
            p(tabs.ddim_t), S, 0, p(b["ctr"]), p(b["t"]), p(lay["start"]), p(lay["cover"]), p(lay["wn"]), p(b["win"]),
            11, N, W, T, F, D, Dp, hip.BF16, 0]
    for a in [a for n, a in dry.lib().args if n == NAME]:
        assert list(a) == want
    assert b["win"].tolist() == [5, (1 << 32) - 1]


def test_eta_zero_is_the_call_list_of_dpmpp2m(dry):
    from inferbiomechanics_amd.diffusion import ConditionalDDIMSampler, DDIMSampler, StitchedDDIMSampler, StochasticStitchedSampler
    m = _tr(torch.bfloat16)
    D, T, S = 44, 8, 5
    mask = torch.zeros(T, D, dtype=torch.bool)
    mask[:, :14] = True
    cols = mask[0].clone()
    xw, ow, xt, ot = torch.randn(3, T, D), torch.randn(3, T, D), torch.randn(2, 17, D), torch.randn(2, 17, D)
    runs = ((lambda sv: DDIMSampler(m, S, solver=sv, spacing="logsnr").sample(xw), "dpmpp2m"),
            (lambda sv: ConditionalDDIMSampler(m, S, solver=sv, spacing="logsnr").sample(xw, ow, mask), "dpmpp2m"),
            (lambda sv: StitchedDDIMSampler(m, S, hop=3, solver=sv, spacing="logsnr").sample(xt, ot, cols), "dpmpp2m"),
            (lambda sv: (StochasticStitchedSampler(m, S, eta=0.0, hop=3, spacing="logsnr", solver=sv) if sv == "dpmpp2m_sde"
                         else StitchedDDIMSampler(m, S, hop=3, solver=sv, spacing="logsnr")).sample(xt, ot, cols), "dpmpp2m"))
    for run, base in runs:
        lists = []
        for sv in (base, "dpmpp2m_sde"):
            dry.lib().calls.clear()
            run(sv)
            lists.append(list(dry.lib().calls))
        assert lists[0] == lists[1] and NAME not in lists[1] and len([c for c in lists[1] if "dpmpp" in c]) == S


def test_sampler_refusals(dry):
    from inferbiomechanics_amd.diffusion import ConditionalDDIMSampler, DDIMSampler, StochasticStitchedSampler
    m = _tr()
    for cls in (DDIMSampler, ConditionalDDIMSampler):
        for eta in (-0.1, 1.5):
            with pytest.raises(ValueError, match="eta"):
                cls(m, 5, eta=eta, solver="dpmpp2m_sde")
        with pytest.raises(ValueError, match="deterministic"):          # 'dpmpp2m' stays refused
            cls(m, 5, eta=0.5, solver="dpmpp2m")
        assert cls(m, 5, eta=1.0, solver="dpmpp2m_sde").solver == "dpmpp2m_sde"
    with pytest.raises(ValueError, match="StitchedDDIMSampler"):
        StochasticStitchedSampler(m, 5, solver="dpmpp2m")
    with pytest.raises(ValueError, match="solver"):
        StochasticStitchedSampler(m, 5, solver="heun")
    with pytest.raises(TypeError):
        StochasticStitchedSampler(m, 5, sovler="ddim")
    assert StochasticStitchedSampler(m, 5).solver == "ddim" and StochasticStitchedSampler(m, 5, solver="ddim").solver == "ddim"
    with pytest.raises(ValueError, match="eta"):
        StochasticStitchedSampler(m, 5, eta=1.5, solver="dpmpp2m_sde")


def test_tables_are_never_served_to_the_other_solvers_loop():
    from inferbiomechanics_amd.diffusion.schedule import DiffusionTables
    tabs = DiffusionTables(torch.device("cpu"), num_sample_steps=10)
    with pytest.raises(ValueError, match="deterministic"):
        tabs.set_sampler(10, 0.5, "dpmpp2m", "logsnr")
    tabs.set_sampler(10, 0.5, "dpmpp2m_sde", "logsnr")
    assert tabs.sde_coef is not None and tabs.sde_obs_noise_coef is not None and tabs.dpmpp_coef is not None
    assert tabs.ddim_coef_eta is None and tabs.obs_noise_coef is None
    assert tabs.sde_coef.dtype == torch.float32 and tuple(tabs.sde_coef.shape) == (10, 6)
    assert tabs.serves(10, 0.5, "dpmpp2m_sde", "logsnr")
    assert not tabs.serves(10, 0.5, "ddim", "logsnr"), "a first-order eta loop must not read the new solver's tables"
    assert not tabs.serves(10, 0.7, "dpmpp2m_sde", "logsnr") and not tabs.serves(10, 0.5, "dpmpp2m_sde", "time")
    assert tabs.serves(10, 0.0, "dpmpp2m", "logsnr") and tabs.serves(10, 0.0, "dpmpp2m_sde", "logsnr")
    assert tabs.serves(10, 0.0, "ddim", "logsnr")
    tabs.set_sampler(10, 0.5, "ddim", "logsnr")
    assert tabs.ddim_coef_eta is not None and tabs.obs_noise_coef is not None and tabs.sde_coef is None
    assert tabs.sde_obs_noise_coef is None
    assert tabs.serves(10, 0.5, "ddim", "logsnr")
    assert not tabs.serves(10, 0.5, "dpmpp2m_sde", "logsnr"), "the new solver's loop must not read the first-order tables"
    tabs.set_sampler(10, 0.0, "dpmpp2m_sde", "logsnr")                 # eta = 0: the 'dpmpp2m' table and no noise table
    assert tabs.dpmpp_coef is not None and tabs.sde_coef is None and tabs.serves(10, 0.0, "dpmpp2m", "logsnr")
    assert not tabs.serves(10, 0.5, "dpmpp2m_sde", "logsnr")


def test_alternating_samplers_on_one_model_read_their_own_tables(dry):
    from inferbiomechanics_amd.diffusion import ConditionalDDIMSampler
    m = _tr(torch.bfloat16)
    D, T, S = 44, 8, 5
    mask = torch.zeros(T, D, dtype=torch.bool)
    mask[:, :14] = True
    first = ConditionalDDIMSampler(m, S, eta=0.5, spacing="logsnr")
    new = ConditionalDDIMSampler(m, S, eta=0.5, solver="dpmpp2m_sde", spacing="logsnr")
    x, o = torch.randn(2, T, D), torch.randn(2, T, D)
    tabs = m.tables(torch.device("cpu"))
    for _ in range(2):
        for s, name, at in ((first, "ib_ddim_cond_step_noise", 7), (new, NAME, 8)):
            dry.lib().args.clear()
            s.sample(x, o, mask)
            got = [a for n, a in dry.lib().args if n == name]
            assert len(got) == S
            table = tabs.obs_noise_coef if s is first else tabs.sde_obs_noise_coef
            assert table is not None and all(a[at] == table.data_ptr() for a in got)
            assert (tabs.sde_obs_noise_coef is None) == (s is first) and (tabs.obs_noise_coef is None) == (s is new)


# ---------------------------------------------------------------------------------------------------------------------
# 4. predictor and commands
# ---------------------------------------------------------------------------------------------------------------------
def _trials(n):
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import SyntheticWindowDataset
    ds = SyntheticWindowDataset(4, 50, 5)                              # windows of 10 frames
    items = [ds[i] for i in range(4)]
    return {k: torch.cat([it[0][k] for it in items[:2]]).unsqueeze(0).repeat(n, 1, 1) for k in items[0][0]}   # [n, 20, c]


def test_predict_trial_ensemble_runs_the_new_solver(dry):
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import LOSS_KEY_ORDER, LOSS_KEY_WIDTHS
    from inferbiomechanics_amd.diffusion import StochasticStitchedSampler
    from inferbiomechanics_amd.models.DiffusionLabelPredictor import DiffusionLabelPredictor
    inputs = _trials(2)
    pred = DiffusionLabelPredictor(_tr(D=177, T=10), 5, eta=0.5, num_samples=3, seed=11, solver="dpmpp2m_sde", spacing="logsnr")
    assert pred.sampler.solver == "dpmpp2m_sde"
    dry.lib().calls.clear()
    dry.lib().args.clear()
    out = pred.predict_trial_ensemble(inputs, hop=4, blend="uniform", draw=1)
    for k, w in zip(LOSS_KEY_ORDER, LOSS_KEY_WIDTHS):
        assert out[k].shape == (2, 20, w) and pred.last_std[k].shape == (2, 20, w)
    calls = dry.lib().calls
    assert calls.count(NAME) == 5 and calls.count("ib_ensemble_stats") == 1 and "ib_stitch_ddim_step_noise" not in calls
    _, sampler, _ = pred._trial_ens
    assert isinstance(sampler, StochasticStitchedSampler) and sampler.solver == "dpmpp2m_sde" and sampler.spacing == "logsnr"
    assert sampler._bufs["win"].tolist() == [3, 4, 5, 6, 7, 8]
    a = next(a for n, a in dry.lib().args if n == NAME)
    assert a[19] == 6 and a[22] == 20                                  # N = 2 trials x 3 members, F = 20
    dry.lib().calls.clear()                                            # the per-window ensemble of the same predictor
    pred({k: v[:, :10] for k, v in inputs.items()})
    assert dry.lib().calls.count(NAME) == 5 and "ib_ddim_cond_step_noise" not in dry.lib().calls
    with pytest.raises(ValueError, match="deterministic"):
        DiffusionLabelPredictor(_tr(D=177, T=10), 5, num_samples=2, solver="dpmpp2m").predict_trial_ensemble(inputs)


def test_analyze_runs_the_new_solver(dry, tmp_path, capsys):
    from inferbiomechanics_amd.cli.analyze import AnalyzeCommand
    from inferbiomechanics_amd.main import main
    p = argparse.ArgumentParser()
    AnalyzeCommand().register_subcommand(p.add_subparsers(dest="command"))
    a = p.parse_args(['analyze', '--model-type', 'diffusion-mlp', '--sampler', 'dpmpp2m_sde', '--sample-spacing', 'logsnr'])
    assert (a.sampler, a.sample_spacing) == ('dpmpp2m_sde', 'logsnr')
    ck = str(tmp_path / "ck")
    common = ['--no-wandb', '--checkpoint-dir', ck, '--data-loading-workers', '0', '--model-type', 'diffusion-mlp',
              '--hidden-dims', '32', '32']
    assert main(['train', '--synthetic-windows', '8', '--feat-dim', '177', '--epochs', '1', '--max-steps', '1',
                 '--batch-size', '4'] + common)
    analyze = ['analyze', '--synthetic-windows', '5', '--sample-steps', '4', '--sample-batch', '2', '--sample-spacing',
               'logsnr'] + common
    batches = 2 * 3                                                    # dev and train, 5 windows in calls of 2
    capsys.readouterr()
    dry.lib().calls.clear()
    assert main(analyze + ['--sampler', 'dpmpp2m_sde', '--sample-eta', '0.5', '--num-samples', '3'])
    calls = dry.lib().calls
    assert calls.count(NAME) == 4 * batches and calls.count("ib_ensemble_stats") == batches
    assert not [c for c in calls if c in OTHERS]
    assert len([l for l in capsys.readouterr().out.splitlines() if l.startswith('Ensemble spread')]) == 2
    dry.lib().calls.clear()
    assert main(analyze + ['--sampler', 'dpmpp2m_sde'])                # eta = 0: the 'dpmpp2m' launches
    assert dry.lib().calls.count("ib_dpmpp_cond_step") == 4 * batches and NAME not in dry.lib().calls
    with pytest.raises(SystemExit, match="dpmpp2m is deterministic"):
        main(analyze + ['--sampler', 'dpmpp2m', '--sample-eta', '0.5'])


def test_visualize_runs_the_new_solver(dry, tmp_path, capsys):
    from inferbiomechanics_amd.cli.visualize import VisualizeCommand
    from inferbiomechanics_amd.main import main
    p = argparse.ArgumentParser()
    VisualizeCommand().register_subcommand(p.add_subparsers(dest="command"))
    assert p.parse_args(["visualize"]).sample_spacing == "time"
    tr = ["visualize", "--synthetic-windows", "60", "--checkpoint-dir", str(tmp_path / "ck"), "--sample-steps", "4",
          "--model-type", "diffusion-transformer", "--trial-frames", "25", "--trial-hop", "4", "--num-frames", "2"]
    capsys.readouterr()
    dry.lib().calls.clear()
    assert main(tr + ["--sampler", "dpmpp2m_sde", "--sample-spacing", "logsnr", "--sample-eta", "0.5", "--num-samples", "2"])
    out = capsys.readouterr().out.splitlines()
    calls = dry.lib().calls
    assert calls.count(NAME) == 2 * 4 + 2 * 4                          # the stitched and the per-window loop of each trial
    assert not [c for c in calls if c in OTHERS] and calls.count("ib_ensemble_stats") == 2 * 2
    assert sum(1 for l in out if "mean std over 2 samples" in l) == 2 * 4
    for bad in (["--sampler", "dpmpp2m", "--sample-eta", "0.5"], ["--sampler", "dpmpp2m", "--num-samples", "2"]):
        with pytest.raises(SystemExit, match="dpmpp2m is deterministic"):
            main(tr + bad)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the binding's refusals and the kernel's registers
# ---------------------------------------------------------------------------------------------------------------------
def test_binding_refusals(dry):
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion.schedule import stitch_layout
    N, W, T, F, D, S = 2, 4, 8, 17, 16, 5
    start, cover, wn, _ = stitch_layout(F, T, 3, "ramp")
    x, eps, hist = torch.zeros(N, W, T, D), torch.zeros(N, W, T, D), torch.zeros(N, W, T, D)
    coef, ts, ids = torch.zeros(S, 6), torch.zeros(S, dtype=torch.int64), torch.zeros(N, dtype=torch.int64)
    go = lambda **kw: hip.sde_dpmpp_step(*[kw.get(k, v) for k, v in (
        ("x", x), ("eps", eps), ("hist", hist), ("x0", None), ("z", None), ("mask", None), ("coef", coef), ("obs_coef", None),
        ("obs_noise_coef", None), ("timesteps", ts), ("start", start), ("cover", cover), ("wn", wn), ("trial_ids", ids),
        ("seed", 1))])
    dry.lib().calls.clear()
    go()
    assert dry.lib().calls == [NAME]
    for bad in (torch.zeros(S, 5), torch.zeros(S, 3)):                 # the tables of the two kernels it joins
        with pytest.raises(hip.HipError, match="coef"):
            go(coef=bad)
    with pytest.raises(hip.HipError, match="hist"):
        go(hist=hist.to(torch.bfloat16))
    with pytest.raises(hip.HipError, match="hist"):
        go(x=x.to(torch.bfloat16), eps=eps.to(torch.bfloat16), hist=hist.to(torch.bfloat16))
    with pytest.raises(hip.HipError, match="hist"):
        go(hist=torch.zeros(N * W, T, D))
    with pytest.raises(hip.HipError, match="trial_ids"):
        go(trial_ids=torch.zeros(N * W, dtype=torch.int64))
    with pytest.raises(hip.HipError):
        go(trial_ids=torch.zeros(N, dtype=torch.int32))
    with pytest.raises(hip.HipError, match="together"):
        go(obs_noise_coef=torch.zeros(S, 2))
    masked = dict(x0=x.clone(), z=x.clone(), mask=torch.zeros(T, D, dtype=torch.uint8), obs_coef=torch.zeros(S + 1, 2))
    with pytest.raises(hip.HipError, match="together"):
        go(**masked)
    for name in ("x0", "z", "mask"):
        with pytest.raises(hip.HipError, match="together"):
            go(**{k: v for k, v in masked.items() if k != name}, obs_noise_coef=torch.zeros(S, 2))
    with pytest.raises(hip.HipError, match="obs_noise_coef"):
        go(**masked, obs_noise_coef=torch.zeros(S + 1, 2))
    go(**masked, obs_noise_coef=torch.zeros(S, 2))
    assert dry.lib().calls == [NAME, NAME], "a refused call reaches the library"


def test_kernel_resources_no_scratch_no_spill():
    import re

    from tools import kernel_resources as kr
    if kr.hipcc() is None:
        pytest.skip("hipcc not installed")
    rows = kr.resources("sde.hip")
    kernels = [r for r in rows if "stitch_step_kernel" in r["kernel"]]
    # stitch_step.h's template with MODE 3: fp32 / bf16 x {8-wide: cond x whole blocks, element-wise: cond}
    assert len(kernels) == 12 == len(rows), [r["kernel"] for r in rows]
    forms = sorted(re.search(r"I(f|DF16b)Li([18])ELb([01])ELi3ELb([01])E", r["mangled"]).groups() for r in kernels)
    assert forms == sorted((ty, v, c, b) for ty in ("f", "DF16b") for v, c, b in
                           (("8", "0", "0"), ("8", "0", "1"), ("8", "1", "0"), ("8", "1", "1"), ("1", "0", "0"), ("1", "1", "0")))
    for r in rows:
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r


def test_the_stitched_family_copies_nothing():
    """one definition of the draw and of the kernel under csrc/: sde.hip and resample.hip include stitch_step.h"""
    import glob

    from inferbiomechanics_amd import hip
    texts = {os.path.basename(f): open(f).read() for f in glob.glob(os.path.join(os.path.dirname(hip.__file__), "csrc", "*"))
             if os.path.isfile(f) and f.endswith((".hip", ".h"))}
    defines = lambda name: sorted(f for f, t in texts.items() if name + "(" in t)     # a use names its template arguments
    assert defines("trial_noise") == ["stitch_step.h"] and defines("stitch_step_kernel") == ["stitch_step.h"]
    assert not defines("jump_noise") and not defines("sde_step_kernel")
    assert not [f for f, t in texts.items() if "jump_noise" in t or "sde_step_kernel" in t]
    for f in ("stitch.hip", "sde.hip", "resample.hip"):
        assert '#include "stitch_step.h"' in texts[f]


def test_makefile_builds_the_new_source_with_the_new_header():
    from inferbiomechanics_amd import hip
    text = open(os.path.join(os.path.dirname(hip.__file__), "csrc", "Makefile")).read()
    srcs = next(l for l in text.splitlines() if l.startswith("SRCS"))
    hdrs = next(l for l in text.splitlines() if l.startswith("HDRS"))
    assert "sde.hip" in srcs.split() and "../../include/ib_hip_sde.h" in hdrs.split()
    assert os.path.exists(os.path.join(os.path.dirname(hip.__file__), "csrc", "sde.hip"))
