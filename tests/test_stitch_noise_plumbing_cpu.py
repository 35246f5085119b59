"""Host-side plumbing of stochastic stitched sampling (no GPU): its declaration in the stitched header, the refusals and the
dry-run launches of StochasticStitchedSampler, predict_trial_ensemble, the visualize flags, and the kernel's registers."""
import os
import re
import subprocess

import pytest
import torch

NAME = "ib_stitch_ddim_step_noise"


@pytest.fixture()
def dry():
    from inferbiomechanics_amd import hip
    hip.set_dry_run(True)
    yield hip
    hip.set_dry_run(False)


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def _tr(dt=torch.float32, D=44, T=8):
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    return DiffusionTransformer(D, T, d_model=32, num_heads=4, dim_feedforward=64, num_layers=1, temb_dim=16, temb_hidden=24,
                                compute_dtype=dt)


def test_third_header_has_its_own_table_and_both_builds_export_it():
    """ib_stitch_ddim_step_noise is declared in the stitched header, bound from its table, exported by both builds"""
    from inferbiomechanics_amd import hip
    assert hip.stitch_symbols() == ["ib_stitch_ddim_step", NAME, "ib_stitch_dpmpp_step"]
    assert NAME not in hip._SIGS and NAME not in hip.declared_symbols()                 # ib_hip.h's table is what it was
    assert len(hip._SIGS) == 127
    res, args = hip._STITCH_SIGS[NAME]
    assert res is hip._c.c_int and len(args) == 26 and args[-1] is hip._vp and args[17] is hip._c.c_uint64
    assert hip._is_launch(NAME) and hip._sig(NAME) == (res, args)
    for path in (hip.LIB_PATH, hip.AB_LIB_PATH):
        if not os.path.exists(path):
            pytest.fail(f"{path} is not built")
        assert NAME in _exports(path), path
    fn = getattr(hip.lib(), NAME)
    assert fn.restype is hip._c.c_int and list(fn.argtypes) == args


def test_a_symbol_declared_in_two_headers_is_refused(monkeypatch):
    """the module is loaded again under another name with a stitched header that declares ib_ddim_step (the first header's)
    once more: the import must raise; so must a name repeated inside the one header"""
    import importlib.util

    from inferbiomechanics_amd import hip
    second = open(hip.STITCH_HEADER_PATH).read()

    def load(extra):
        spec = importlib.util.spec_from_file_location("inferbiomechanics_amd._hip_twice", hip.__file__)
        mod = importlib.util.module_from_spec(spec)
        real_open = open

        def fake_open(path, *a, **kw):
            f = real_open(path, *a, **kw)
            if os.path.abspath(str(path)) != os.path.abspath(hip.STITCH_HEADER_PATH):
                return f
            f.close()
            import io
            return io.StringIO(second.replace("#ifdef __cplusplus\n}", extra + "\n#ifdef __cplusplus\n}"))

        mod.__dict__["open"] = fake_open                               # the module's own lookup of open() finds this one
        spec.loader.exec_module(mod)
        return mod

    assert NAME in load("").stitch_symbols()                           # the loader itself works on the real text
    # the second copy of the module raises its own HipError class, a RuntimeError like the first
    with pytest.raises(RuntimeError, match="declared in two headers.*ib_ddim_step"):
        load("int ib_ddim_step(void* x, ib_stream_t stream);")
    with pytest.raises(RuntimeError, match="ib_stitch_dpmpp_step is declared twice"):
        load("int ib_stitch_dpmpp_step(void* x, ib_stream_t stream);")


@pytest.mark.parametrize("cond", [False, True])
def test_dry_run_issues_one_noise_launch_per_step(dry, cond):
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion import StochasticStitchedSampler
    N, F, D, T, S = 2, 17, 44, 8, 5
    m = _tr(torch.bfloat16)
    s = StochasticStitchedSampler(m, S, eta=0.5, hop=3, seed=(7 << 32) + 3)
    cols = torch.zeros(D, dtype=torch.bool)
    cols[:14] = True
    dry.lib().calls.clear()
    dry.lib().args.clear()
    out = s.sample(torch.randn(N, F, D), *((torch.randn(N, F, D), cols) if cond else ()), trial_ids=[5, (1 << 32) - 1])
    assert out.shape == (N, F, D)
    calls = dry.lib().calls
    assert calls.count(NAME) == S and calls.count("ib_ddim_cond_init") == (1 if cond else 0)
    for other in ("ib_stitch_ddim_step", "ib_stitch_dpmpp_step", "ib_ddim_step", "ib_ddim_cond_step", "ib_ddim_step_noise",
                  "ib_ddim_cond_step_noise", "ib_dpmpp_step", "ib_dpmpp_cond_step"):
        assert other not in calls
    b, lay, tabs = s._bufs, s.layout, m.tables(torch.device("cpu"))
    Dp, W = b["x"].shape[-1], lay["W"]
    assert W == 4 and Dp % 8 == 0 and Dp >= D
    p = lambda t: None if t is None else t.data_ptr()
    cnd = [p(b["x0"]), p(b["z"]), p(b["mask"])] if cond else [None, None, None]
    want = [p(b["x"]), p(b["eps"])] + cnd + \
           [p(tabs.ddim_coef_eta), p(tabs.obs_coef) if cond else None, p(tabs.obs_noise_coef) if cond else None,
            p(tabs.ddim_t), S, 0, p(b["ctr"]), p(b["t"]), p(lay["start"]), p(lay["cover"]), p(lay["wn"]), p(b["win"]),
            (7 << 32) + 3, N, W, T, F, D, Dp, hip.BF16, 0]
    got = [a for n, a in dry.lib().args if n == NAME]
    assert len(got) == S
    for a in got:
        assert list(a) == want
    assert b["win"].tolist() == [5, (1 << 32) - 1] and b["t"].numel() == N * W        # 'win': one id per trial here
    assert tuple(tabs.ddim_coef_eta.shape) == (S, 3)
    # default ids 0 .. N-1, through sample_noise as well
    s.sample(torch.randn(N, F, D), *((torch.randn(N, F, D), cols) if cond else ()))
    assert s._bufs["win"].tolist() == [0, 1]
    s.sample_noise(N, F, D, *((torch.randn(N, F, D), cols) if cond else (None, None)), seed=1, trial_ids=[9, 4])
    assert s._bufs["win"].tolist() == [9, 4]


def test_eta_zero_runs_the_parents_update(dry):
    from inferbiomechanics_amd.diffusion import StochasticStitchedSampler
    s = StochasticStitchedSampler(_tr(torch.bfloat16), 5, eta=0.0, hop=3)
    dry.lib().calls.clear()
    s.sample(torch.randn(2, 17, 44))
    assert dry.lib().calls.count("ib_stitch_ddim_step") == 5 and NAME not in dry.lib().calls


def test_sampler_refusals(dry):
    import inspect

    from inferbiomechanics_amd.diffusion import StitchedDDIMSampler, StochasticStitchedSampler
    m = _tr()
    for eta in (-0.1, 1.5):
        with pytest.raises(ValueError, match="eta"):
            StochasticStitchedSampler(m, 5, eta=eta)
    assert "solver" not in inspect.signature(StochasticStitchedSampler.__init__).parameters
    with pytest.raises(ValueError, match="hop"):
        StochasticStitchedSampler(m, 5, hop=9)
    s = StochasticStitchedSampler(m, 5)
    assert isinstance(s, StitchedDDIMSampler) and s.eta == 1.0 and s.solver == "ddim" and s.hop == 4 and s.blend == "ramp"
    z = torch.randn(2, 17, 44)
    with pytest.raises(ValueError, match="one id per trial"):
        s.sample(z, trial_ids=[1, 2, 3])
    with pytest.raises(ValueError, match="one id per trial"):
        s.sample(z, trial_ids=list(range(2 * 3)))                      # one per window is not one per trial
    with pytest.raises(ValueError, match="2\\^32"):
        s.sample(z, trial_ids=[0, 1 << 32])
    with pytest.raises(ValueError, match="2\\^32"):
        s.sample(z, trial_ids=[-1, 0])
    with pytest.raises(ValueError, match="together"):
        s.sample(z, torch.randn(2, 17, 44), None)
    with pytest.raises(ValueError, match="eta"):                       # the deterministic class keeps its refusal
        StitchedDDIMSampler(m, 5, eta=0.5)


def test_binding_refusals(dry):
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion.schedule import stitch_layout
    N, W, T, F, D, S = 2, 4, 8, 17, 16, 5
    start, cover, wn, _ = stitch_layout(F, T, 3, "ramp")
    assert start.numel() == W
    x, eps = torch.zeros(N, W, T, D), torch.zeros(N, W, T, D)
    coef, ts, ids = torch.zeros(S, 3), torch.zeros(S, dtype=torch.int64), torch.zeros(N, dtype=torch.int64)
    go = lambda **kw: hip.stitch_ddim_step_noise(*[kw.get(k, v) for k, v in (
        ("x", x), ("eps", eps), ("x0", None), ("z", None), ("mask", None), ("coef", coef), ("obs_coef", None),
        ("obs_noise_coef", None), ("timesteps", ts), ("start", start), ("cover", cover), ("wn", wn), ("trial_ids", ids),
        ("seed", 1))])
    go()
    with pytest.raises(hip.HipError):
        go(coef=torch.zeros(S, 2))
    with pytest.raises(hip.HipError, match="trial_ids"):
        go(trial_ids=torch.zeros(N * W, dtype=torch.int64))
    with pytest.raises(hip.HipError):
        go(trial_ids=torch.zeros(N, dtype=torch.int32))
    with pytest.raises(hip.HipError, match="together"):
        go(obs_noise_coef=torch.zeros(S, 2))
    with pytest.raises(hip.HipError, match="together"):
        go(x0=x.clone(), z=x.clone(), mask=torch.zeros(T, D, dtype=torch.uint8), obs_coef=torch.zeros(S + 1, 2))
    with pytest.raises(hip.HipError, match="obs_noise_coef"):
        go(x0=x.clone(), z=x.clone(), mask=torch.zeros(T, D, dtype=torch.uint8), obs_coef=torch.zeros(S + 1, 2),
           obs_noise_coef=torch.zeros(S + 1, 2))


def _trials(n):
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import SyntheticWindowDataset
    ds = SyntheticWindowDataset(4, 50, 5)                              # windows of 10 frames
    items = [ds[i] for i in range(4)]
    return {k: torch.cat([it[0][k] for it in items[:2]]).unsqueeze(0).repeat(n, 1, 1) for k in items[0][0]}   # [n, 20, c]


def test_predict_trial_ensemble_layout_in_dry_run(dry):
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import LOSS_KEY_ORDER, LOSS_KEY_WIDTHS
    from inferbiomechanics_amd.diffusion import StochasticStitchedSampler
    from inferbiomechanics_amd.models.DiffusionLabelPredictor import DiffusionLabelPredictor
    inputs = _trials(2)
    pred = DiffusionLabelPredictor(_tr(D=177, T=10), 5, eta=1.0, num_samples=3, seed=11)
    dry.lib().calls.clear()
    dry.lib().args.clear()
    out = pred.predict_trial_ensemble(inputs, hop=4, blend="uniform", draw=1)
    assert list(out) == LOSS_KEY_ORDER and list(pred.last_std) == LOSS_KEY_ORDER
    for k, w in zip(LOSS_KEY_ORDER, LOSS_KEY_WIDTHS):
        assert out[k].shape == (2, 20, w) and out[k].dtype == torch.float32
        assert pred.last_std[k].shape == (2, 20, w) and pred.last_std[k].dtype == torch.float32
    calls = dry.lib().calls
    assert calls.count(NAME) == 5 and calls.count("ib_diffusion_draw") == 6 and calls.count("ib_ensemble_stats") == 1
    _, sampler, _ = pred._trial_ens
    assert isinstance(sampler, StochasticStitchedSampler) and sampler.eta == 1.0 and sampler.seed == 11
    assert sampler._bufs["win"].tolist() == [3, 4, 5, 6, 7, 8]         # member k of trial i = draw + b: i K + k
    a = next(a for n, a in dry.lib().args if n == NAME)
    assert a[18] == 6 and a[21] == 20                                  # N = 2 trials x 3 members, F = 20
    assert pred.predict_trial_ensemble(inputs, hop=4, blend="uniform") and pred._trial_ens[1] is sampler   # kept per (hop, blend, D)
    with pytest.raises(ValueError, match="shorter"):
        pred.predict_trial_ensemble({k: v[:, :9] for k, v in inputs.items()})
    with pytest.raises(ValueError, match="eta"):                       # predict_trial keeps its refusals
        pred.predict_trial(inputs)
    with pytest.raises(ValueError, match="deterministic"):
        DiffusionLabelPredictor(_tr(D=177, T=10), 5, num_samples=2, solver="dpmpp2m").predict_trial_ensemble(inputs)


def test_visualize_ensemble_flags_and_spread_lines(dry, tmp_path, capsys):
    import argparse

    from inferbiomechanics_amd.cli.visualize import VisualizeCommand
    from inferbiomechanics_amd.main import main
    p = argparse.ArgumentParser()
    VisualizeCommand().register_subcommand(p.add_subparsers(dest="command"))
    a = p.parse_args(["visualize"])
    assert (a.sample_eta, a.num_samples, a.sampler) == (0.0, 1, "ddim")
    tr = ["visualize", "--synthetic-windows", "60", "--checkpoint-dir", str(tmp_path / "ck"), "--sample-steps", "4",
          "--model-type", "diffusion-transformer", "--trial-frames", "25", "--trial-hop", "4", "--num-frames", "2"]
    capsys.readouterr()
    dry.lib().calls.clear()
    assert main(tr + ["--sample-eta", "1", "--num-samples", "2"])
    out = capsys.readouterr().out.splitlines()
    calls = dry.lib().calls
    assert calls.count(NAME) == 2 * 4 and calls.count("ib_ddim_cond_step_noise") == 2 * 4
    assert "ib_stitch_ddim_step" not in calls and calls.count("ib_ensemble_stats") == 2 * 2
    assert calls.count("ib_diffusion_draw") == 2 * 2 * (1 + 3)
    # a dry run computes nothing: the figures are whatever the unwritten buffers hold, so only their layout is checked
    fig = r"-?(?:\d+\.\d+|nan|inf)"
    for k in range(2):
        lines = [l for l in out if re.match(rf"^trial {k} +\w+: mean std over 2 samples ", l)]
        assert len(lines) == 4, out
        for name, line in zip(("cop", "force", "torque", "wrench"), lines):
            assert re.match(rf"^trial {k} +{name}: mean std over 2 samples stitched {fig}, per-window {fig}$", line), line
        assert sum(1 for l in out if re.match(rf"^trial {k} +\w+: RMS err stitched ", l)) == 4
    # the defaults print no spread line and run the deterministic loops
    dry.lib().calls.clear()
    assert main(tr)
    assert "mean std over" not in capsys.readouterr().out
    assert NAME not in dry.lib().calls and dry.lib().calls.count("ib_stitch_ddim_step") == 2 * 4
    for bad, msg in ((tr + ["--sample-eta", "1.5"], "sample-eta"), (tr + ["--num-samples", "0"], "num-samples")):
        with pytest.raises(SystemExit, match=msg):
            main(bad)
    for bad in (["--sampler", "dpmpp2m", "--sample-eta", "0.5"], ["--sampler", "dpmpp2m", "--num-samples", "2"]):
        with pytest.raises(SystemExit, match="dpmpp2m is deterministic"):
            main(tr + bad)
    # the deterministic second-order loop through the same flag
    dry.lib().calls.clear()
    assert main(tr + ["--sampler", "dpmpp2m"])
    calls = dry.lib().calls
    assert calls.count("ib_stitch_dpmpp_step") == 2 * 4 and calls.count("ib_dpmpp_cond_step") == 2 * 4 and NAME not in calls
    assert "mean std over" not in capsys.readouterr().out


def test_kernel_resources_no_scratch_no_spill():
    from tools import kernel_resources as kr
    if kr.hipcc() is None:
        pytest.skip("hipcc not installed")
    resources = kr.resources
    rows = resources("stitch.hip")
    kernels = [r for r in rows if "stitch_step_kernel" in r["kernel"]]
    # the 16 deterministic forms + the noise forms: fp32 / bf16 x {8-wide: cond x whole blocks, element-wise: cond}
    assert len(kernels) == 16 + 2 * (4 + 2), [r["kernel"] for r in rows]
    noise = [r for r in kernels if re.search(r"Li[18]ELb[01]ELi2ELb[01]E", r["mangled"])]
    assert len(noise) == 2 * (4 + 2), [r["mangled"] for r in kernels]
    for r in rows:
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
