"""Host side of the stochastic sampler (eta > 0) and the posterior ensembles of `analyze`, without a GPU: the float64
schedule tables, the C-ABI in dry-run mode (which entries the samplers launch, the window-id buffer, argument checks), the
predictor's window-id arithmetic and the CLI flags, and the register / scratch budget of the new kernels."""
import argparse
import ctypes
import os

import pytest
import torch

from oracle import ref_cpu as R


@pytest.fixture()
def dry():
    from inferbiomechanics_amd import hip
    hip.set_dry_run(True)
    yield hip
    hip.set_dry_run(False)


# ---------------------------------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [10, 100, 1000])
def test_eta_zero_tables_are_the_deterministic_ones_bit_for_bit(steps):
    from inferbiomechanics_amd.diffusion import schedule as S
    c = S.ddim_coefficients_eta(1000, steps, 0.0)
    assert c.dtype == torch.float64 and c.shape == (steps, 3)
    assert torch.equal(c[:, :2], S.ddim_coefficients(1000, steps)) and torch.equal(c[:, :2], R.ddim_coeffs(1000, steps))
    assert not c[:, 2].any()
    on = S.observation_noise_coefficients(1000, steps, 0.0)
    assert on.shape == (steps, 2)
    assert torch.equal(on[:-1], torch.tensor([[1.0, 0.0]], dtype=torch.float64).expand(steps - 1, 2))
    assert on[-1].tolist() == [0.0, 0.0]
    tabs = S.DiffusionTables(torch.device("cpu"), num_sample_steps=steps)
    before = (tabs.ddim_coef.clone(), tabs.obs_coef.clone(), tabs.ddim_t.clone())
    assert tabs.eta == 0.0 and tabs.ddim_coef_eta is None and tabs.obs_noise_coef is None
    tabs.set_sampler(steps, 0.5)
    assert tabs.eta == 0.5 and tabs.ddim_coef_eta.shape == (steps, 3) and tabs.obs_noise_coef.shape == (steps, 2)
    assert tabs.ddim_coef_eta.dtype == tabs.obs_noise_coef.dtype == torch.float32
    assert torch.equal(tabs.ddim_coef_eta, S.ddim_coefficients_eta(1000, steps, 0.5).to(torch.float32))
    for a, b in zip(before, (tabs.ddim_coef, tabs.obs_coef, tabs.ddim_t)):
        assert torch.equal(a, b)
    tabs.set_sampler(steps)                                     # without eta: what it did before
    assert tabs.eta == 0.0 and tabs.ddim_coef_eta is None


@pytest.mark.parametrize("steps", [10, 100, 1000])
@pytest.mark.parametrize("eta", [0.25, 0.5, 1.0])
def test_eta_tables_last_row_and_unit_noise(steps, eta):
    from inferbiomechanics_amd.diffusion import schedule as S
    c = S.ddim_coefficients_eta(1000, steps, eta)
    on = S.observation_noise_coefficients(1000, steps, eta)
    assert float(c[-1, 2]) == 0.0 and on[-1].tolist() == [0.0, 0.0]
    assert bool((c[:-1, 2] > 0).all())
    assert torch.equal(c[:, 0], S.ddim_coefficients(1000, steps)[:, 0])          # c_x does not depend on eta
    assert torch.equal(c[-1, :2], S.ddim_coefficients(1000, steps)[-1])          # sigma = 0: the deterministic row
    unit = (on[:-1] ** 2).sum(1)
    assert float((unit - 1).abs().max()) <= 4 * 2.0 ** -52
    ab = S.alphas_cumprod(1000)
    ts = S.ddim_timesteps(1000, steps).tolist()
    p = torch.stack([ab[t] for t in ts[1:]])
    assert torch.allclose(on[:-1, 1], c[:-1, 2] / torch.sqrt(1 - p), rtol=1e-14, atol=0)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            S.ddim_coefficients_eta(1000, steps, bad)
        with pytest.raises(ValueError):
            S.DiffusionTables(torch.device("cpu")).set_sampler(steps, bad)


def test_eta_one_full_length_is_the_ddpm_posterior():
    """Ho et al. 2020, eq. 6-7 and Algorithm 2: x_{t-1} = (x_t - beta_t eps / sqrt(1 - ab_t)) / sqrt(alpha_t) + sigma_t z with
    sigma_t^2 = beta_t (1 - ab_{t-1}) / (1 - ab_t); 1e-10 relative (measured 6e-13: float64 cancellation in c_eps)"""
    from inferbiomechanics_amd.diffusion import schedule as S
    N = 1000
    c = S.ddim_coefficients_eta(N, N, 1.0)
    beta = S.linear_beta_schedule(N)
    ab = S.alphas_cumprod(N)
    t = torch.arange(N - 1, -1, -1)
    ab_prev = torch.cat([torch.ones(1, dtype=torch.float64), ab[:-1]])
    rel = lambda a, e: float(((a - e) / e).abs().max())
    assert rel(c[:, 0], 1 / torch.sqrt(1 - beta[t])) <= 1e-10
    assert rel(c[:, 1], -beta[t] / (torch.sqrt(1 - beta[t]) * torch.sqrt(1 - ab[t]))) <= 1e-10
    var = beta[t] * (1 - ab_prev[t]) / (1 - ab[t])
    assert rel(c[:-1, 2] ** 2, var[:-1]) <= 1e-10 and float(c[-1, 2]) == 0.0 and float(var[-1]) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# C-ABI and samplers in dry-run mode
# ---------------------------------------------------------------------------------------------------------------------
NEW = ("ib_ddim_step_noise", "ib_ddim_cond_step_noise", "ib_ensemble_stats")


def test_header_library_and_dry_run_have_the_new_entries(dry):
    names = dry.declared_symbols()
    for n in NEW:
        assert n in names and n in dry._SIGS
        assert callable(getattr(dry.lib(), n))
    real = ctypes.CDLL(dry.LIB_PATH)
    for n in NEW:
        assert hasattr(real, n)


def small_transformer(dt):
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    return DiffusionTransformer(177, 10, d_model=32, num_heads=4, dim_feedforward=64, num_layers=1, temb_dim=16,
                                temb_hidden=24, compute_dtype=dt)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_samplers_launch_the_old_entries_at_eta_zero_and_the_new_ones_above(dry, dt):
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler, DDIMSampler
    m = small_transformer(dt)
    mask = torch.zeros(10, 177, dtype=torch.bool)
    mask[:, :147] = True
    xT, obs = torch.randn(2, 10, 177), torch.randn(2, 10, 177)
    per_loop = {}
    for eta in (0.0, 0.5, 1.0):
        for cls in (DDIMSampler, ConditionalDDIMSampler):
            smp = cls(m, 4, eta=eta, seed=7)
            dry.lib().calls.clear()
            out = smp.sample(xT, obs, mask) if cls is ConditionalDDIMSampler else smp.sample(xT)
            calls = list(dry.lib().calls)
            assert out.shape == (2, 10, 177)
            old, new = ("ib_ddim_cond_step", "ib_ddim_cond_step_noise") if cls is ConditionalDDIMSampler else \
                ("ib_ddim_step", "ib_ddim_step_noise")
            want, other = (old, new) if eta == 0.0 else (new, old)
            assert calls.count(want) == 4 and other not in calls, (eta, cls.__name__)
            assert calls.count("ib_ddim_cond_init") == (1 if cls is ConditionalDDIMSampler else 0)
            per_loop.setdefault(cls, set()).add(len(calls))
            assert ("win" in smp._bufs) == (eta > 0.0)
            assert smp._sig[-1 if eta == 0.0 else -4] == eta
            if eta > 0.0:
                tabs = m.tables(torch.device("cpu"))
                assert smp._sig[-3:] == (7, tabs.ddim_coef_eta.data_ptr(), tabs.obs_noise_coef.data_ptr())
    for cls, counts in per_loop.items():
        assert len(counts) == 1, f"{cls.__name__}: the launch count of a loop depends on eta: {counts}"
    assert DDIMSampler(m, 4).eta == 0.0 and ConditionalDDIMSampler(m, 4).eta == 0.0
    for bad in (-0.01, 1.01):
        with pytest.raises(ValueError):
            DDIMSampler(m, 4, eta=bad)
        with pytest.raises(ValueError):
            ConditionalDDIMSampler(m, 4, eta=bad)


def test_window_ids_are_refreshed_in_the_buffer_the_step_reads(dry):
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler, DDIMSampler
    m = small_transformer(torch.float32)
    mask = torch.zeros(10, 177, dtype=torch.bool)
    mask[:, :147] = True
    xT, obs = torch.randn(3, 10, 177), torch.randn(3, 10, 177)
    for cls in (DDIMSampler, ConditionalDDIMSampler):
        smp = cls(m, 4, eta=1.0, seed=1)
        run = (lambda **k: smp.sample(xT, obs, mask, **k)) if cls is ConditionalDDIMSampler else (lambda **k: smp.sample(xT, **k))
        run()
        buf, sig = smp._bufs["win"], smp._sig
        assert buf.dtype == torch.int64 and buf.tolist() == [0, 1, 2]
        run(window_ids=[40, 2 ** 32 - 1, 7])
        assert smp._bufs["win"] is buf and smp._sig is sig, "new ids must not re-create the captured step's buffers"
        assert buf.tolist() == [40, 2 ** 32 - 1, 7]
        run(window_ids=torch.tensor([5, 6, 8]))
        assert buf.tolist() == [5, 6, 8]
        run()
        assert buf.tolist() == [0, 1, 2]
        for bad in ([1, 2], [1, 2, -1], [0, 1, 2 ** 32]):
            with pytest.raises(ValueError):
                run(window_ids=bad)
    a, b, c = DDIMSampler(m, 4, eta=1.0, seed=1), DDIMSampler(m, 4, eta=1.0, seed=2), DDIMSampler(m, 4, eta=0.5, seed=1)
    a.sample(xT)
    b.sample(xT)
    assert a._sig != b._sig and a._sig[:-3] == b._sig[:-3], "the seed is part of the capture signature"
    c.sample(xT)
    assert a._sig[-4] == 1.0 and c._sig[-4] == 0.5


def test_bindings_reject_wrong_arguments(dry):
    from inferbiomechanics_amd.diffusion.schedule import DiffusionTables
    tabs = DiffusionTables(torch.device("cpu"), num_sample_steps=4)
    tabs.set_sampler(4, 1.0)
    x = torch.zeros(2, 10, 192)
    mk = torch.zeros(10, 192, dtype=torch.uint8)
    win = torch.zeros(2, dtype=torch.int64)
    step = lambda **k: dry.ddim_step_noise(k.get("x", x), k.get("eps", x), k.get("coef", tabs.ddim_coef_eta), tabs.ddim_t,
                                           k.get("win", win), 3, D=k.get("D", 177), t_out=k.get("t_out"))
    step()
    for bad in (dict(coef=tabs.ddim_coef), dict(win=win.to(torch.int32)), dict(win=torch.zeros(3, dtype=torch.int64)),
                dict(D=193), dict(D=0), dict(eps=x.to(torch.bfloat16)), dict(eps=torch.zeros(2, 10, 177)),
                dict(x=torch.zeros(20, 192)), dict(t_out=torch.zeros(3, dtype=torch.int64))):
        with pytest.raises(dry.HipError):
            step(**bad)
    cond = lambda **k: dry.ddim_cond_step_noise(k.get("x", x), k.get("eps", x), k.get("x0", x), k.get("z", x), k.get("mask", mk),
                                                k.get("coef", tabs.ddim_coef_eta), k.get("oc", tabs.obs_coef),
                                                k.get("on", tabs.obs_noise_coef), tabs.ddim_t, k.get("win", win), 3,
                                                D=k.get("D", 177))
    cond()
    for bad in (dict(coef=tabs.ddim_coef), dict(on=tabs.obs_coef), dict(on=tabs.obs_noise_coef.double()),
                dict(oc=tabs.obs_noise_coef), dict(mask=mk.bool()), dict(mask=torch.zeros(10, 177, dtype=torch.uint8)),
                dict(z=torch.zeros(2, 10, 177)), dict(win=torch.zeros(1, dtype=torch.int64)), dict(D=193)):
        with pytest.raises(dry.HipError):
            cond(**bad)
    ens = torch.zeros(3, 4, 10, 30)
    mean, std = dry.ensemble_stats(ens)
    assert mean.shape == std.shape == (3, 10, 30) and mean.dtype == std.dtype == torch.float32
    for bad in (torch.zeros(3, 4), ens[:, :, :, ::2], ens.double()):
        with pytest.raises(dry.HipError):
            dry.ensemble_stats(bad)
    with pytest.raises(dry.HipError):
        dry.ensemble_stats(ens, mean=torch.zeros(3, 10, 29))


# ---------------------------------------------------------------------------------------------------------------------
# the seven sampler-update wrappers (the DPM-Solver++ pair included: one harness) on the smallest state on which every operand
# check can fire: x [2, 3, 8], fp32 and bf16, S = 4 steps, and D = 6 feature columns in front of the pitch ld = 8
# ---------------------------------------------------------------------------------------------------------------------
S_, B_, T_, LD_ = 4, 2, 3, 8
# wrapper -> (its positional operands, columns of coef, the entry's pointer arguments in ABI order, its scalar arguments)
WRAPPERS = {
    "ddim_step": ("x eps coef timesteps", 2, "x eps coef timesteps step_dev t_out", "S step B n dtype"),
    "ddim_cond_step": ("x eps x0 z mask coef obs_coef timesteps", 2,
                       "x eps x0 z mask coef obs_coef timesteps step_dev t_out", "S step B T D ld dtype"),
    "ddim_cond_init": ("x x0 z mask obs_coef", None, "x x0 z mask obs_coef", "B T D ld dtype"),
    "ddim_step_noise": ("x eps coef timesteps win_id seed", 3, "x eps coef timesteps step_dev t_out win_id",
                        "S step seed B T D ld dtype"),
    "ddim_cond_step_noise": ("x eps x0 z mask coef obs_coef obs_noise_coef timesteps win_id seed", 3,
                             "x eps x0 z mask coef obs_coef obs_noise_coef timesteps step_dev t_out win_id",
                             "S step seed B T D ld dtype"),
    "dpmpp_step": ("x eps hist coef timesteps", 5, "x eps hist coef timesteps step_dev t_out", "S step B n dtype"),
    "dpmpp_cond_step": ("x eps hist x0 z mask coef obs_coef timesteps", 5,
                        "x eps hist x0 z mask coef obs_coef timesteps step_dev t_out", "S step B T D ld dtype"),
}


def sampler_operands(dt, ncols):
    st = lambda: torch.zeros(B_, T_, LD_, dtype=dt)
    return dict(x=st(), eps=st(), x0=st(), z=st(), hist=torch.zeros(B_, T_, LD_), mask=torch.zeros(T_, LD_, dtype=torch.uint8),
                coef=torch.zeros(S_, ncols or 2), obs_coef=torch.zeros(S_ + 1, 2), obs_noise_coef=torch.zeros(S_, 2),
                timesteps=torch.zeros(S_, dtype=torch.int64), win_id=torch.zeros(B_, dtype=torch.int64), seed=-5,
                t_out=torch.zeros(B_, dtype=torch.int64), step_dev=torch.zeros(1, dtype=torch.int32))


def call_wrapper(hip, name, ops, **kw):
    return getattr(hip, name)(*[ops[k] for k in WRAPPERS[name][0].split()], **kw)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", sorted(WRAPPERS))
def test_sampler_wrapper_marshals_one_call_of_its_entry(dry, name, dt):
    positional, ncols, pointers, scalars = WRAPPERS[name]
    ops = sampler_operands(dt, ncols)
    masked_or_noise = "D" in scalars
    has_tables = ncols is not None
    rec = dry.lib()
    # the call the sampler loops make: device counter, next-timestep vector, D columns in front of the pitch
    kw = dict(step=3, step_dev=ops["step_dev"], t_out=ops["t_out"]) if has_tables else {}
    if masked_or_noise:
        kw["D"] = 6
    assert call_wrapper(dry, name, ops, **kw) is ops["x"]
    assert rec.calls == ["ib_" + name] and [n for n, _ in rec.args] == rec.calls
    sig = dry._SIGS["ib_" + name][1]
    args = rec.args[0][1]
    assert len(args) == len(sig)
    got_ptrs = [v for v, t in zip(args, sig) if t is ctypes.c_void_p]
    got_scalars = [v for v, t in zip(args, sig) if t is not ctypes.c_void_p]
    assert got_ptrs == [ops[k].data_ptr() for k in pointers.split()] + [0]          # ... and the (dry-run) stream last
    code = {torch.float32: 0, torch.bfloat16: 1}[dt]
    want = dict(S=4, step=3, seed=2 ** 64 - 5, B=2, T=3, D=6, ld=8, n=48, dtype=code)
    assert got_scalars == [want[k] for k in scalars.split()], (got_scalars, scalars)
    # the defaults: host step 0, no counter, no t_out, D = ld
    call_wrapper(dry, name, ops)
    args = rec.args[1][1]
    want.update(step=0, D=8)
    assert [v for v, t in zip(args, sig) if t is not ctypes.c_void_p] == [want[k] for k in scalars.split()]
    none_at = [k for k, v in zip(pointers.split(), [v for v, t in zip(args, sig) if t is ctypes.c_void_p]) if v is None]
    assert none_at == (["step_dev", "t_out"] if has_tables else [])
    assert rec.calls == ["ib_" + name] * 2


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", sorted(WRAPPERS))
def test_sampler_wrapper_refuses_every_wrong_operand_before_the_library(dry, name, dt):
    positional, ncols, pointers, scalars = WRAPPERS[name]
    good = sampler_operands(dt, ncols)
    other = torch.float32 if dt == torch.bfloat16 else torch.bfloat16
    i64, i32 = torch.int64, torch.int32
    has = lambda k: k in positional.split()
    bad = []                                                        # (what is wrong, operands replaced, keywords)
    if has("eps"):
        bad += [("eps of another shape", dict(eps=torch.zeros(B_, T_, LD_ - 1, dtype=dt)), {}),
                ("eps of another dtype", dict(eps=torch.zeros(B_, T_, LD_, dtype=other)), {}),
                ("eps not contiguous", dict(eps=torch.zeros(B_, T_, 2 * LD_, dtype=dt)[:, :, ::2]), {})]
    if has("hist"):
        bad += [("hist in the state's dtype", dict(hist=torch.zeros(B_, T_, LD_, dtype=torch.bfloat16)), {}),
                ("hist of another shape", dict(hist=torch.zeros(B_, T_, LD_ - 1)), {})]
    if has("coef"):
        bad += [("coef one column short", dict(coef=torch.zeros(S_, ncols - 1)), {}),
                ("coef not contiguous", dict(coef=torch.zeros(S_, 2 * ncols)[:, ::2]), {}),
                ("timesteps one short", dict(timesteps=torch.zeros(S_ - 1, dtype=i64)), {}),
                ("t_out of B + 1", {}, dict(t_out=torch.zeros(B_ + 1, dtype=i64))),
                ("t_out int32", {}, dict(t_out=torch.zeros(B_, dtype=i32))),
                ("step_dev int64", {}, dict(step_dev=torch.zeros(1, dtype=i64)))]
    if has("mask"):
        bad += [("mask [T, ld - 1]", dict(mask=torch.zeros(T_, LD_ - 1, dtype=torch.uint8)), {}),
                ("mask bool", dict(mask=torch.zeros(T_, LD_, dtype=torch.bool)), {}),
                ("x0 of another shape", dict(x0=torch.zeros(B_, T_, LD_ - 1, dtype=dt)), {}),
                ("z of another dtype", dict(z=torch.zeros(B_, T_, LD_, dtype=other)), {}),
                ("obs_coef with three columns", dict(obs_coef=torch.zeros(S_ + 1, 3)), {})]
        if has("coef"):                                             # (ddim_cond_init reads row 0 only: it has no S)
            bad += [("obs_coef with S rows", dict(obs_coef=torch.zeros(S_, 2)), {})]
    if has("obs_noise_coef"):
        bad += [("obs_noise_coef with S + 1 rows", dict(obs_noise_coef=torch.zeros(S_ + 1, 2)), {})]
    if has("win_id"):
        bad += [("win_id of B + 1", dict(win_id=torch.zeros(B_ + 1, dtype=i64)), {}),
                ("win_id int32", dict(win_id=torch.zeros(B_, dtype=i32)), {})]
    if "D" in scalars:
        bad += [("D = 0", {}, dict(D=0)), ("D = ld + 1", {}, dict(D=LD_ + 1)),
                ("x without the frame axis", dict(x=torch.zeros(B_ * T_, LD_, dtype=dt)), {})]
    else:
        bad += [("x without any axis", dict(x=torch.zeros((), dtype=dt), eps=torch.zeros((), dtype=dt),
                                            hist=torch.zeros(())), {})]
    bad += [("x not contiguous", dict(x=torch.zeros(B_, T_, 2 * LD_, dtype=dt)[:, :, ::2]), {})]
    rec = dry.lib()
    for what, ops, kw in bad:
        with pytest.raises(dry.HipError) as e:
            call_wrapper(dry, name, {**good, **ops}, **kw)
        assert rec.calls == [] and rec.args == [], f"{name}, {what}: the library was called"
        assert not str(e.value).startswith(tuple(w + ":" for w in WRAPPERS if w != name)), \
            f"{name}, {what}: the message names another wrapper: {e.value}"
    call_wrapper(dry, name, good)                                   # and the operands they were derived from are accepted
    assert rec.calls == ["ib_" + name]


def test_new_entries_return_error_codes_on_bad_arguments():
    from inferbiomechanics_amd import hip
    lib = hip.lib()
    buf = ctypes.create_string_buffer(4096)
    a = ctypes.cast(buf, ctypes.c_void_p).value // 16 * 16 + 16          # any aligned non-NULL address: nothing is launched
    P = lambda ok=True: ctypes.c_void_p(a) if ok else None
    # x, eps, coef, timesteps | S, step, step_dev, t_out, win_id, seed | B, T, D, ld, dtype
    step = lambda nulls=(), win=True, t_out=False, B=2, T=10, D=177, ld=192, S=4, dtype=1: lib.ib_ddim_step_noise(
        *[P(i not in nulls) for i in range(4)], S, 0, None, P() if t_out else None, P(win), 5, B, T, D, ld, dtype, None)
    for i in range(3):
        assert step(nulls=(i,)) == -1, i
    assert step(nulls=(3,), t_out=True) == -1 and step(win=False) == -1
    assert step(ld=176) == -1 and step(B=0) == -1 and step(T=0) == -1 and step(D=0) == -1 and step(S=0) == -1
    assert step(dtype=7) == -2 and step(T=1 << 24, ld=192) == -5
    cond = lambda nulls=(), win=True, ld=192, dtype=1: lib.ib_ddim_cond_step_noise(
        *[P(i not in nulls) for i in range(9)], 4, 0, None, None, P(win), 5, 2, 10, 177, ld, dtype, None)
    for i in range(8):                                            # x, eps, x0, z, mask, coef, obs_coef, obs_noise_coef
        assert cond(nulls=(i,)) == -1, i
    assert cond(win=False) == -1 and cond(ld=100) == -1 and cond(dtype=7) == -2
    ens = lambda nulls=(), B=2, K=3, n=5, dtype=1: lib.ib_ensemble_stats(*[P(i not in nulls) for i in range(3)], B, K, n, dtype, None)
    for i in range(3):
        assert ens(nulls=(i,)) == -1
    assert ens(B=0) == -1 and ens(K=0) == -1 and ens(n=0) == -1 and ens(dtype=7) == -2


# ---------------------------------------------------------------------------------------------------------------------
# predictor and CLI
# ---------------------------------------------------------------------------------------------------------------------
def windows(n):
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import SyntheticWindowDataset
    ds = SyntheticWindowDataset(n, 50, 5)
    items = [ds[i] for i in range(n)]
    return ({k: torch.stack([it[0][k] for it in items]) for k in items[0][0]},
            {k: torch.stack([it[1][k] for it in items]) for k in items[0][1]})


def test_predictor_replicates_windows_and_numbers_the_members(dry, monkeypatch):
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import LOSS_KEY_ORDER, LOSS_KEY_WIDTHS
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionMLP
    from inferbiomechanics_amd.models.DiffusionLabelPredictor import DiffusionLabelPredictor
    inputs, labels = windows(6)
    model = DiffusionMLP(177, [32, 32], temb_dim=16, temb_hidden=24)
    seen = []
    orig = ConditionalDDIMSampler.sample

    def spy(self, x_T, observed, mask, steps=None, window_ids=None):
        seen.append((tuple(x_T.shape), observed.clone(), None if window_ids is None else list(window_ids)))
        return orig(self, x_T, observed, mask, steps, window_ids)

    monkeypatch.setattr(ConditionalDDIMSampler, "sample", spy)
    K = 4
    pred = DiffusionLabelPredictor(model, 5, seed=3, eta=1.0, num_samples=K)
    assert pred.sampler.eta == 1.0 and pred.sampler.seed == 3
    ids = {}
    for batch in (1, 3, 6):                                       # --sample-batch: the same ids whatever the batching
        seen.clear()
        dry.lib().calls.clear()
        got = []
        for i in range(0, 6, batch):
            one = lambda d: {k: v[i:i + batch] for k, v in d.items()}
            out = pred(one(inputs), one(labels), draw=i)
            assert list(out) == LOSS_KEY_ORDER and list(pred.last_std) == LOSS_KEY_ORDER
            for k, w in zip(LOSS_KEY_ORDER, LOSS_KEY_WIDTHS):
                assert out[k].shape == pred.last_std[k].shape == (batch, 10, w)
                assert out[k].dtype == pred.last_std[k].dtype == torch.float32
            shape, observed, wids = seen[-1]
            assert shape == (batch * K, 10, 177)                  # B K sampler rows
            want_obs = DiffusionLabelPredictor.window_matrix(one(inputs))
            assert torch.equal(observed.view(batch, K, 10, 177), want_obs.unsqueeze(1).expand(batch, K, 10, 177))
            got += wids
        ids[batch] = got
        calls = dry.lib().calls
        assert calls.count("ib_ensemble_stats") == 6 // batch and calls.count("ib_ddim_cond_step_noise") == 5 * (6 // batch)
        assert calls.count("ib_diffusion_draw") == 6 * K and "ib_ddim_cond_step" not in calls
    assert ids[1] == ids[3] == ids[6] == [i * K + k for i in range(6) for k in range(K)]
    assert pred.member_ids(2, 2) == [8, 9, 10, 11, 12, 13, 14, 15]

    # defaults: the deterministic path, no ensemble launch, no std
    seen.clear()
    dry.lib().calls.clear()
    base = DiffusionLabelPredictor(model, 5, seed=3)
    base(inputs, labels, draw=2)
    assert base.last_std is None and seen[-1][2] is None and seen[-1][0] == (6, 10, 177)
    assert "ib_ensemble_stats" not in dry.lib().calls and dry.lib().calls.count("ib_ddim_cond_step") == 5
    # K > 1 at eta = 0: members differ by their start draws only
    dry.lib().calls.clear()
    DiffusionLabelPredictor(model, 5, num_samples=2)(inputs, labels)
    assert dry.lib().calls.count("ib_ddim_cond_step") == 5 and dry.lib().calls.count("ib_ensemble_stats") == 1
    for bad in (dict(eta=-0.5), dict(eta=2.0), dict(num_samples=0), dict(num_samples=1.5)):
        with pytest.raises(ValueError):
            DiffusionLabelPredictor(model, 5, **bad)


def test_analyze_flags_validate_and_report_the_spread(dry, tmp_path, capsys):
    from inferbiomechanics_amd.cli.analyze import AnalyzeCommand
    from inferbiomechanics_amd.main import main
    p = argparse.ArgumentParser()
    sp = p.add_subparsers(dest="command")
    AnalyzeCommand().register_subcommand(sp)
    a = p.parse_args(['analyze', '--model-type', 'diffusion-mlp'])
    assert (a.sample_eta, a.num_samples) == (0.0, 1)
    a = p.parse_args(['analyze', '--model-type', 'diffusion-mlp', '--sample-eta', '0.5', '--num-samples', '8'])
    assert (a.sample_eta, a.num_samples) == (0.5, 8)

    ck = str(tmp_path / "ck")
    common = ['--no-wandb', '--checkpoint-dir', ck, '--data-loading-workers', '0', '--model-type', 'diffusion-mlp',
              '--hidden-dims', '32', '32']
    assert main(['train', '--synthetic-windows', '8', '--feat-dim', '177', '--epochs', '1', '--max-steps', '1',
                 '--batch-size', '4'] + common)
    analyze = ['analyze', '--synthetic-windows', '5', '--sample-steps', '4', '--sample-batch', '2'] + common
    for bad in (['--sample-eta', '1.5'], ['--sample-eta', '-0.1'], ['--num-samples', '0']):
        with pytest.raises(SystemExit):
            main(analyze + bad)
    capsys.readouterr()
    dry.lib().calls.clear()
    assert main(analyze)
    plain = capsys.readouterr().out
    assert 'Ensemble spread' not in plain and "ib_ensemble_stats" not in dry.lib().calls
    assert "ib_ddim_cond_step_noise" not in dry.lib().calls
    dry.lib().calls.clear()
    assert main(analyze + ['--sample-eta', '1', '--num-samples', '3'])
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith('Ensemble spread')]
    assert len(lines) == 2 and lines[0].startswith('Ensemble spread (dev, 3 samples per window): ')
    assert lines[1].startswith('Ensemble spread (train, 3 samples per window): ')
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import LOSS_KEY_ORDER
    for k in LOSS_KEY_ORDER:
        assert f'{k}: mean std ' in lines[0] and 'RMS err of mean ' in lines[0]
    calls = dry.lib().calls
    assert calls.count("ib_ensemble_stats") == 6 and calls.count("ib_ddim_cond_step_noise") == 6 * 4
    rows = open(os.path.join(ck, 'diffusion-mlp', 'dev_analysis.csv')).read().strip().splitlines()
    assert rows == [f'synthetic_subject_0,window_{i}' for i in range(5)] * 2


# ---------------------------------------------------------------------------------------------------------------------
# register / scratch budget of the new kernels (compiles csrc/diffusion.hip's device side once)
# ---------------------------------------------------------------------------------------------------------------------
def test_new_kernels_do_not_spill():
    from tools import kernel_resources as kr
    if kr.hipcc() is None:
        pytest.skip("hipcc not installed")
    res = [k for k in kr.resources("diffusion.hip")
           if k["kernel"].startswith(("ddim_step_noise_kernel", "ddim_cond_step_noise_kernel", "ensemble_stats_kernel"))]
    names = {k["kernel"] for k in res}
    for dt in ("float", "bf16"):
        for form in ("1,0", "8,1", "8,0"):
            assert f"ddim_step_noise_kernel<{dt},{form}>" in names and f"ddim_cond_step_noise_kernel<{dt},{form}>" in names, names
        assert f"ensemble_stats_kernel<{dt}>" in names, names
    bad = [f"{k['kernel']}: {k['vgpr_spill']} VGPRs spilled, {k['scratch']} B/lane scratch, {k['occupancy']} waves/SIMD"
           for k in res if k["vgpr_spill"] or k["scratch"] or k["occupancy"] < 4]
    assert not bad, "\n".join(bad)
