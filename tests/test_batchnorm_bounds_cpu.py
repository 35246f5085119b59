"""The elementwise BatchNorm1d bound of tests/batchnorm_cases.py, checked without a GPU.

a. A torch-CPU emulation of csrc/batchnorm.hip's arithmetic (fp32; the rows split over 4 waves, each summing its rows in
   order, combined as ((w0 + w1) + w2) + w3; two passes for the variance; outputs stored in the case dtype) stays inside
   the bound on every case, in both dtypes, forward and backward, training and eval: the bound admits a correct kernel.
b. Nine one-line bugs, applied to that emulation, fall outside the bound on NAMED cases: the bound and the inputs are sharp
   enough to see them.
c. The float64 reference equals torch.nn.functional.batch_norm (and its autograd) in float64 to 1e-12.
d. The launch geometry restated in Python gives what each case of the table says it pins.
The largest emulation error / bound of each (case, dtype) is printed (pytest -s, or -rP) and never asserted beyond <= 1."""
import pytest
import torch

from tests.batchnorm_cases import (ACTS, BF16_K, BF16_OFFSET, BF16_STEP, BN_COLS, BN_WAVES, BY_NAME, CASES, DT, EPS, MOMENTUM,
                                   TRAIN_CASES, U, UB16, act64, bound_bwd, bound_fwd, geometry, is_offset, make_inputs, n_adds,
                                   reference_bwd, reference_fwd, saved_stats, violations)

F32 = torch.float32


def _t(v):
    return torch.tensor(v, dtype=F32)


def wave_sum(terms, mutant=None):
    """[B, C] fp32 -> [C]: the kernel's column sum, in its order"""
    B, C = terms.shape
    acc = torch.zeros(BN_WAVES, C, dtype=F32)
    rows = BN_WAVES * (B // BN_WAVES) if mutant == "drop_wave_tail" else B
    for b in range(rows):
        acc[b % BN_WAVES] += terms[b]
    return ((acc[0] + acc[1]) + acc[2]) + acc[3]


def act_bwd32(act, a):
    """ib_act_bwd of csrc/ib_common.h in fp32"""
    if act == "relu":
        return (a > 0).to(F32)
    if act == "tanh":
        return 1 - a * a
    if act == "sigmoid":
        return a * (1 - a)
    if act == "elu":
        return torch.where(a > 0, torch.ones_like(a), a + 1)
    if act == "silu":
        s = 1 / (1 + torch.exp(-a))
        return s * (1 + a * (1 - s))
    raise KeyError(act)


def emulate_fwd(inp, dt, training, mutant=None):
    x, g, bt = inp.x.float(), inp.gamma, inp.beta
    rm, rv = inp.running_mean.clone(), inp.running_var.clone()
    B = x.shape[0]
    m, eps = _t(MOMENTUM), _t(EPS)
    if training or mutant == "eval_uses_batch_stats":
        mean = wave_sum(x, mutant) / B
        if mutant == "one_pass_var":
            ss = wave_sum(x * x, mutant) - B * mean * mean
        else:
            d = x - mean
            ss = wave_sum(d * d, mutant)
        var = ss / B
        rstd = 1 / torch.sqrt(var if mutant == "rstd_without_eps" else var + eps)
        if training:
            rm = (1 - m) * rm + m * mean
            rv = (1 - m) * rv + m * (ss / (B if mutant == "biased_running_var" else B - 1))
    else:
        mean = rm
        rstd = 1 / torch.sqrt(rv if mutant == "rstd_without_eps" else rv + eps)
    y = ((x - mean) * rstd * g + bt).to(DT[dt])
    assert all(t.dtype == F32 for t in (mean, rstd, rm, rv))
    return {"y": y, "save_mean": mean, "save_rstd": rstd, "running_mean": rm, "running_var": rv}


def emulate_bwd(inp, dt, training, act, save_mean, save_rstd, accumulate=False, mutant=None):
    x, d, g = inp.x.float(), inp.dy.float(), inp.gamma
    B = x.shape[0]
    xh = (x - save_mean) * save_rstd
    tg = wave_sum(d if mutant == "dgamma_from_dy_only" else d * xh, mutant)
    tb = wave_sum(d, mutant)
    k, invB = g * save_rstd, _t(1.0) / _t(float(B))
    if training and mutant != "dx_without_mean_terms":
        v = k * (d - invB * (tb + xh * tg))
    else:
        v = k * d
    if act != "none":
        a = inp.aux[act].float()
        if mutant == "act_from_wrong_operand" and act == "silu":
            a = a / (1 + torch.exp(-a))                             # the derivative taken from the OUTPUT silu(z)
        v = v * act_bwd32(act, a)
    if accumulate and mutant != "accumulate_overwrites":
        tg, tb = inp.dgamma_old + tg, inp.dbeta_old + tb
    assert all(t.dtype == F32 for t in (v, tg, tb))
    return {"dx": v.to(DT[dt]), "dgamma": tg, "dbeta": tb}


def _check(got, ref, bnd, tag):
    """-> (messages, worst ratio)"""
    msgs, worst = [], 0.0
    for k in ref:
        msg, r = violations(f"{tag} {k}", got[k], ref[k], bnd[k])
        worst = max(worst, r)
        if msg:
            msgs.append(msg)
    return msgs, worst


def _forward_runs(c, dt, mutant=None):
    inp = make_inputs(c, dt)
    for training in ((True, False) if c.B > 1 else (False,)):
        yield (inp, training, emulate_fwd(inp, dt, training, mutant), reference_fwd(inp, training), bound_fwd(inp, dt, training))


def _backward_runs(c, dt, mutant=None, acts=ACTS, accumulate=(False, True)):
    inp = make_inputs(c, dt)
    for training in ((True, False) if c.B > 1 else (False,)):
        sm, sr = saved_stats(inp, training)
        for act in acts:
            for acc in accumulate:
                yield (training, act, acc, emulate_bwd(inp, dt, training, act, sm, sr, acc, mutant),
                       reference_bwd(inp, training, act, sm, sr, acc), bound_bwd(inp, dt, training, act, sm, sr, acc))


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_emulation_is_inside_the_bound(c, dt):
    msgs, wf, wb = [], 0.0, 0.0
    for _, training, got, ref, bnd in _forward_runs(c, dt):
        m, r = _check(got, ref, bnd, f"forward training={training}")
        msgs, wf = msgs + m, max(wf, r)
    for training, act, acc, got, ref, bnd in _backward_runs(c, dt):
        m, r = _check(got, ref, bnd, f"backward training={training} act={act} accumulate={acc}")
        msgs, wb = msgs + m, max(wb, r)
    print(f"emulation error / bound  {c.name:15s} {dt}  forward {wf:.3f}  backward {wb:.3f}")
    assert not msgs, "\n".join(msgs)


# mutant -> (direction, the outputs it may show in, [(case, dtype)] that must each catch it)
BOTH = lambda *names: [(n, dt) for n in names for dt in ("fp32", "bf16")]
MUTANTS = {
    "one_pass_var": ("fwd", ("save_rstd", "running_var", "y"), BOTH("offset", "offset_small_B")),
    "drop_wave_tail": ("fwd", ("save_mean", "save_rstd", "y"), BOTH("ragged_waves", "block_plus_one", "mid")),
    "biased_running_var": ("fwd", ("running_var",), BOTH("two_rows")),
    # eps = 1e-5 against var ~ 1e-4: 5 % of rstd; on unit-variance data it is 5e-6 and below the bf16 cases' e_mean
    "rstd_without_eps": ("fwd", ("save_rstd",), [("offset", "fp32"), ("offset_small_B", "fp32")]),
    "eval_uses_batch_stats": ("fwd", ("save_mean", "save_rstd", "y"), BOTH("two_rows", "mid", "offset")),
    "dx_without_mean_terms": ("bwd", ("dx",), BOTH("two_rows", "ragged_waves", "mid")),
    "dgamma_from_dy_only": ("bwd", ("dgamma", "dx"), BOTH("two_rows", "mid")),
    "act_from_wrong_operand": ("bwd", ("dx",), BOTH("three_rows", "mid")),
    "accumulate_overwrites": ("bwd", ("dgamma", "dbeta"), BOTH("two_rows", "block_plus_one")),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutant_is_outside_the_bound(mutant):
    direction, shows, where = MUTANTS[mutant]
    for name, dt in where:
        c = BY_NAME[name]
        caught, worst = set(), 0.0
        if direction == "fwd":
            for _, training, got, ref, bnd in _forward_runs(c, dt, mutant):
                for k in shows:
                    msg, r = violations(k, got[k], ref[k], bnd[k])
                    worst = max(worst, r)
                    if msg:
                        caught.add((training, k))
            if mutant == "eval_uses_batch_stats":
                assert any(not t for t, _ in caught), (mutant, name, dt)
        else:
            acts = ("silu",) if mutant == "act_from_wrong_operand" else ("none", "tanh")
            acc = (True,) if mutant == "accumulate_overwrites" else (False,)
            for training, act, _, got, ref, bnd in _backward_runs(c, dt, mutant, acts, acc):
                for k in shows:
                    msg, r = violations(k, got[k], ref[k], bnd[k])
                    worst = max(worst, r)
                    if msg:
                        caught.add((training, k))
            if mutant == "dx_without_mean_terms":
                assert all(t for t, _ in caught), "the eval form has no mean terms"
        print(f"{mutant:24s} {name:15s} {dt}  error / bound {worst:.3g}")
        assert caught, f"{mutant} stays inside the bound on {name} ({dt}): strengthen the inputs or the table, not S"


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_reference_is_torch_batch_norm_in_float64(c):
    """pins the restatement itself: forward, running statistics and the three gradients, training and eval"""
    rel = lambda a, b: float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)
    for dt in ("fp32", "bf16"):
        inp = make_inputs(c, dt)
        for training in ((True, False) if c.B > 1 else (False,)):
            x = inp.x.double().requires_grad_(True)
            g, bt = inp.gamma.double().requires_grad_(True), inp.beta.double().requires_grad_(True)
            rm, rv = inp.running_mean.double().clone(), inp.running_var.double().clone()
            y = torch.nn.functional.batch_norm(x, rm, rv, g, bt, training, MOMENTUM, EPS)
            ref = reference_fwd(inp, training)
            for k, t in (("y", y.detach()), ("running_mean", rm), ("running_var", rv)):
                assert rel(ref[k], t) <= 1e-12, (c.name, dt, training, k, rel(ref[k], t))
            y.backward(inp.dy.double())
            # the backward expressions of reference_bwd, on the float64 statistics themselves
            sm, sr = ref["save_mean"], ref["save_rstd"]
            X, D = inp.x.double(), inp.dy.double()
            xh = (X - sm) * sr
            tg, tb = (D * xh).sum(0), D.sum(0)
            dx = g.detach() * sr * ((D - (tb + xh * tg) / c.B) if training else D)
            for k, a, t in (("dx", dx, x.grad), ("dgamma", tg, g.grad), ("dbeta", tb, bt.grad)):
                scale = max(float(t.abs().max()), float((D.abs().sum(0) * sr).max()) * 1e-3)
                assert float((a - t).abs().max()) <= 1e-12 * scale, (c.name, dt, training, k)


def test_reference_bwd_matches_autograd_through_the_activation():
    """reference_bwd with act_below: autograd of batch_norm(act(z)) in float64, evaluated where the fp32 statistics ARE the
    float64 ones (eval mode with running statistics, which are fp32 operands) so the comparison is exact to roundoff"""
    c = BY_NAME["mid"]
    for dt in ("fp32", "bf16"):
        inp = make_inputs(c, dt)
        sm = inp.running_mean
        sr = (1 / torch.sqrt(inp.running_var.double() + EPS))
        for act in ACTS[1:]:
            aux = inp.aux[act].double()
            # a pre-activation whose activation is the stored aux: invert (relu / elu / tanh / sigmoid are monotone)
            if act == "silu":
                z = aux.clone().requires_grad_(True)
            elif act == "relu":
                z = torch.where(aux > 0, aux, -torch.ones_like(aux)).requires_grad_(True)
            elif act == "tanh":
                z = torch.atanh(aux.clamp(-1 + 1e-12, 1 - 1e-12)).requires_grad_(True)
            elif act == "sigmoid":
                z = torch.logit(aux.clamp(1e-12, 1 - 1e-12)).requires_grad_(True)
            else:
                z = torch.where(aux > 0, aux, torch.log1p(aux.clamp_min(-1 + 1e-12))).requires_grad_(True)
            a = torch.nn.functional.silu(z) if act == "silu" else act64(act, z)
            # x of the case is independent of aux in the kernel's eyes: feed the layer x, route the gradient through a
            y = torch.nn.functional.batch_norm(inp.x.double() + (a - a.detach()), sm.double(), inp.running_var.double(),
                                               inp.gamma.double(), inp.beta.double(), False, MOMENTUM, EPS)
            y.backward(inp.dy.double())
            # save_rstd in fp32 differs from sr by 2^-24: compare at that
            ref = reference_bwd(inp, False, act, sm, sr.float())
            ok = aux.abs() < 1 - 1e-6 if act in ("tanh",) else torch.ones_like(aux, dtype=torch.bool)
            if act == "sigmoid":
                ok = (aux > 1e-6) & (aux < 1 - 1e-6)
            if act == "elu":
                ok = aux > -1 + 1e-6
            err = ((ref["dx"] - z.grad).abs() * ok)
            assert float(err.max()) <= 1e-6 * float(z.grad.abs().max()), (dt, act, float(err.max()))


def test_table_is_what_it_says():
    assert len(BY_NAME) == len(CASES)
    for c in CASES:
        assert geometry(c.B, c.C) == c.geom, (c.name, geometry(c.B, c.C))
        assert c.ld >= c.C and n_adds(c.B) == max(c.geom[2]) + 3
        assert sum(c.geom[2]) == c.B and c.geom[0] == -(-c.C // BN_COLS)
    assert [c.name for c in CASES if c.B == 1] == ["eval_one_row"] and len(TRAIN_CASES) == len(CASES) - 1
    g = lambda n: BY_NAME[n]
    assert g("two_rows").geom[2] == (1, 1, 0, 0) and g("two_rows").B / (g("two_rows").B - 1) == 2
    assert g("three_rows").C == BN_COLS and g("three_rows").geom[2][3] == 0
    assert g("ragged_waves").geom[2] == (2, 2, 1, 1) and g("ragged_waves").C % BN_COLS and g("ragged_waves").ld > g("ragged_waves").C
    assert g("block_plus_one").geom[:2] == (2, 1)
    assert g("mid").geom[0] == 3 and g("mid").B % 4 == 1
    assert g("long").geom[2][0] == 258 and g("long").B * g("long").ld <= 1030 * 72
    assert {c.name for c in CASES if is_offset(c)} == {"offset", "offset_small_B"}
    assert any(c.ld > c.C for c in CASES) and any(c.ld == c.C for c in CASES)


def test_inputs_are_what_the_cases_need():
    for c in CASES:
        for dt in ("fp32", "bf16"):
            inp = make_inputs(c, dt)
            assert inp.x.dtype == inp.dy.dtype == DT[dt] and inp.gamma.dtype == torch.float32
            assert inp.gamma[0] < 0 and inp.gamma[-1] == 0 and (inp.gamma != 0).sum() == c.C - 1
            assert (inp.running_var > 0).all() and not torch.equal(inp.running_mean, torch.zeros(c.C))
            assert not torch.equal(inp.running_var, torch.ones(c.C))
            assert (inp.aux["relu"] == 0).any() and (inp.aux["relu"] > 0).any()
            if is_offset(c) and c.B > 1:
                x = inp.x.double()
                spread = x.std(0, unbiased=False)
                assert (spread > 0).all(), "a column collapsed to one value"
                assert (x.mean(0).abs() > 20 * spread).all(), "the offset is not large against the spread"
                if dt == "bf16":
                    k = (x - BF16_OFFSET) / BF16_STEP
                    assert torch.equal(k, k.round()) and k.abs().max() <= BF16_K
    assert U["bf16"] == UB16 == 2.0 ** -8
