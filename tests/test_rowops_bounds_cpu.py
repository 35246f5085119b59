"""The elementwise LayerNorm bound of tests/rowops_cases.py, checked without a GPU.

a. A torch-CPU emulation of csrc/rowops.hip's arithmetic in fp32 stays inside HALF of the bound on every case of the table,
   in every dtype of the case, forward and backward, plain, accumulating and through the fast kernels' own order: the
   bound admits a correct kernel.  The emulation keeps the kernel's summation order: a row is laid out over LPR lanes x CH
   chunks of 8 columns, a lane adds its 8 CH values in order, group_sum combines the lanes as a binary tree inside 16 lanes
   and as ((r0 + r1) + r2) + r3 across the four 16-lane rows of LPR = 64; the column sums go lane (one row per trip) ->
   shuffle tree over the rows of a wave -> 8 waves in order (16 in the fast kernel) -> `parts` partial rows ->
   segment_colsum's RL row lanes in the 4-way grouped order -> RL in order.
   CAP: the emulation (and only the emulation) skips the two largest loop-trip cases, fast_16387 and fast_16387_res
   (16387 x 512: a second of fp32 emulation and four of float64 bound each); their second trip is the same code as the
   first, which fast_4099 emulates, and the reference and bound of both are still evaluated by test_reference_alone.
b. Thirteen one-line bugs, applied to that emulation, fall outside the bound on NAMED cases (MUTANTS), in every dtype of
   the case.  The factor by which the worst element falls outside (error / bound; inf: a bound of exactly 0, or an output
   that is not finite), as test_mutants_fall_outside prints it, fp32 / bf16 storage:
     one_pass_var         offset_40 rstd      inf (var < 0) / 8.7   offset_520 rstd             inf / 13
     div_by_n_minus_1     width_8 mean        7.9e4 / 7.5e4         flags_264_none rstd         3.4e2 / 3.4e2
     eps_after_sqrt       const_row_256 rstd  inf / inf (1 / 0)     width_8 rstd                8.7 / 8.2
     drop_tail_chunk      width_129 mean      5.2e3 / 3.4e3         width_513 mean              1.2e3 / 1.2e3
     gamma_chunk_off      width_129 y         inf / inf             flags_40_none y             inf / inf   (the gamma = 0 column)
     drop_c1              flags_40_none dx    2.9e5 / 3.8e3         flags_520_silu_res dx       4.6e4 / 1.7e4
     c2_not_over_n        flags_40_none dx    4.9e6 / 2.2e5         flags_264_none dx           1.4e7 / 2.9e6
     elu_act_grad_one     flags_40_elu dx     1.8e7 / 1.3e4         flags_520_elu_dres dx       3.5e7 / 4.5e4   (dx ONLY)
     dres_times_act       flags_40_tanh_dres  5.4e5 / 1.3e2         flags_520_silu_res_dres     9.6e5 / 1.4e2
     add_row_mod_seg      add_div_vec_40 dx   2.2e6 / 5.1e4         add_div_odd_520 dx          3.2e6 / 3.7e5
     res_missing_in_h     flags_40_none_res dgamma 3.8e5 / 2.3e5    flags_264_silu_res_dres dx  5.6e4 / 1.2e4
     accumulate_ignored   flags_40_none dgamma 1.5e5 / 1.6e5        rows_lpr64_17 dbeta         1.7e5 / 1.3e5
     idle_block_unwritten rows_lpr16_17       inf / inf (NaN)       rows_lpr16_33               inf / inf
   elu_act_grad_one is the bug act_bwd_pre had (no ELU case: the derivative was taken as 1).
c. The reference alone (float64; no emulation, no GPU) is finite on every case, gives the exact values the table promises
   (constant rows, gamma = 0, dy = 0) and equals torch.nn.functional.layer_norm and its autograd in float64 to F64_AGREE
   (2^24 float64 roundings: the two differ in the order of their float64 operations only).
d. Every case's pins hold against ln_dispatch / ln_geometry, and the table reaches every instantiation it claims."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.rowops_cases import (BY_NAME, CASES, CONST_VALUE, DT, EPS, LN_BWD_WPB, LNF_ROWS, LNF_WAVES, PARAMS, Case,
                                bound_bwd, bound_fwd, case_id, colsum_adds, colsum_rl, dispatch_of, ln_bwd_parts, ln_dispatch,
                                ln_geometry, ln_table, make_inputs, pinned, reference_bwd, reference_fwd, saved_stats,
                                violations)

F32 = torch.float32
EMULATION_CAP = ("fast_16387", "fast_16387_res")
F64_AGREE = 2.0 ** 24 * 2.0 ** -53                                # two float64 evaluations of one formula


# ---- the emulation -----------------------------------------------------------------------------------------------------
def act32(act, z, mutant=None):
    """(ln_act_both's value, its derivative) in fp32"""
    one = torch.ones_like(z)
    if act == "none":
        return z, one
    if act == "relu":
        return z.clamp_min(0), (z > 0).to(F32)
    if act == "tanh":
        t = torch.tanh(z)
        return t, 1 - t * t
    if act == "sigmoid":
        s = 1 / (1 + torch.exp(-z))
        return s, s * (1 - s)
    if act == "silu":
        s = 1 / (1 + torch.exp(-z))
        return z * s, s * (1 + z * (1 - s))
    if act == "elu":
        E = torch.exp(z)
        return torch.where(z > 0, z, E - 1), (one if mutant == "elu_act_grad_one" else torch.where(z > 0, one, E))
    raise KeyError(act)


def prologue32(c, inp, mutant=None, with_res=True):
    z = inp.x.float()
    if inp.add is not None:
        rows = torch.arange(c.M)
        rows = rows % c.seg if mutant == "add_row_mod_seg" else rows // c.seg
        z = z + inp.add.float()[rows.clamp_max(inp.add.shape[0] - 1)]
    t, f = act32(c.act, z, mutant)
    if inp.res is not None and with_res:
        t = t + inp.res.float()
    return t, f


def lanes(t, LPR, CH):
    """[M, N] -> [M, CH, LPR, 8]: chunk c of lane l holds the columns (c LPR + l) 8 ..., zeros past N"""
    M, N = t.shape
    assert N <= CH * LPR * 8
    return F.pad(t, (0, CH * LPR * 8 - N)).reshape(M, CH, LPR, 8)


def row_sum(t4):
    """[M, CH, LPR, 8] -> [M]: the lane's serial sum, then group_sum<LPR>"""
    M, CH, LPR, _ = t4.shape
    s = torch.zeros(M, LPR, dtype=F32)
    for c in range(CH):
        for e in range(8):
            s = s + t4[:, c, :, e]
    k = s.reshape(M, LPR // 16, 16)
    for _ in range(4):
        k = k[..., 0::2] + k[..., 1::2]
    k = k[..., 0]
    return ((k[:, 0] + k[:, 1]) + k[:, 2]) + k[:, 3] if LPR == 64 else k[:, 0]


def colsum_emul(x):
    """segment_colsum_kernel over the cnt rows of one segment: [cnt, N] -> [N]"""
    cnt, N = x.shape
    RL = colsum_rl(cnt)
    t = torch.zeros(N, dtype=F32)
    for rl in range(RL):
        acc, r = torch.zeros(N, dtype=F32), rl
        while r + 3 * RL < cnt:
            acc = acc + ((x[r] + x[r + RL]) + (x[r + 2 * RL] + x[r + 3 * RL]))
            r += 4 * RL
        while r < cnt:
            acc = acc + x[r]
            r += RL
        t = t + acc
    return t


def col_sum(terms, kernel, LPR, mutant=None):
    """[M, N] -> [N]: the backward's column sum through the partial rows"""
    M, N = terms.shape
    g = ln_geometry("bwd", kernel, LPR, M)
    parts, T = g["blocks"], g["trips"]
    padded = F.pad(terms, (0, 0, 0, T * g["rows_per_trip"] - M))
    if kernel == "fast512":
        r = padded.reshape(T * LNF_ROWS, parts, LNF_WAVES, N)
        acc = torch.zeros(parts, LNF_WAVES, N, dtype=F32)
        for t in range(T * LNF_ROWS):
            acc = acc + r[t]
        own = LNF_WAVES
    else:
        RPW = 64 // LPR
        r = padded.reshape(T, parts, LN_BWD_WPB, RPW, N)
        acc = torch.zeros(parts, LN_BWD_WPB, RPW, N, dtype=F32)
        for t in range(T):
            acc = acc + r[t]
        while acc.shape[2] > 1:
            acc = acc[:, :, 0::2] + acc[:, :, 1::2]
        acc = acc[:, :, 0]
        own = LN_BWD_WPB * RPW
    partial = torch.zeros(parts, N, dtype=F32)
    for w in range(acc.shape[1]):
        partial = partial + acc[:, w]
    if mutant == "idle_block_unwritten":
        for b in range(parts):
            if b * own >= M:
                partial[b] = float("nan")                            # what the poisoned workspace held
    return colsum_emul(partial)


def emulate_fwd(c, inp, dt, disp=None, mutant=None):
    _, LPR, CH = (disp or dispatch_of(c, "fwd", dt))[:3]
    N = c.N
    v, _ = prologue32(c, inp, mutant)
    live = lanes(torch.ones(1, N), LPR, CH) > 0
    v4 = lanes(v, LPR, CH)
    invN = torch.tensor(1.0, dtype=F32) / torch.tensor(float(N - 1 if mutant == "div_by_n_minus_1" else N), dtype=F32)
    s4 = v4
    if mutant == "drop_tail_chunk":
        s4 = lanes(F.pad(v[:, :(N // 8) * 8], (0, N - (N // 8) * 8)), LPR, CH)
    mu = row_sum(s4) * invN
    if mutant == "one_pass_var":
        var = row_sum(v4 * v4) * invN - mu * mu
    else:
        d = torch.where(live, v4 - mu[:, None, None, None], torch.zeros_like(v4))
        var = row_sum(d * d) * invN
    eps = torch.tensor(EPS, dtype=F32)
    rs = 1 / torch.sqrt(var) + eps if mutant == "eps_after_sqrt" else 1 / torch.sqrt(var + eps)
    gm = inp.gamma
    if mutant == "gamma_chunk_off":
        gm = torch.roll(gm, -8)
    y = ((v - mu[:, None]) * rs[:, None] * gm + inp.beta).to(DT[dt])
    assert mu.dtype == rs.dtype == F32
    return {"y": y, "mean": mu, "rstd": rs}


def emulate_bwd(c, inp, dt, mean, rstd, accumulate=False, disp=None, mutant=None):
    kernel, LPR, CH = (disp or dispatch_of(c, "bwd", dt))[:3]
    N = c.N
    v, f = prologue32(c, inp, mutant, with_res=mutant != "res_missing_in_h")
    dy, gm = inp.dy.float(), inp.gamma
    invN = torch.tensor(1.0, dtype=F32) / torch.tensor(float(N), dtype=F32)
    h = (v - mean[:, None]) * rstd[:, None]
    g = dy * gm
    c1 = row_sum(lanes(g, LPR, CH)) * invN
    c2 = row_sum(lanes(g * h, LPR, CH))
    if mutant != "c2_not_over_n":
        c2 = c2 * invN
    if mutant == "drop_c1":
        c1 = torch.zeros_like(c1)
    dv = (g - c1[:, None] - h * c2[:, None]) * rstd[:, None]
    dx = dv * f
    dg, db = col_sum(dy * h, kernel, LPR, mutant), col_sum(dy, kernel, LPR, mutant)
    if accumulate and mutant != "accumulate_ignored":
        dg, db = inp.dgamma_old + dg, inp.dbeta_old + db
    assert all(t.dtype == F32 for t in (dx, dv, dg, db))
    return {"dx": dx.to(DT[dt]), "dres": (dx if mutant == "dres_times_act" else dv).to(DT[dt]), "dgamma": dg, "dbeta": db}


def _check(got, ref, bnd, tag, keys=None, scale=1.0):
    """-> (messages, {key: worst ratio})"""
    msgs, worst = [], {}
    for k in (keys or ref):
        msg, r = violations(f"{tag} {k}", got[k], ref[k], bnd[k] * scale)
        worst[k] = r
        if msg:
            msgs.append(msg)
    return msgs, worst


def _runs(c, dt, mutant=None, accumulate=(False, True)):
    """(tag, emulation, reference, bound) of the forward and of the backward(s) of a case"""
    inp = make_inputs(c, dt)
    yield "fwd", emulate_fwd(c, inp, dt, mutant=mutant), reference_fwd(c, inp, dt), bound_fwd(c, inp, dt)
    mean, rstd = saved_stats(c, inp, dt)
    for acc in accumulate:
        yield ("bwd" + ("+acc" if acc else ""), emulate_bwd(c, inp, dt, mean, rstd, acc, mutant=mutant),
               reference_bwd(c, inp, dt, mean, rstd, acc), bound_bwd(c, inp, dt, mean, rstd, acc))


# ---- a. the bound admits the emulation ---------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [p for p in PARAMS if p[0].name not in EMULATION_CAP], ids=case_id)
def test_emulation_within_half_the_bound(p):
    c, dt = p
    worst = 0.0
    for tag, got, ref, bnd in _runs(c, dt):
        msgs, w = _check(got, ref, bnd, f"{c.name} {dt} {tag}", scale=0.5)
        assert not msgs, "\n".join(msgs)
        worst = max(worst, *w.values())
    print(f"emulation error / bound  {c.name:34s} {dt}  {worst / 2:.3f}")


def test_generic_order_on_the_fast_shape():
    """the four non-qualifying cases run the generic kernels at the fast shape; and the fast rows in the generic order"""
    c = BY_NAME["fast_4099_res"]
    inp = make_inputs(c, "bf16")
    mean, rstd = saved_stats(c, inp, "bf16")
    for direction in ("fwd", "bwd"):
        disp = ("generic",) + ln_table(direction, c.N)
        if direction == "fwd":
            got, ref, bnd = emulate_fwd(c, inp, "bf16", disp), reference_fwd(c, inp, "bf16"), bound_fwd(c, inp, "bf16", disp)
        else:
            got = emulate_bwd(c, inp, "bf16", mean, rstd, disp=disp)
            ref, bnd = reference_bwd(c, inp, "bf16", mean, rstd), bound_bwd(c, inp, "bf16", mean, rstd, dispatch=disp)
        msgs, _ = _check(got, ref, bnd, f"generic order {direction}", scale=0.5)
        assert not msgs, "\n".join(msgs)


# ---- b. the bound has teeth --------------------------------------------------------------------------------------------
MUTANTS = {   # mutant: (the cases it must fall outside on, the outputs that must show it)
    "one_pass_var": (("offset_40", "offset_520"), ("rstd", "y")),
    "div_by_n_minus_1": (("width_8", "flags_264_none"), ("mean", "rstd", "y")),
    "eps_after_sqrt": (("const_row_256", "width_8"), ("rstd",)),
    "drop_tail_chunk": (("width_129", "width_513"), ("mean", "y")),
    "gamma_chunk_off": (("width_129", "flags_40_none"), ("y",)),
    "drop_c1": (("flags_40_none", "flags_520_silu_res"), ("dx",)),
    "c2_not_over_n": (("flags_40_none", "flags_264_none"), ("dx",)),
    "elu_act_grad_one": (("flags_40_elu", "flags_264_elu_res_dres", "flags_520_elu_dres"), ("dx",)),
    "dres_times_act": (("flags_40_tanh_dres", "flags_520_silu_res_dres"), ("dres",)),
    "add_row_mod_seg": (("add_div_vec_40", "add_div_odd_520"), ("y", "dx")),
    "res_missing_in_h": (("flags_40_none_res", "flags_264_silu_res_dres"), ("dx", "dgamma")),
    "accumulate_ignored": (("flags_40_none", "rows_lpr64_17"), ("dgamma", "dbeta")),
    "idle_block_unwritten": (("rows_lpr16_17", "rows_lpr16_33"), ("dgamma", "dbeta")),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutants_fall_outside(mutant):
    names, keys = MUTANTS[mutant]
    for name in names:
        c = BY_NAME[name]
        for dt in c.dts:
            worst = {}
            for tag, got, ref, bnd in _runs(c, dt, mutant):
                if mutant == "accumulate_ignored" and not tag.endswith("+acc"):
                    continue
                _, w = _check(got, ref, bnd, tag)
                for k, r in w.items():
                    worst[k] = max(worst.get(k, 0.0), r)
            seen = {k: worst[k] for k in keys if k in worst}
            print(f"mutant {mutant:22s} {name:28s} {dt}  " + "  ".join(f"{k} {r:.1e}" for k, r in seen.items()))
            assert seen and max(seen.values()) > 1, f"{mutant} stays inside the bound on {name} {dt}: {worst}"
            if mutant == "elu_act_grad_one":                         # the bug the kernel had: dx, and nothing else
                assert all(r <= 1 for k, r in worst.items() if k != "dx"), worst


def test_mutants_named_in_the_issue_are_all_here():
    assert len(MUTANTS) == 13
    for names, _ in MUTANTS.values():
        assert all(n in BY_NAME for n in names)
    assert {"width_129", "width_513"} == set(MUTANTS["drop_tail_chunk"][0])


# ---- c. the reference alone --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", PARAMS, ids=case_id)
def test_reference_alone(p):
    c, dt = p
    inp = make_inputs(c, dt)
    ref, bnd = reference_fwd(c, inp, dt), bound_fwd(c, inp, dt)
    mean, rstd = saved_stats(c, inp, dt)
    rb, bb = reference_bwd(c, inp, dt, mean, rstd), bound_bwd(c, inp, dt, mean, rstd)
    for d in (ref, bnd, rb, bb):
        for k, t in d.items():
            assert torch.isfinite(t).all() and t.dtype == torch.float64, (c.name, k)
    for d in (bnd, bb):
        assert all((t >= 0).all() for t in d.values())
    # the reference rounded to the storage dtype is inside its own bound (the storage term alone covers it)
    assert violations("y", ref["y"].to(DT[dt]), ref["y"], bnd["y"])[0] is None
    assert violations("dx", rb["dx"].to(DT[dt]), rb["dx"], bb["dx"])[0] is None
    zero_g = inp.gamma == 0
    assert torch.equal(ref["y"][:, zero_g], inp.beta.double()[zero_g].expand(c.M, -1)) and (bnd["y"][:, zero_g] == 0).all()
    if c.values == "const":
        assert (ref["mean"] == CONST_VALUE).all() and (ref["rstd"] == 1 / math.sqrt(EPS)).all()
        assert torch.equal(ref["y"], inp.beta.double().expand(c.M, -1))
    if c.values == "gamma0":
        assert (rb["dx"] == 0).all() and (bb["dx"] == 0).all() and (rb["dres"] == 0).all() and (bb["dres"] == 0).all()
    if c.values == "dy0":
        assert all((rb[k] == 0).all() and (bb[k] == 0).all() for k in rb)
    if c.M > 64:
        return
    # against torch's own layer norm and autograd, in float64
    x = inp.x.double().requires_grad_()
    leaves = [x]
    z = x
    if inp.add is not None:
        a = inp.add.double().requires_grad_()
        z = x + a[torch.arange(c.M) // c.seg]
    t = {"none": lambda q: q, "silu": F.silu, "relu": F.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid, "elu": F.elu}[c.act](z)
    r = inp.res.double().requires_grad_() if inp.res is not None else None
    v = t + r if r is not None else t
    gm, bt = inp.gamma.double().requires_grad_(), inp.beta.double().requires_grad_()
    y = F.layer_norm(v, (c.N,), gm, bt, EPS)
    assert torch.allclose(y, ref["y"], rtol=F64_AGREE, atol=F64_AGREE)
    # the backward reference on the reference's own (float64) statistics, so that it IS the gradient
    y.backward(inp.dy.double())
    mu64, rs64 = ref["mean"][:, None], ref["rstd"][:, None]
    h = (v.detach() - mu64) * rs64
    g = inp.dy.double() * inp.gamma.double()
    dv = (g - g.mean(1, keepdim=True) - h * (g * h).mean(1, keepdim=True)) * rs64
    if r is not None:
        assert torch.allclose(r.grad, dv, rtol=F64_AGREE, atol=F64_AGREE)
    assert torch.allclose(gm.grad, (inp.dy.double() * h).sum(0), rtol=F64_AGREE, atol=F64_AGREE)
    assert torch.allclose(bt.grad, inp.dy.double().sum(0), rtol=F64_AGREE, atol=F64_AGREE)
    # reference_bwd, handed those float64 statistics instead of their fp32 roundings, IS the gradient
    exact = reference_bwd(c, inp, dt, ref["mean"], ref["rstd"])
    assert torch.allclose(exact["dx"], x.grad, rtol=F64_AGREE, atol=F64_AGREE)
    assert torch.allclose(exact["dres"], dv, rtol=F64_AGREE, atol=F64_AGREE)
    assert torch.allclose(exact["dgamma"], gm.grad, rtol=F64_AGREE, atol=F64_AGREE)


# ---- d. pins and coverage ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_pins(c):
    assert isinstance(c, Case) and c.pins
    for dt in c.dts:
        have = pinned(c, dt)
        for k, want in c.pins.items():
            if k in ("vec32", "vec16") and k not in have:
                continue                                             # the other dtype's flag
            assert k in have and have[k] == want, f"{c.name} {dt}: pins {k} = {want}, the dispatch gives {have.get(k)}"


def test_coverage_of_the_table():
    reached = {(d, dt): set() for d in ("fwd", "bwd") for dt in ("fp32", "bf16")}
    flags = {(d, dt): set() for d in ("fwd", "bwd") for dt in ("fp32", "bf16")}
    kernels, trips, acts = set(), set(), set()
    for c in CASES:
        for dt in c.dts:
            for d in ("fwd", "bwd"):
                k, LPR, CH, tmpl, vec, vecp = dispatch_of(c, d, dt)
                g = ln_geometry(d, k, LPR, c.M)
                if k == "generic":
                    reached[d, dt].add((LPR, CH))
                    flags[d, dt] |= {("vec", vec), ("vecp", vecp)}
                    trips.add((d, LPR, min(g["trips"], 2)))
                    acts.add((d, tmpl))
                else:
                    trips.add((d, "fast", min(g["trips"], 2)))
                kernels.add((d, dt, k))
    want = {"fwd": {(16, 1), (16, 2), (16, 4), (64, 2), (64, 4)}, "bwd": {(16, 1), (16, 2), (64, 1), (64, 2), (64, 4)}}
    for (d, dt), got in reached.items():
        print(f"reached {d} {dt}: {sorted(got)}  flags {sorted(flags[d, dt])}")
        assert got == want[d], (d, dt, got)
        assert flags[d, dt] == {("vec", 0), ("vec", 1), ("vecp", 0), ("vecp", 1)}, (d, dt, flags[d, dt])
    assert {("fwd", "bf16", "fast512"), ("bwd", "bf16", "fast512")} <= kernels
    assert {("fwd", 16, 2), ("fwd", 64, 2), ("bwd", 16, 2), ("bwd", 64, 2), ("bwd", "fast", 2)} <= trips
    assert {(d, t) for d in ("fwd", "bwd") for t in (0, 4, -1)} <= acts
    # both sides of every boundary of both tables, and every N % 8 class
    widths = {c.N for c in CASES if c.name.startswith("width_")}
    assert {128, 129, 256, 257, 512, 513, 1024, 1025, 2048} <= widths
    assert {n % 8 for n in widths} >= {0, 4, 1}
    # idle backward blocks, and blocks with rows, in one launch
    assert any(pinned(c, "fp32")["bwd_idle"] > 0 for c in CASES if "fp32" in c.dts)


def test_dispatch_restated():
    assert [ln_bwd_parts(m) for m in (1, 16, 17, 4096, 4097, 10 ** 6)] == [1, 1, 2, 256, 256, 256]
    assert ln_dispatch("fwd", "bf16", 4096, 512) == ("fast512", 64, 1, 0, 1, 1)
    assert ln_dispatch("fwd", "bf16", 4095, 512) == ("generic", 16, 4, 0, 1, 1)
    assert ln_dispatch("bwd", "bf16", 4096, 512, has_dres=True) == ("generic", 64, 1, 0, 1, 1)
    assert ln_dispatch("fwd", "bf16", 4096, 512, has_dres=True)[0] == "fast512"
    assert ln_dispatch("bwd", "fp32", 4096, 512)[0] == "generic"
    assert ln_dispatch("bwd", "bf16", 4096, 512, act="relu")[:4] == ("generic", 64, 1, -1)
    assert ln_dispatch("fwd", "fp32", 5, 12)[4:] == (1, 1) and ln_dispatch("fwd", "bf16", 5, 12)[4:] == (0, 1)
    assert ln_dispatch("fwd", "fp32", 5, 40, has_add=True, ld_add=49)[4] == 0
    with pytest.raises(ValueError):
        ln_dispatch("fwd", "fp32", 5, 2049)
    assert ln_geometry("fwd", "generic", 16, 32771) == {"blocks": 2048, "rows_per_trip": 32768, "trips": 2, "idle": 0}
    assert ln_geometry("bwd", "fast512", 64, 16387)["rows_per_trip"] == 16384
    assert ln_geometry("bwd", "generic", 16, 17) == {"blocks": 2, "rows_per_trip": 64, "trips": 1, "idle": 1}
    assert [colsum_rl(r) for r in (32, 33)] == [4, 16] and colsum_adds(256) == 32 and colsum_adds(5) == 6
