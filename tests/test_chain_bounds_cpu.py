"""The checks of tests/chain_cases.py, checked without a GPU.

a. The restated geometry equals the C query functions (the library loads on the CPU): ib_mlp_chain_supported,
   ib_mlp_chain_packed_elems and ib_mlp_chain_partial_width for every D % 4 == 0 up to 516 (and the odd widths around the
   edges), H in {64, 128, 256, 512, 1024}, L = 0 ... 5; ib_mlp_chain_workgroups for M = 1 ... 20000.  Every case reaches the
   instantiation, the panel height, the last panel and the e path(s) it names, and the table reaches every item of the list
   the case table was built for (test_the_table_reaches_every_edge spells the list out).
b. The bound admits a correct kernel: an fp32 emulation of the kernel's arithmetic (emulate) -- bf16 where the kernel stores
   or stages bf16, the row sums in the kernel's grouping (even / odd columns per lane, then the DPP tree; 8 in sequence per
   lane in the backward), the column sums per lane over its rows, then across a wave's row groups, then in wave order,
   torch.sigmoid in fp32 for exp + rcp, unfused multiply-adds where the compiler may fuse -- passes check() on every case.
   The three P = 64 cases are emulated on their first, one middle and their last panel.  The worst error / bound per stage
   is printed.
c. check() rejects one-line bugs: the issue's seventeen bugs as the eighteen mutants of MUTANTS (gamma and beta shifted count
   once each), every one on its NAMED cases, must fail, and the same cases pass without the bug."""
import ctypes
import math

import pytest
import torch

from tests.chain_cases import (BF, BY_NAME, CASES, CH_NWIN, F32, GR, LARGE, LN_EPS, REFUSED, TABLE_ROWS, alloc, body, case_id,
                               chain_shape, check, dp16_form, emulated_panels, geometry, gscale32, layout, make_inputs,
                               packed_elems, panel_info, panels_of, partial_columns, partial_width, supported, up8, workgroups,
                               zero_rows)


# ---- the emulation -----------------------------------------------------------------------------------------------------------
def bf(t):
    return t.to(BF).to(F32)


def tree(t):
    """group_sum: the DPP levels pair neighbours, then pairs of pairs ... (the last dimension is a power of two)"""
    while t.shape[-1] > 1:
        t = t[..., 0::2] + t[..., 1::2]
    return t[..., 0]


def seq(t, dim):
    """a sum in sequence along dim"""
    parts = t.unbind(dim)
    s = parts[0]
    for p in parts[1:]:
        s = s + p
    return s


def colsum(x, H):
    """dgamma | dbeta | dbias of bwd_layer: x [np, 64, H], zero in the rows beyond the panel; row r = RSTEP j + RPW wave + sub"""
    rpw = 512 // H
    x = x.view(x.shape[0], 64 // (8 * rpw), 8, rpw, H)
    s = seq(x, 1)                                                   # per lane over its rows j          [np, 8, rpw, H]
    s = tree(s.transpose(2, 3))                                     # the row groups of a wave          [np, 8, H]
    return seq(s, 1)                                                # wave order                        [np, H]


def emulate(c, inp, bug=None, panels=None):
    """-> the output buffers of alloc(c), filled as the kernel fills them, in fp32 arithmetic (see the module docstring)"""
    g = geometry(c)
    M, D, H, L, T, P = g.M, c.D, c.H, c.L, c.T, g.P
    outs = alloc(c)
    pan = list(range(g.nwg)) if panels is None else panels
    info = [panel_info(M, T, j) for j in pan]
    r0 = torch.tensor([i[0] for i in info])
    nrows = torch.tensor([i[1] for i in info])
    nwin = torch.tensor([i[3] for i in info])
    r = torch.arange(64)
    valid = r[None, :] < nrows[:, None]                             # [np, 64]
    rc = r0[:, None] + torch.minimum(r[None, :], nrows[:, None] - 1)    # rows beyond the panel: the clamped duplicate
    rows_v = rc[valid]
    LPR = H // 8
    invH = torch.tensor(1.0 / H, dtype=F32)

    def store(name, val):
        body(c, outs, name)[rows_v] = val[valid].to(outs[name].dtype)

    # q_sample
    k = inp["t"][rc // T]
    k = k % TABLE_ROWS if bug == "t_noclamp" else k.clamp(0, TABLE_ROWS - 1)
    cx, cy = inp["sab"][k][..., None], inp["s1m"][k][..., None]
    x0, eps = inp["x0"].view(M, D)[rc].float(), inp["eps"].view(M, D)[rc].float()
    xt = bf(cx * x0 + cy * eps)
    store("xt", xt)
    if bug == "dup_row" and pan[-1] == g.nwg - 1:                   # the last panel's clamped duplicate row, stored past M
        outs["xt"][GR + M, :D] = xt[-1, 63].to(BF)

    # forward
    win = rc // T
    last_win = (r0 + nrows - 1) // T
    us, hs, stats = [], [], []
    cur = xt
    for i in range(L):
        z = cur @ inp["W"][i].float().T
        w = torch.minimum(win + 1, last_win[:, None]) if bug == "e_neighbour" else win
        blk = 0 if bug == "e_block0" else i
        er = inp["e"][w, blk * H:(blk + 1) * H].float()
        if bug == "e_unstaged_dropped":
            er = torch.where((nwin > CH_NWIN)[:, None, None], torch.zeros_like(er), er)
        b = torch.zeros(H) if bug == "no_bias" else inp["bias"][i]
        u = bf((z + b) + er)
        sg = torch.sigmoid(u)
        v = u * sg
        x8 = v.view(-1, 64, LPR, 8)
        a0 = ((x8[..., 0] + x8[..., 2]) + x8[..., 4]) + x8[..., 6]
        a1 = ((x8[..., 1] + x8[..., 3]) + x8[..., 5]) + x8[..., 7]
        q8 = x8 * x8
        q0 = ((q8[..., 0] + q8[..., 2]) + q8[..., 4]) + q8[..., 6]
        q1 = ((q8[..., 1] + q8[..., 3]) + q8[..., 5]) + q8[..., 7]
        mean = (tree(a0 + a1) * invH)[..., None]
        inv2 = torch.tensor(1.0 / (H - 1), dtype=F32) if bug == "var_h1" else invH
        var = (tree(q0 + q1)[..., None] * inv2 - mean * mean).clamp_min(0)
        rstd = torch.rsqrt(var + torch.tensor(0.0 if bug == "no_eps" else LN_EPS, dtype=F32))
        gm = inp["gamma"][i].roll(8) if bug == "gamma_shift" else inp["gamma"][i]
        bt = inp["beta"][i].roll(8) if bug == "beta_shift" else inp["beta"][i]
        h = bf((v - mean) * rstd * gm + bt)
        store(f"u{i}", u)
        store(f"h{i}", h)
        us.append(u)
        stats.append((mean, rstd))
        cur = h

    # head, loss, dpred
    cols = partial_columns(D, H, L)
    prow = torch.zeros(len(pan), g.width, dtype=F32)
    hb = torch.zeros(D) if bug == "no_head_bias" else inp["bias"][L]
    pred = bf(cur @ inp["W"][L].float().T + hb)
    d = pred - eps
    sq = torch.where(valid[..., None], d * d, torch.zeros_like(d))
    lsum = sq.sum((1, 2))
    if bug == "loss_pad":                                           # the image columns D .. 128 ntd - 1 hold the last block's u
        pad = us[-1][:, :, D:min(g.DN, H)]
        lsum = lsum + torch.where(valid[..., None], pad * pad, torch.zeros_like(pad)).sum((1, 2))
    gs = torch.tensor(1.0 / (M * D) if bug == "gscale" else gscale32(M, D), dtype=F32)
    dp = bf(d * gs)
    dpv = dp if bug == "colsum_rows" else torch.where(valid[..., None], dp, torch.zeros_like(dp))
    cs = seq(dpv.view(-1, 4, 16, D), 1)                             # per lane over the 4 m-tiles
    prow[:, cols["head"]:cols["head"] + D] = tree(cs.transpose(1, 2))
    prow[:, cols["loss"]] = lsum
    store("dpred", dp)
    if dp16_form(c) and up8(D) > D:
        c0 = layout(c)["dpred"][1]
        outs["dpred"][GR + rows_v, c0 + D:c0 + up8(D)] = 0

    # backward
    gk = dp
    for i in range(L - 1, -1, -1):
        if i == L - 1:
            Wm = inp["W"][L]
        elif bug == "wrong_wt":
            Wm = inp["W"][(i + 1) % (L - 1) + 1]
        else:
            Wm = inp["W"][i + 1]
        dh = gk @ Wm.float()
        mean, rstd = stats[i]
        dd = torch.where(valid[..., None], dh, torch.zeros_like(dh))
        xx = torch.where(valid[..., None], us[i], torch.zeros_like(dh))
        sg = torch.sigmoid(xx)
        v = xx * sg
        ds = sg * (1 - sg) if bug == "silu_grad" else sg * (1 + xx * (1 - sg))
        xh = (v - mean) * rstd
        dxh = dd * inp["gamma"][i]
        sa = tree(seq(dxh.view(-1, 64, LPR, 8), 3))[..., None]
        sb = tree(seq((dxh * xh).view(-1, 64, LPR, 8), 3))[..., None]
        ma = torch.zeros_like(sa) if bug == "no_ma" else sa * invH
        mb = sb * invH
        dz = bf(rstd * (dxh - ma - xh * mb) * ds)
        zr = torch.where(valid[..., None], dz, torch.zeros_like(dz))
        dgam, dbet, dbs = colsum(dd * xh, H), colsum(dd, H), colsum(zr, H)
        prow[:, cols["dgamma"][i]:cols["dgamma"][i] + H] = dgam
        prow[:, cols["dbeta"][i]:cols["dbeta"][i] + H] = dbet
        prow[:, cols["dbias"][i]:cols["dbias"][i] + H] = dbs
        if c.de_lp:
            body(c, outs, "de_lp")[torch.tensor(pan), i * H:(i + 1) * H] = (dbet if bug == "de_from_dbeta" else dbs).to(BF)
        store(f"dz{i}", dz)
        gk = dz
    # the three floats behind the squared-error sum are never written
    keep = body(c, outs, "partial")[torch.tensor(pan), cols["loss"] + 1:].clone()
    body(c, outs, "partial")[torch.tensor(pan)] = prow
    body(c, outs, "partial")[torch.tensor(pan), cols["loss"] + 1:] = keep
    return outs


# ---- a. geometry -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from inferbiomechanics_amd import hip
    return hip.lib()


def test_geometry_equals_the_c_query_functions(lib):
    widths = sorted(set(range(0, 520, 4)) | {1, 2, 3, 5, 6, 63, 65, 127, 129, 255, 257, 319, 321, 383, 385, 511, 513, -4})
    for H in (64, 128, 256, 512, 1024):
        for D in widths:
            for L in range(0, 6):
                assert bool(lib.ib_mlp_chain_supported(D, H, L)) == supported(D, H, L), (D, H, L)
                assert int(lib.ib_mlp_chain_packed_elems(D, H, L)) == packed_elems(D, H, L), (D, H, L)
                assert int(lib.ib_mlp_chain_partial_width(D, H, L)) == partial_width(D, H, L), (D, H, L)
    p = ctypes.c_int(0)
    ref = ctypes.cast(ctypes.pointer(p), ctypes.c_void_p)
    for M in range(1, 20001):
        assert (int(lib.ib_mlp_chain_workgroups(M, ref)), p.value) == workgroups(M), M
    for D, H, L in REFUSED:
        assert not supported(D, H, L) and not lib.ib_mlp_chain_supported(D, H, L)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_case_reaches_what_it_names(c):
    g = geometry(c)
    assert (g.nth, g.ntd, g.kbd, g.keep) == c.geom
    pans = panels_of(c)
    assert g.P == c.P and pans[-1][1] == c.last and len(pans) == g.nwg
    assert {p[4] for p in pans} == c.paths
    assert c.nwins <= {p[3] for p in pans}
    assert sum(p[1] for p in pans) == g.M and all(1 <= p[1] <= g.P for p in pans)
    if c.de_lp:
        assert g.P == c.T and g.M % c.T == 0
    lay = layout(c)
    assert lay["partial"][3] % 4 == 0 and lay["xt"][3] % 4 == 0 and lay["dpred"][3] % 4 == 0


def test_the_table_reaches_every_edge():
    geo = {(c.geom, c.L) for c in CASES}
    inst = [(4, 1, 2), (4, 1, 4), (4, 2, 8), (4, 3, 10), (4, 3, 12), (4, 4, 16), (2, 3, 10), (1, 1, 2), (1, 1, 4)]
    for i in inst:                                                   # all nine instantiations, KEEP on (L = 1, 2) and off (L = 3, 4)
        assert any(gm[:3] == i and gm[3] for gm, _ in geo) and any(gm[:3] == i and not gm[3] for gm, _ in geo), i
    for L in (1, 2, 3, 4):
        assert any(c.L == L for c in CASES)
    assert any(c.L == 4 and c.H == 512 for c in CASES) and any(c.L == 4 and c.H == 128 for c in CASES)
    # the D edges, both sides of every geometry switch, and the refusals
    assert {4, 64, 68, 128, 132, 256, 260, 320, 324, 384, 388, 512} <= {c.D for c in CASES if c.H == 512}
    assert {320} <= {c.D for c in CASES if c.H == 256} and {64, 68, 128} <= {c.D for c in CASES if c.H == 128}
    assert (324, 256) in {(D, H) for D, H, _ in REFUSED} and (132, 128) in {(D, H) for D, H, _ in REFUSED}
    # panel heights
    Ms = {c.B * c.T for c in CASES}
    assert {1, 15, 16, 17, 4096, 16129} <= Ms
    assert any(c.P == 17 and c.last < 17 for c in CASES) and any(c.P == 33 for c in CASES)
    large = [c for c in CASES if c.P == 64]
    assert {c.name for c in large} == set(LARGE) and len(large) <= 3 and not any(c.B * c.T > 9000 for c in CASES if c.P < 64)
    assert sum(c.H == 128 and c.D <= 64 and c.L == 1 for c in large) == 2 and sum(c.H == 512 for c in large) == 1
    assert any(c.last == 1 for c in large) and any(c.last == 64 for c in large)
    for H in (128, 256):                                             # ends inside / just past a row group, around the 32-row half
        assert {1, 2, 3, 5, 17, 33} <= {c.last for c in CASES if c.H == H}, H
    # windows
    allp = [(c, p) for c in CASES for p in panels_of(c)]
    assert any(c.de_lp and p[3] == 1 and p[1] == c.T for c, p in allp)               # panel == window
    assert any(p[3] == 1 and c.T >= 100 * c.P for c, p in allp)                      # a window much longer than the panel
    for n in (2, 3, 8, 9, 16, 64):
        assert any(p[3] == n for _, p in allp), n
    assert any(p[3] == 8 and p[4] == "staged" for _, p in allp) and any(p[3] == 9 and p[4] == "unstaged" for _, p in allp)
    assert any({"staged", "unstaged"} <= c.paths for c in CASES)
    assert any({8, 9} <= {p[3] for p in panels_of(c)} for c in CASES)                # 8 and 9 windows in one launch
    inner = lambda c, p: [b for b in range(p[0] + 1, p[0] + p[1]) if b % c.T == 0]     # window boundaries inside a panel
    assert any(any((b - p[0]) % 16 == 0 for b in inner(c, p)) for c, p in allp)
    assert any(any((b - p[0]) % 16 != 0 for b in inner(c, p)) for c, p in allp)
    # store forms
    assert any(c.xt == "D" and c.D % 8 == 4 for c in CASES) and any(c.dp == "D" and c.D % 8 == 4 for c in CASES)
    assert any(c.dp == "up8" and c.D % 8 == 4 and dp16_form(c) for c in CASES)
    assert any(c.dp == "off8" and layout(c)["dpred"][3] % 8 == 0 and not dp16_form(c) for c in CASES)
    assert any(c.ld_e_extra for c in CASES) and any(c.ld_part_extra for c in CASES) and any(c.slots for c in CASES)
    # t: 0, the last table row, a negative value, a value beyond the table
    for c in CASES:
        t = make_inputs(c)["t"] if c.name not in LARGE else None
        if t is not None and c.B >= 4:
            assert {0, TABLE_ROWS - 1} <= set(t.tolist()) and bool((t < 0).any()) and bool((t >= TABLE_ROWS).any())
    assert sum(c.B >= 4 for c in CASES) >= 10


def test_inputs_are_what_the_docstring_says():
    for c in CASES:
        if c.name in LARGE:
            continue
        inp = make_inputs(c)
        w, zr = zero_rows(c)
        assert (c.B * c.T == 1) == (w is None)
        if w is not None:
            assert not inp["x0"].view(-1, c.D)[zr].any() and not inp["eps"].view(-1, c.D)[zr].any()
            assert torch.equal(inp["e"][w, :c.H].float(), -inp["bias"][0])
        for b in inp["bias"]:
            assert torch.equal(b.to(BF).float(), b)
        for i in range(c.L):                                         # a shift by 4 or 8 columns changes gamma and beta everywhere
            for v in (inp["gamma"][i], inp["beta"][i]):
                assert bool((v != v.roll(4)).all()) and bool((v != v.roll(8)).all())
        if c.B > 1:                                                  # distinct e rows per window and per block
            e = inp["e"][:, :c.L * c.H].float()
            assert bool((e[0] != e[1]).any()) and (c.L == 1 or bool((e[:, :c.H] != e[:, c.H:2 * c.H]).any()))


# ---- b. the emulation is inside every bound ----------------------------------------------------------------------------------
WORST = {}


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_the_bound_admits_the_emulation(c):
    inp = make_inputs(c)
    pan = emulated_panels(c)
    worst = check(c, inp, emulate(c, inp, panels=pan), panels=pan)
    print(c.name, " ".join(f"{k}={v:.3g}" for k, v in worst.items()))
    assert all(v < 1 for v in worst.values()), worst
    for k, v in worst.items():
        WORST[k] = max(WORST.get(k, 0.0), v)


def test_worst_ratio_per_stage():
    for c in CASES if not WORST else ():                            # run alone: the cases have not been emulated yet
        test_the_bound_admits_the_emulation(c)
    print("worst error / bound per stage over all cases (fp32 emulation):")
    for k, v in WORST.items():
        print(f"  {k:10s} {v:.3g}")
    assert all(v < 1 for v in WORST.values())


# ---- c. the mutants ----------------------------------------------------------------------------------------------------------
MUTANTS = [
    ("e row of the neighbouring window", "e_neighbour", ["h512_d132_m39", "h128_m8208", "h256_m21"]),
    ("e columns of block 0 used for block 1", "e_block0", ["h512_d68_m16", "h128_d128_m19"]),
    ("e dropped on the unstaged path only", "e_unstaged_dropped", ["h512_d388_m18", "h128_mix", "h512_d128_m17"]),
    ("bias dropped", "no_bias", ["h512_d4_m1", "h256_m19", "h128_d4_m21"]),
    ("t not clamped", "t_noclamp", ["h512_d324_m20", "h512_d4_m1", "h128_d128_m19"]),
    ("the clamped duplicate row stored past M", "dup_row", ["h512_d128_m17", "h256_m21", "h128_d64_m17"]),
    ("LayerNorm eps omitted", "no_eps", ["h512_d68_m16", "h256_d4_m18", "h128_d68_m18"]),
    ("variance over H - 1", "var_h1", ["h512_d260_m40", "h256_m19", "h128_d64_m17"]),
    ("gamma shifted by 8 columns", "gamma_shift", ["h512_d64_m15", "h256_d320_m17", "h128_d64_m17"]),
    ("beta shifted by 8 columns", "beta_shift", ["h512_d64_m15", "h256_d320_m17", "h128_d64_m17"]),
    ("SiLU' written as sigma (1 - sigma)", "silu_grad", ["h512_d4_m1", "h256_m21", "h128_d68_m18"]),
    ("the mean term ma dropped in the LayerNorm backward", "no_ma", ["h512_d132_m39", "h256_m19", "h128_d4_m21"]),
    ("gscale 1 / (M D)", "gscale", ["h512_d4_m1", "h256_d4_m18", "h128_d128_m19"]),
    ("head bias dropped", "no_head_bias", ["h512_d512_m50", "h256_m19", "h128_d4_m21"]),
    ("transposed weights of the wrong block in the backward", "wrong_wt", ["h512_d64_m15", "h256_m21", "h128_d128_m19"]),
    ("rows >= nrows included in a column sum", "colsum_rows", ["h512_d128_m17", "h256_m19", "h128_d68_m18"]),
    ("loss summed over columns >= D", "loss_pad", ["h512_d4_m1", "h256_m21", "h128_d68_m18"]),
    ("de_lp taken from dbeta", "de_from_dbeta", ["h512_d4_m1", "h512_d384_m32", "h256_m4114"]),
]


@pytest.mark.parametrize("name,bug,cases", MUTANTS, ids=[m[1] for m in MUTANTS])
def test_mutants_are_rejected(name, bug, cases):
    for cn in cases:
        c = BY_NAME[cn]
        inp = make_inputs(c)
        with pytest.raises(AssertionError):
            check(c, inp, emulate(c, inp, bug=bug))
        assert not math.isnan(sum(check(c, inp, emulate(c, inp)).values()))     # the same case passes without the bug
