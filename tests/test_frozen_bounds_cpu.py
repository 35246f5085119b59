"""The checks of tests/frozen_cases.py, checked without a GPU.

a. The restated launch geometry equals the C query functions (the library loads on the CPU) for M = 1 ... 33000 and every
   supported ffn and chunks value: ib_linear_ln_panel_workgroups, ib_linear_panel_workgroups, ib_ffn_infer_workgroups /
   _workspace, ib_ffn_chain_workgroups, and -- ib_gemm_nt_splitk_splits is not exported -- ib_linear_ln_fwd_workspace =
   max(linear_ln_split, nt_splitk_splits) M N 4 over the (N, K) pairs of the table.  Every case reaches the instantiation it
   names, and the table reaches every instantiation of the issue's dispatch table.
b. The CPU assertions hold for every case: every GEMM exact (|a| @ |b|^T < 2^24), every bf16 value a kernel keeps an exactly
   representable integer <= 256 (s1 and x of the chain: half-integers), s1 of the chain +-c with 256 columns of each sign,
   x1 odd, the offset rows offset, no dead 16 x 32 block in any weight (reference() asserts; here it is run for every case).
c. The bound admits a correct kernel: an fp32 emulation of each kernel's arithmetic -- the same roundings (bf16 where the
   kernel stores bf16) and the same grouping of every row sum (per-lane order, then the DPP / shuffle tree); the GEMMs are
   exact, so their order does not matter; unfused multiply-adds, where the compiler may fuse: one rounding fewer, inside the
   same count -- passes check() on every case.  The worst error / bound per family is printed.
d. The checks reject one-line bugs.  The thirteen bugs of the issue's list, as 17 mutants of the emulation (gamma / beta
   shifted, residual / x1 / x addend dropped, eps omitted in both LayerNorms / in LN2 alone count once each), each on the
   NAMED cases of MUTANTS: check() must fail.  The eps mutants fall on the zero-variance rows every LayerNorm family has."""
import ctypes

import pytest
import torch

from tests.frozen_cases import (BF, BY_NAME, CASES, D, EPS, F32, FAMILIES, REFUSED, SLAB_LN, case_id, check, dead_blocks,
                                ffn_coop_geometry, ffn_geometry, ffn_infer_workspace, kernel_of, lin_panel_geometry,
                                linear_ln_plan, linear_ln_split, linear_ln_supported, linear_panel_workgroups,
                                linln_panel_workgroups, make_inputs, reference, relu, weights)


# ---- the emulation -------------------------------------------------------------------------------------------------------
def bf(t):
    return t.to(BF).to(F32)


def tree(t):
    """ff_row_sum: the DPP levels pair neighbours, then pairs of pairs ... (the last dimension is a power of two)"""
    while t.shape[-1] > 1:
        t = t[..., 0::2] + t[..., 1::2]
    return t[..., 0]


def butterfly(t):
    """slab_ln_kernel: s += __shfl_xor(s, o) for o = LPR / 2 ... 1"""
    o = t.shape[-1] // 2
    while o >= 1:
        t = t[..., :o] + t[..., o:2 * o]
        o //= 2
    return t[..., 0]


def emu_ln(v, gamma, beta, kind, bug=None):
    """-> (y as stored, mean, rstd) of fp32 rows v; kind: "panel" (linln_panel_kernel), (LPR, NCH) (slab_ln_kernel) or "rows"
    (ff_ln_rows_fwd)"""
    M, N = v.shape
    eps = torch.tensor(0.0 if bug == "no_eps" else EPS, dtype=F32)
    inv = torch.tensor(1.0 / (N - 1 if bug == "var_n1" else N), dtype=F32)
    invm = torch.tensor(1.0 / N, dtype=F32)
    g = gamma.roll(4) if bug == "gamma_shift" else gamma
    b = beta.roll(4) if bug == "beta_shift" else beta
    if kind == "rows":
        x = v.view(M, 64, 8)
        a0, a1 = ((x[..., 0] + x[..., 2]) + x[..., 4]) + x[..., 6], ((x[..., 1] + x[..., 3]) + x[..., 5]) + x[..., 7]
        q0 = ((x[..., 0] * x[..., 0] + x[..., 2] * x[..., 2]) + x[..., 4] * x[..., 4]) + x[..., 6] * x[..., 6]
        q1 = ((x[..., 1] * x[..., 1] + x[..., 3] * x[..., 3]) + x[..., 5] * x[..., 5]) + x[..., 7] * x[..., 7]
        s = a0 + a1
        mean = tree(s[:, :32]) * (2 * invm) if bug == "mean256" else tree(s) * invm
        rstd = torch.rsqrt((tree(q0 + q1) * inv - mean * mean).clamp_min(0) + eps)
        y = (v - mean[:, None]) * rstd[:, None] * g + b
        return bf(y), mean, rstd
    if kind == "panel":
        x = v.view(M, 64, 8)
        s = ((x[..., 0] + x[..., 1]) + (x[..., 2] + x[..., 3])) + ((x[..., 4] + x[..., 5]) + (x[..., 6] + x[..., 7]))
        mean = tree(s[:, :32]) * (2 * invm) if bug == "mean256" else tree(s) * invm
        d = x - mean[:, None, None]
        q = torch.zeros(M, 64)
        for k in range(8):
            q = q + d[..., k] * d[..., k]
        rstd = 1.0 / torch.sqrt(tree(q) * inv + eps)
        return bf(d.reshape(M, N) * rstd[:, None] * g + b), mean, rstd
    LPR, NCH = kind
    x = v.view(M, NCH, LPR, 4)                                       # chunk c of lane l: columns (c LPR + l) 4 ... + 3
    s = torch.zeros(M, LPR)
    for c in range(NCH):
        s = s + ((x[:, c, :, 0] + x[:, c, :, 1]) + (x[:, c, :, 2] + x[:, c, :, 3]))
    if bug == "mean256":
        half = v[:, :N // 2].reshape(M, -1, 4)
        mean = butterfly((half[..., 0] + half[..., 1]) + (half[..., 2] + half[..., 3])) * (2 * invm)
    else:
        mean = butterfly(s) * invm
    d = x - mean[:, None, None, None]
    q = torch.zeros(M, LPR)
    for c in range(NCH):
        e = d[:, c]
        q = q + ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + (e[..., 2] * e[..., 2] + e[..., 3] * e[..., 3]))
    rstd = 1.0 / torch.sqrt(butterfly(q) * inv + eps)
    return bf((v - mean[:, None]) * rstd[:, None] * g + b), mean, rstd


def _gemm(x, w, bug):
    """x @ w^T, exact in fp32 (frozen_cases.exact_gemm asserts it for the unmutated operands)"""
    if bug == "drop_last_kblock":
        x = x.clone()
        x[:, -32:] = 0.0
    return x @ w.T


def _bias(b, bug, chunked=True):
    if bug == "bias_tile":
        b = b.clone()
        b[5 * 16:6 * 16] = 0.0
    if bug == "bias_chunk0" and chunked:
        b = b[:D].repeat(b.numel() // D)
    return b


def _last_panel_from_before(y, P, bug):
    M = y.shape[0]
    r0 = (M - 1) // P * P
    if bug == "last_panel_from_before" and r0 > 0:
        y = y.clone()
        y[r0:] = y[r0 - P:M - P]
    return y


def emulate(c, bug=None):
    """the outputs of a case as frozen_cases.check takes them, from the fp32 emulation (with one bug)"""
    inp = make_inputs(c)
    W = weights(c.fam, c.N, c.K, c.ffn)
    M = c.M
    if c.fam == "linln_panel":
        P = linln_panel_workgroups(M)[1]
        t = _gemm(inp["x"], W["w"], bug)
        if c.bias:
            t = t + _bias(W["bias"], bug, False)
        if c.res and bug != "addend_dropped":
            res = inp["res"]
            if bug == "res_last_row":                                 # the clamp min(row, nrows - 1) applied to every row
                rows = torch.arange(M)
                res = res[torch.minimum(rows // P * P + P - 1, torch.tensor(M - 1))]
            t = t + res
        return {"y": _last_panel_from_before(emu_ln(t, W["gamma"], W["beta"], "panel", bug)[0], P, bug)}
    if c.fam == "linear_panel":
        y = _gemm(inp["x"], W["w"], bug)
        if c.bias:
            y = y + _bias(W["bias"], bug)
        return {"y": _last_panel_from_before(bf(y), lin_panel_geometry(M, c.chunks)[1], bug)}
    if c.fam == "linear_ln":
        prod, used, _ = linear_ln_plan(M, c.N, c.K)
        kc = c.K // used if prod == "nt_splitk" else linear_ln_split(M, c.N, c.K)[1]
        x = inp["x"].clone()
        if bug == "drop_last_kblock":
            x[:, -32:] = 0.0
        slabs = [x[:, k:k + kc] @ W["w"][:, k:k + kc].T for k in range(0, c.K, kc)]
        v = slabs[0]
        for s in slabs[1:]:
            v = v + s
        out = {"slab_sum": v, "nslab": len(slabs)}
        if c.bias:
            v = v + _bias(W["bias"], bug, False)
        out["a_out"] = bf(v)
        if c.saved:
            v = out["a_out"]
        if c.res and bug != "addend_dropped":
            v = v + inp["res"]
        out["y"], out["mean"], out["rstd"] = emu_ln(v, W["gamma"], W["beta"], SLAB_LN[c.N], bug)
        return out
    act = (lambda t: t) if bug == "no_relu" else relu
    if c.fam == "ffn_infer":
        panels, P, nc, sb = ffn_coop_geometry(M, D, c.ffn)
        x1 = inp["x1"]
        h = bf(act(_gemm(x1, W["w1"], bug) + _bias(W["b1"], bug)))
        hc = D // sb
        slabs = [h[:, j * hc:(j + 1) * hc] @ W["w2"][:, j * hc:(j + 1) * hc].T for j in range(nc * sb)]
        if bug == "swap_slabs":
            slabs[0], slabs[1] = slabs[1], slabs[0]
        v = slabs[0]
        for s in slabs[1:]:
            v = v + s
        v = v + W["b2"]
        if bug != "addend_dropped":
            v = v + x1
        slabs = _last_panel_from_before(torch.stack(slabs).transpose(0, 1), P, bug).transpose(0, 1)
        return {"slabs": slabs, "y": emu_ln(v, W["gamma"], W["beta"], (64, 2), bug)[0]}
    P = ffn_geometry(M, D, c.ffn)[1]
    s1 = _gemm(inp["attn"], W["wo"], bug) + _bias(W["bo"], bug, False)
    s1 = bf(s1 + inp["x"]) if bug != "x_dropped" else bf(s1)
    x1 = emu_ln(s1, W["gamma1"], W["beta1"], "rows", bug if bug in ("no_eps", "var_n1", "mean256") else None)[0]
    h = bf(act(x1 @ W["w1"].T + W["b1"]))
    s2 = (h @ W["w2"].T + W["b2"])
    s2 = bf(s2 + x1) if bug != "addend_dropped" else bf(s2)
    y = emu_ln(s2, W["gamma"], W["beta"], "rows", "no_eps" if bug == "no_eps_ln2" else bug)[0]
    out = {"y": _last_panel_from_before(y, P, bug)}
    if c.tail:
        q = bf(y @ W["wqkv"].T + _bias(W["bqkv"], "bias_chunk0" if bug == "bias_chunk0" else None))
        out["qkv"] = q.roll(D, 1) if bug == "qkv_rotate" else q
    return out


# ---- a. geometry ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from inferbiomechanics_amd import hip
    return hip.lib()


def test_geometry_equals_the_c_query_functions(lib):
    i32 = ctypes.c_int32
    rows, panels = i32(0), i32(0)
    nk = sorted({(c.N, c.K) for c in CASES if c.fam == "linear_ln"})
    for M in range(1, 33001):
        nwg, P = linln_panel_workgroups(M)
        rows.value = -1
        assert lib.ib_linear_ln_panel_workgroups(M, D, D, ctypes.byref(rows)) == nwg and (not nwg or rows.value == P), M
        for ch in range(1, 10):
            assert lib.ib_linear_panel_workgroups(M, ch * D, D) == linear_panel_workgroups(M, ch * D, D), (M, ch)
        for nc in range(1, 10):
            ffn = nc * D
            pn, P, _, sb = ffn_coop_geometry(M, D, ffn)
            got = lib.ib_ffn_infer_workgroups(M, D, ffn, ctypes.byref(rows), ctypes.byref(panels))
            assert got == pn * nc * sb and (not pn or (rows.value, panels.value) == (P, pn)), (M, ffn)
            assert lib.ib_ffn_infer_workspace(M, D, ffn) == ffn_infer_workspace(M, D, ffn), (M, ffn)
            nwg, P, _ = ffn_geometry(M, D, ffn)
            assert lib.ib_ffn_chain_workgroups(M, D, ffn, ctypes.byref(rows)) == nwg and (not nwg or rows.value == P), (M, ffn)
        for N, K in nk:
            assert lib.ib_linear_ln_fwd_workspace(M, N, K) == linear_ln_plan(M, N, K)[2] * M * N * 4, (M, N, K)
    assert lib.ib_linear_ln_panel_workgroups(64, 256, D, None) == 0 and lib.ib_linear_ln_panel_workgroups(64, D, 1024, None) == 0
    assert lib.ib_linear_panel_workgroups(64, 300, D) == 0 and lib.ib_linear_panel_workgroups(64, D, 256) == 0
    assert lib.ib_ffn_infer_workgroups(64, 256, 2048, None, None) == 0 and lib.ib_ffn_chain_workgroups(64, 256, 2048, None) == 0
    assert lib.ib_ffn_infer_workgroups(64, D, 768, None, None) == 0 and lib.ib_ffn_chain_workgroups(64, D, 768, None) == 0


def test_every_case_reaches_the_instantiation_it_names():
    for c in CASES:
        assert kernel_of(c) == c.kernel, f"{c.name}: lands in {kernel_of(c)}, the table says {c.kernel}"
    reached = {c.kernel for c in CASES}
    for k in ("linln_panel<1>", "linln_panel<2>", "linear_panel<1,1>", "linear_panel<1,4>", "linear_panel<2,4>", "linear_panel<4,4>",
              "coop_small<4>+slab_ln<64,2>", "coop_small<2>+slab_ln<64,2>", "coop+slab_ln<64,2>", "chain_infer", "chain_infer_qkv"):
        assert k in reached, k
    for N, (LPR, NCH) in SLAB_LN.items():
        assert any(k.startswith("ring/") and k.endswith(f"slab_ln<{LPR},{NCH}>") for k in reached), N
        assert N == 64 or any(k.startswith("nt_splitk/") and k.endswith(f"slab_ln<{LPR},{NCH}>") for k in reached), N
    assert {"ring/1", "ring/4", "nt_splitk/2", "nt_splitk/4"} <= {k.split("+")[0] for k in reached if "/" in k}
    # the edges: both sides of each are in the table
    for fam, key, edges in (("linln_panel", {}, ((256, 257), (4096, 4097))),
                            ("linear_panel", dict(chunks=3), ((416, 417), (1360, 1361), (2720, 2721), (5440, 5441))),
                            ("linear_panel", dict(chunks=1), ((1280, 1281),)), ("linear_panel", dict(chunks=8), ((160, 161),)),
                            ("ffn_infer", dict(ffn=2048), ((320, 321), (640, 641), (1024, 1025), (4096, 4097))),
                            ("ffn_infer", dict(ffn=512), ((1280, 1281), (2560, 2561))),
                            ("ffn_infer", dict(ffn=4096), ((160, 161), (320, 321)))):
        have = {c.M for c in CASES if c.fam == fam and all(getattr(c, k) == v for k, v in key.items())}
        for lo, hi in edges:
            assert {lo, hi} <= have, (fam, key, lo, hi)
    assert linln_panel_workgroups(4100) == (242, 17) and 4100 - 241 * 17 == 3
    assert ffn_geometry(8193, D, 2048)[:2] == (249, 33) and 8193 - 248 * 33 == 9
    assert ffn_coop_geometry(4097, D, 2048)[:2] == (65, 64)
    # the refusals are refusals of the restated predicates too
    assert not linln_panel_workgroups(8193)[0] and not lin_panel_geometry(8193, 3)[0] and not lin_panel_geometry(64, 9)[0]
    for _, a in REFUSED["ffn_infer"]:
        assert not ffn_coop_geometry(a["M"], a["d"], a["ffn"])[0]
    for _, a in REFUSED["chain"]:
        assert not ffn_geometry(a["M"], a["d"], a["ffn"])[0]
    for _, a in REFUSED["linear_ln"]:
        assert not linear_ln_supported(64, a["N"], a["K"], a["dtype"])


# ---- b. the CPU assertions -------------------------------------------------------------------------------------------------
def test_no_weight_has_a_dead_block():
    seen = 0
    for c in CASES:
        for k, w in weights(c.fam, c.N, c.K, c.ffn).items():
            if w.dim() == 2:
                assert dead_blocks(w) == 0 and bool((w.abs() <= 1).all()), (c.name, k)
                seen += 1
    assert seen


# ---- b, c. exactness of every case, and the emulation inside the bound ------------------------------------------------------
WORST = {}


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_case_is_exact_and_the_bound_admits_the_emulation(c):
    reference(c)                                                       # the assertions of frozen_cases: exact, representable
    msgs, worst = check(c, emulate(c))
    assert not msgs, "\n".join(msgs)
    WORST[c.fam] = max(WORST.get(c.fam, 0.0), worst)
    print(f"emulation error / bound  {c.name:36s} {worst:.3f}  {c.kernel}")


def test_worst_ratio_per_family():
    for fam in FAMILIES:
        print(f"emulation error / bound, worst of the family  {fam:13s} {WORST.get(fam, float('nan')):.3f}")
        assert fam == "linear_panel" or not WORST or 0.0 < WORST.get(fam, 1.0) <= 1.0


# ---- d. mutants ------------------------------------------------------------------------------------------------------------
MUTANTS = (        # (name, the bug emulate() applies, the cases that must reject it)
    ("bias_tile", "bias_tile", ("linln_panel_257", "linear_panel_417_chunks3", "ffn_infer_321_ffn2048", "chain_17_ffn512")),
    ("bias_chunk0", "bias_chunk0", ("linear_panel_417_chunks3", "ffn_infer_321_ffn2048", "chain_17_ffn512_tail")),
    ("drop_last_kblock", "drop_last_kblock", ("linln_panel_257", "linear_panel_1_chunks3", "ffn_infer_1_ffn2048", "chain_17_ffn512",
                                              "linear_ln_100_N128_K256")),
    ("drop_last_kblock_of_wo_breaks_the_balance", "drop_last_kblock", ("chain_4097_ffn512",)),
    ("swap_slabs", "swap_slabs", ("ffn_infer_1_ffn2048", "ffn_infer_321_ffn2048", "ffn_infer_161_ffn4096")),
    ("no_relu", "no_relu", ("ffn_infer_321_ffn2048", "chain_17_ffn512")),
    ("res_last_row", "res_last_row", ("linln_panel_257", "linln_panel_257_r")),
    ("addend_dropped", "addend_dropped", ("linln_panel_257", "ffn_infer_321_ffn2048", "chain_17_ffn512", "linear_ln_100_N128_K256")),
    ("x_dropped", "x_dropped", ("chain_17_ffn512",)),
    ("gamma_shift", "gamma_shift", ("linln_panel_257", "ffn_infer_1_ffn2048", "chain_17_ffn512", "linear_ln_37_N64_K64")),
    ("beta_shift", "beta_shift", ("linln_panel_257", "ffn_infer_1_ffn2048", "chain_17_ffn512", "linear_ln_37_N64_K64")),
    ("no_eps", "no_eps", ("linln_panel_257", "linear_ln_100_N128_K256", "ffn_infer_321_ffn2048", "chain_17_ffn512",
                          "chain_4097_ffn2048")),
    ("no_eps_ln2", "no_eps_ln2", ("chain_17_ffn512", "chain_15_ffn2048_tail")),
    ("var_n1", "var_n1", ("linear_ln_100_N128_K256", "linear_ln_639_N512_K512")),
    ("mean256", "mean256", ("linln_panel_257", "ffn_infer_1_ffn2048", "chain_17_ffn512", "linear_ln_100_N128_K256")),
    ("last_panel_from_before", "last_panel_from_before", ("linln_panel_257", "linear_panel_417_chunks3", "ffn_infer_321_ffn2048",
                                                          "chain_17_ffn512")),
    ("qkv_rotate", "qkv_rotate", ("chain_17_ffn512_tail",)),
)


@pytest.mark.parametrize("name,bug,cases", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_mutants_are_rejected(name, bug, cases):
    for case in cases:
        c = BY_NAME[case]
        msgs, worst = check(c, emulate(c, bug))
        assert msgs, f"{name} on {case} passes every check (worst error / bound {worst:.3g})"
        print(f"{name:24s} {case:28s} rejected: {msgs[0][:150]}")
