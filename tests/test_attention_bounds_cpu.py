"""The elementwise attention bound of tests/attention_cases.py, checked without a GPU.

a. A torch-CPU emulation of each path's arithmetic (fp32 math; on the MFMA paths P, dS and the outputs pass through bf16
   where the kernels narrow them; lse = m + log(l) in fp32) stays inside the bound on every case of the GPU table: the bound
   admits a correct implementation.
b. Six one-line bugs, applied to that emulation, fall outside the bound on a named table case: the bound, and the inputs of
   the table, are sharp enough to see them.
c. The dispatch arithmetic of csrc/attention.hip / attention_mfma.hip restated in Python gives every case's stated path, so
   a mistyped case fails here and not on the GPU."""
import math
import zlib

import pytest
import torch

from tests.attention_cases import (BY_NAME, CASES, DROP, DT, MFMA_T, REFUSALS, case_inputs, dispatch, evaluate, heads,
                                   ref_lse, unheads, up_of, valu_lds, violations)


def _bf(t):
    return t.to(torch.bfloat16).float()


def emulate(x, dt, path_fwd, path_bwd, mask=None, lse_bwd=None, mutant=None):
    """fp32 restatement of the kernels' arithmetic -> (O, lse, dqkv) in the kernels' layouts and storage dtypes.  lse_bwd:
    the [B, H, T] lse the backward is given (None: the forward's own).  mutant: one of MUTANTS."""
    B, T, d3 = x.qkv.shape
    d, H, dh = d3 // 3, x.H, x.dh
    N = B * H
    Q, K, V = (heads(x.qkv[..., i * d:(i + 1) * d], H).float() for i in range(3))
    dO = heads(x.dout, H).float()
    M = torch.ones(N, T, T) if mask is None else mask.float().reshape(N, T, T)
    scale = torch.tensor(1.0 / math.sqrt(dh), dtype=torch.float32)
    if mutant == "scale":
        scale = scale * (1 + 2.0 ** -5)
    if mutant == "swap_k_heads":                                    # head h reads the keys of head h ^ 1
        K = K.reshape(B, H, T, dh)[:, [h ^ 1 if (h ^ 1) < H else h for h in range(H)]].reshape(N, T, dh)
    Tk = T
    if mutant == "pad_zero_key":                                    # one zero-filled padding key, not masked
        K, V = (torch.cat([t, torch.zeros(N, 1, dh)], 1) for t in (K, V))
        M, Tk = torch.cat([M, torch.ones(N, T, 1)], 2), T + 1
    if mutant == "drop_last_key":
        K, V, M, Tk = K[:, :T - 1], V[:, :T - 1], M[:, :, :T - 1], T - 1
    mf, mb = path_fwd != "attn_valu", path_bwd != "attn_valu"
    narrow_f = _bf if mf else (lambda t: t)
    narrow_b = _bf if mb else (lambda t: t)
    # forward
    S = (Q @ K.transpose(1, 2)) * scale if mf else (Q * scale) @ K.transpose(1, 2)
    m = S.amax(-1, keepdim=True)
    p = torch.exp(S - m)
    l = p.sum(-1, keepdim=True)
    O = ((narrow_f(p * M) @ V) * (1.0 / l)).to(DT[dt])
    if mutant == "dup_last_row" and T > 1:
        O[:, T - 1] = O[:, T - 2]
    lse = (m + torch.log(l)).squeeze(-1)
    # backward
    lb = lse if lse_bwd is None else lse_bwd.float().reshape(N, T)
    pb = torch.exp((Q @ K.transpose(1, 2)) * scale - lb[..., None])
    dp = (dO @ V.transpose(1, 2)) * M
    if mutant == "d_from_bf16_out":
        D = (dO * O.float()).sum(-1, keepdim=True)
    else:
        D = (pb * dp).sum(-1, keepdim=True)
    dS = narrow_b(pb * (dp - D))
    dQ = ((dS @ K) * scale).to(DT[dt])
    dK = ((dS.transpose(1, 2) @ Q) * scale).to(DT[dt])
    dV = (narrow_b(pb * M).transpose(1, 2) @ dO).to(DT[dt])
    if Tk != T:                                                     # back to T key rows (the dropped key gets no gradient)
        fix = (lambda t: t[:, :T]) if Tk > T else (lambda t: torch.cat([t, torch.zeros(N, 1, dh, dtype=t.dtype)], 1))
        dK, dV = fix(dK), fix(dV)
    dqkv = torch.cat([unheads(t, B) for t in (dQ, dK, dV)], -1)
    return unheads(O, B), lse.reshape(B, H, T), dqkv


def _cpu_mask(c):
    """Bernoulli(1 - p) multipliers in fp32, as ib_attention_drop_mask writes them (the draw itself does not matter here)"""
    if not c.opt.get("drop"):
        return None
    g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()) ^ 0x5A5A)
    keep = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - DROP[0])
    return (torch.rand(c.B, c.H, c.T, c.T, generator=g) >= DROP[0]).float() * keep


def _check_all(c, x, mask, outs):
    """outs = [(O, lse, dqkv, lse given to that backward)]: one evaluate() for all of them"""
    ref, bound = evaluate(x, c.dt, up_of(c.fwd), up_of(c.bwd), mask, [o[3] for o in outs])
    msgs = []
    for i, (O, lse, dqkv, _) in enumerate(outs):
        for what, got, r, b, path in (("O", O, ref["O"], bound["O"], c.fwd), ("lse", lse, ref["lse"], bound["lse"], c.fwd),
                                      ("dqkv", dqkv, ref["dqkv"], bound["dqkv"][i], c.bwd)):
            msg, _ = violations(what, got, r, b, c.H, path)
            if msg:
                msgs.append(msg)
    return ref, msgs


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_emulation_is_inside_the_bound(c):
    x, mask = case_inputs(c), _cpu_mask(c)
    bwd = c.bwd if c.bwd != "-" else "attn_valu"                    # refused on the GPU; the arithmetic is still defined
    lse_ref = ref_lse32(x)
    a = emulate(x, c.dt, c.fwd, bwd, mask, lse_bwd=lse_ref)          # the backward alone, on the reference lse
    b = emulate(x, c.dt, c.fwd, bwd, mask)                           # as training: on the forward's own lse
    _, msgs = _check_all(c._replace(bwd=bwd), x, mask, [a + (lse_ref,), b + (b[1],)])
    assert not msgs, "\n".join(msgs)


def ref_lse32(x):
    return ref_lse(x).float()


# mutant -> (the table case that must catch it, the outputs it may show in).
# d_from_bf16_out is the bug the backward kernels' comment describes: D = rowsum(dO o bf16(O)) instead of rowsum(P o dP).
# It is caught on the `offset` family (at every length above 1), where O is near 8, its bf16 rounding is large and
# dS = P (dP - D) cancels.  The `peaked` family does NOT see it: there e_s, the worst-case (linear in dh, on |q| . |k|)
# fp32 score error, is 6e-4 for scores of magnitude 30 and eta G is several times the damage; the statistical score error
# is sqrt(dh) times smaller, but the bound is a theorem and keeps the worst case.
MUTANTS = {
    "pad_zero_key": ("mfma1p_bf16_b2h2_T17_dh64_negative", ("O", "lse")),
    "drop_last_key": ("mfma1p_bf16_b2h2_T17_dh64_gauss", ("O", "lse")),
    "swap_k_heads": ("mfma1p_bf16_b2h2_T65_dh64_gauss", ("O", "lse")),
    "scale": ("mfma1p_bf16_b2h2_T65_dh64_peaked", ("O", "lse")),
    "d_from_bf16_out": ("mfma1p_bf16_b2h2_T16_dh64_offset", ("dqkv",)),
    "dup_last_row": ("mfma1p_bf16_b2h2_T17_dh64_peaked", ("O",)),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutant_is_outside_the_bound(mutant):
    name, shows = MUTANTS[mutant]
    c = BY_NAME[name]
    x = case_inputs(c)
    lse_ref = ref_lse32(x)
    clean = emulate(x, c.dt, c.fwd, c.bwd, lse_bwd=lse_ref)
    bad = emulate(x, c.dt, c.fwd, c.bwd, lse_bwd=lse_ref, mutant=mutant)
    ref, bound = evaluate(x, c.dt, up_of(c.fwd), up_of(c.bwd), None, [lse_ref])
    b = {"O": bound["O"], "lse": bound["lse"], "dqkv": bound["dqkv"][0]}
    got = lambda o: {"O": o[0], "lse": o[1], "dqkv": o[2]}
    for what in ("O", "lse", "dqkv"):
        assert violations(what, got(clean)[what], ref[what], b[what], c.H, "-")[0] is None, (name, what)
    caught = [what for what in shows if violations(what, got(bad)[what], ref[what], b[what], c.H, "-")[0] is not None]
    assert caught, f"{mutant} stays inside the bound on {name}: the inputs are too tame, strengthen the case"


def test_every_offset_case_sees_d_from_the_rounded_output():
    """not one lucky seed: each `offset` length above 1 on the small MFMA shape catches that mutant"""
    for T in MFMA_T[1:]:
        c = BY_NAME[f"mfma1p_bf16_b2h2_T{T}_dh64_offset"]
        x = case_inputs(c)
        lse_ref = ref_lse32(x)
        dqkv = emulate(x, c.dt, c.fwd, c.bwd, lse_bwd=lse_ref, mutant="d_from_bf16_out")[2]
        ref, bound = evaluate(x, c.dt, up_of(c.fwd), up_of(c.bwd), None, [lse_ref])
        assert violations("dqkv", dqkv, ref["dqkv"], bound["dqkv"][0], c.H, "-")[0] is not None, c.name


def test_mutants_are_seen_on_the_valu_path_too():
    """the same six on an fp32 case (u_P = 0), where the bound is five orders tighter"""
    for mutant, fam in (("pad_zero_key", "negative"), ("drop_last_key", "gauss"), ("swap_k_heads", "gauss"),
                        ("scale", "gauss"), ("dup_last_row", "gauss")):
        c = BY_NAME[f"valu_fp32_b2h3_T63_dh64_{fam}"]
        x = case_inputs(c)
        lse_ref = ref_lse32(x)
        O, lse, dqkv = emulate(x, c.dt, c.fwd, c.bwd, lse_bwd=lse_ref, mutant=mutant)
        ref, bound = evaluate(x, c.dt, 0.0, 0.0, None, [lse_ref])
        assert violations("O", O, ref["O"], bound["O"], c.H, "-")[0] is not None, mutant


def test_table_paths_follow_the_dispatch_arithmetic():
    assert len(BY_NAME) == len(CASES), "case names are not unique"
    for c in CASES:
        r = dispatch(c.dt, c.B, c.T, c.H, c.dh, c.opt.get("misalign"))
        assert (r["fwd"], r["bwd"]) == (c.fwd, c.bwd), (c.name, r)
        for k in ("nt", "two_pass", "qsplit"):
            if k in c.opt:
                assert r[k] == c.opt[k], (c.name, k, r)
        assert r["lds_fwd"] <= 160 * 1024 and (r["lds_bwd"] or 0) <= 160 * 1024, (c.name, r)
    for dt, B, T, H, dh, fwd, bwd in REFUSALS:
        r = dispatch(dt, B, T, H, dh)
        assert (r["fwd"], r["bwd"]) == (fwd, bwd), ((dt, B, T, H, dh), r)
    # the two LDS limits of the VALU kernels, at their edges
    assert valu_lds(256, 76)[0] <= 160 * 1024 < valu_lds(256, 77)[0]
    assert valu_lds(256, 72)[1] <= 160 * 1024 < valu_lds(256, 73)[1]
    assert valu_lds(152, 128)[0] <= 160 * 1024 < valu_lds(153, 128)[0]
    assert valu_lds(144, 128)[1] <= 160 * 1024 < valu_lds(145, 128)[1]


def test_table_covers_what_it_must():
    """every path in both directions, every key-tile instance on each MFMA forward, dropout on each path, and the
    `negative` family at every MFMA length that is not a whole number of key tiles"""
    assert {(c.fwd, c.bwd) for c in CASES} >= {("attn_mfma", "attn_mfma"), ("attn_mfma_2p", "attn_mfma"),
                                               ("attn_valu", "attn_valu"), ("attn_mfma", "attn_valu"), ("attn_valu", "-")}
    assert {c.opt["nt"] for c in CASES if c.fwd == "attn_mfma" and "nt" in c.opt} == {4, 8, 14, 16}
    assert {c.opt["nt"] for c in CASES if c.fwd == "attn_mfma_2p"} == {8, 14, 16}
    for drop in (False, True):
        got = {(c.fwd, c.opt.get("nt")) for c in CASES if bool(c.opt.get("drop")) == drop}
        assert got >= {("attn_mfma", 4), ("attn_mfma", 8), ("attn_mfma", 14), ("attn_mfma", 16), ("attn_mfma_2p", 8),
                       ("attn_mfma_2p", 14), ("attn_mfma_2p", 16), ("attn_valu", None)}, (drop, got)
    neg = {c.T for c in CASES if c.family == "negative" and c.fwd == "attn_mfma" and c.bwd == "attn_mfma"}
    assert neg >= {T for T in MFMA_T if T % 16}
    from inferbiomechanics_amd import hip
    assert {18: "attn_valu", 19: "attn_mfma", 20: "attn_mfma_2p"}.items() <= hip.PATH_NAMES.items()
