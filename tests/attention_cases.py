"""Shared by tests/test_attention_edges_gpu.py and tests/test_attention_bounds_cpu.py: the case table of the standalone
attention kernels (csrc/attention.hip, csrc/attention_mfma.hip), the dispatch arithmetic restated in Python, the seeded input
families, the float64 reference and the ELEMENTWISE error bound every output is held to.

Layouts: qkv [B, T, 3 H dh] (q | k | v, head h in columns h dh .. (h + 1) dh of each third), out / dout [B, T, H dh],
lse [B, H, T] fp32, the dropout multipliers (0 or 1 / (1 - p)) mask [B, H, T, T].

Reference (float64, on the STORED inputs), scale = 1 / sqrt(dh), per (window, head):
  S = scale Q K^T,  P = softmax(S),  lse = logsumexp(S) (of the undropped scores),  O = (P o mask) V
  dP = mask o (dO V^T),  D = rowsum(P o dP),  dS = P o (dP - D)
  dQ = scale dS K,  dK = scale dS^T Q,  dV = (P o mask)^T dO

The bound.  u is the unit roundoff of the storage format, |fl(x) - x| <= u |x| under round to nearest: 2^-24 for fp32 (24
significant bits) and 2^-8 for bf16 (8 significant bits: just above a power of two 2^e the spacing is 2^(e-7) and half of it
is 2^-8 of the value; 2^-9 holds only at the top of a binade, and test_attention_bounds_cpu.py has correctly rounded results
beyond it).  u_P = 2^-8 where the kernel narrows P and dS to bf16 before the second product (the MFMA kernels) and 0 on the
VALU path.  Per query row i
  e_s(i)  = dh 2^-23 scale max_j (|q_i| . |k_j|)
      the fp32 score error: dh products (exact for bf16 operands) summed in fp32 in any order, <= dh 2^-24 |q_i| . |k_j|,
      and as much again for the multiplication by scale (the VALU forward scales q first, the backward the finished sum)
  eps(i)  = 2 e_s(i) + T 2^-23 + 2^-16
      a probability is exp(s_j - m) / sum_l exp(s_l - m).  The score error enters the numerator and the denominator once
      each (2 e_s); the row sum of T positive terms adds T 2^-24 and the division and the final sum over the keys as much
      again (T 2^-23); the subtraction s - m rounds by 2^-24 |x| and the hardware exponential is within (|x| + 2) 2^-24 for
      |x| <= 104, together (2 |x| + 2) 2^-24 <= 2^-17 for |x| <= 63, once for the numerator and once for the denominator
      (2^-16).  A probability below e^-63 falls under FLOOR below.
  eps_b(i) = e_s(i) + |lse_used_i - lse_ref_i| + 2^-17
      the backward's probability exp(s - lse): the score error, the error of the lse it was GIVEN, one exponential
  eta(i)  = 2 eps_b(i) + (T + 2 dh) 2^-23
      dS = P (dP - D): P is off by eps_b, dP (a dh-term fp32 dot product) by dh 2^-24 a_ij, D (T terms of P dP) by
      (eps_b + dh 2^-24 + T 2^-24) sum_l P_il a_il, with a_ij = mask_ij |dO_i| . |V_j| >= |dP_ij|; the final sum over T
      terms adds T 2^-24
Forward:
  |O - O^|     <= rel_f (P o mask) |V| + FLOOR,       rel_f = (1 + u)(1 + u_P)(1 + eps) - 1
  |lse - lse^| <= e_s + 2^-23 |lse^| + T 2^-24 + 2^-16
Backward, with G_ij = P_ij (a_ij + sum_l P_il a_il) and E_ij = u_P |dS_ij| + (1 + u_P) eta(i) G_ij:
  |dV - dV^| <= sum_i rel_b(i) (P o mask)_ij |dO_i| + FLOOR,   rel_b(i) = (1 + u)(1 + u_P)(1 + eps_b(i) + T 2^-24) - 1
  |dQ - dQ^| <= u |dQ^| + (1 + u) scale E |K| + FLOOR
  |dK - dK^| <= u |dK^| + (1 + u) scale E^T |Q| + FLOOR
Two terms beyond the first-order statement u + u_P + eps, each with its reason:
  * the products (1 + u)(1 + u_P)(1 + eps): a rounding acts on the value that already carries the earlier errors, so the
    storage rounding of x = x^ + err is bounded by u (|x^| + |err|), not by u |x^| -- second order, kept so that the bound
    is a theorem and no constant has to absorb it;
  * FLOOR = 2^-80 (absolute): fp32 flushes products below 2^-126 to zero, and a probability below e^-63 (4e-28) may have a
    relative error above 2^-17 (its exponent |x| > 63, but at most 2^-16 up to |x| = 104, where fp32 is long at zero);
    with at most 256 such terms, each times operand products below 2^18 (|dO| . |V| over dh <= 128 columns, times |K|),
    this stays under 256 * 4e-28 * 2^-16 * 2^18 < 2^-80.  No output of these inputs is resolved anywhere near that.
Nothing here was fitted to a kernel's output: tests/test_attention_bounds_cpu.py shows that a plain fp32 emulation of each
path's arithmetic stays inside, and that six one-line bugs fall outside."""
import math
import zlib
from collections import namedtuple

import torch

DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
U = {"bf16": 2.0 ** -8, "fp32": 2.0 ** -24}
FLOOR = 2.0 ** -80
DROP = (0.3, 0x51, 7, None)            # (p, seed, step, step_dev) of the cases that run the _drop entry points
MAX_T, MAX_DH, LDS_LIMIT = 256, 128, 160 * 1024

# opt: misalign = "qkv" (qkv at a 2-byte-odd offset: both directions leave the MFMA domain) or "dqkv" (only the backward
# does), drop = True (p = 0.3), nt / two_pass / qsplit = what the dispatch arithmetic must give for this shape
Case = namedtuple("Case", "name dt B T H dh family fwd bwd opt")


def _c(tag, dt, B, T, H, dh, family, fwd, bwd, **opt):
    name = f"{tag}_{dt}_b{B}h{H}_T{T}_dh{dh}_{family}"
    if opt.get("drop"):
        name += "_drop"
    if opt.get("misalign"):
        name += "_mis_" + opt["misalign"]
    return Case(name, dt, B, T, H, dh, family, fwd, bwd, opt)


MFMA_T = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 223, 224, 225, 255, 256)
_NT = lambda T: 4 if T <= 64 else 8 if T <= 128 else 14 if T <= 224 else 16


def _build_table():
    t = []
    # ---- bf16, dh = 64, one-pass MFMA forward: every key-tile count edge, T % 16 in {15, 0, 1} --------------------------
    for T in MFMA_T:
        t.append(_c("mfma1p", "bf16", 1, T, 1, 64, "gauss", "attn_mfma", "attn_mfma", nt=_NT(T), two_pass=False,
                    qsplit=(T + 63) // 64))
        for fam in ("gauss", "peaked", "offset") + (("negative",) if T % 16 else ()):
            t.append(_c("mfma1p", "bf16", 2, T, 2, 64, fam, "attn_mfma", "attn_mfma", nt=_NT(T), two_pass=False,
                        qsplit=(T + 63) // 64))
    t.append(_c("mfma1p", "bf16", 64, 50, 4, 64, "gauss", "attn_mfma", "attn_mfma", nt=4, two_pass=False, qsplit=1))
    t.append(_c("mfma1p", "bf16", 127, 129, 1, 64, "gauss", "attn_mfma", "attn_mfma", nt=14, two_pass=False, qsplit=2))
    t.append(_c("mfma1p", "bf16", 127, 129, 1, 64, "negative", "attn_mfma", "attn_mfma", nt=14, two_pass=False, qsplit=2))
    # ---- bf16, dh = 64, eight-wave two-pass forward (B H ceil(T / 128) >= 256, T > 64); the backward is attn_mfma -------
    for B, H, T, qs in ((128, 1, 129, 2), (32, 8, 65, 1), (32, 8, 128, 1), (16, 8, 129, 2), (16, 8, 224, 2),
                        (16, 8, 225, 2), (16, 8, 255, 2), (16, 8, 256, 2), (64, 4, 200, 1)):
        fams = ["gauss"] + (["negative"] if T % 16 else [])
        if (B, H, T) in ((128, 1, 129), (32, 8, 65), (16, 8, 225), (16, 8, 256)):
            fams += ["peaked", "offset"]
        for fam in fams:
            t.append(_c("mfma2p", "bf16", B, T, H, 64, fam, "attn_mfma_2p", "attn_mfma", nt=_NT(T), two_pass=True, qsplit=qs))
    # ---- bf16 outside the MFMA domain: the fp32-VALU kernels on bf16 storage --------------------------------------------
    for dh in (32, 80):
        for T, fam in ((50, "gauss"), (65, "gauss"), (65, "peaked"), (65, "negative"), (65, "offset")):
            t.append(_c("valu", "bf16", 2, T, 3, dh, fam, "attn_valu", "attn_valu"))
    for T, fam in ((50, "gauss"), (129, "gauss"), (129, "negative"), (129, "peaked")):
        t.append(_c("valu", "bf16", 2, T, 2, 64, fam, "attn_valu", "attn_valu", misalign="qkv"))
        t.append(_c("mixed", "bf16", 2, T, 2, 64, fam, "attn_mfma", "attn_valu", misalign="dqkv"))
    # ---- fp32: a sparse cross of dh in {1, 8, 36, 63, 64, 65, 128} and T in {1, 3, 4, 5, 63, 64, 65, 200, 256} ---------
    for T, dh in ((1, 8), (1, 64), (3, 1), (3, 65), (4, 36), (4, 128), (5, 65), (5, 8), (63, 64), (63, 36), (64, 63),
                  (64, 65), (65, 128), (65, 1), (200, 64), (200, 36), (256, 8), (256, 65), (256, 63)):
        t.append(_c("valu", "fp32", 2, T, 3, dh, "gauss", "attn_valu", "attn_valu"))
    for T, dh in ((5, 65), (63, 64), (65, 128), (65, 1), (200, 36)):
        for fam in ("peaked", "negative", "offset"):
            t.append(_c("valu", "fp32", 2, T, 3, dh, fam, "attn_valu", "attn_valu"))
    # the largest shapes each direction's LDS budget admits: the backward holds two more row buffers than the forward
    # (csrc/attention.hip fwd_lds / bwd_lds), so T = 256 ends at dh = 72 for the backward and 76 for the forward, and
    # dh = 128 at T = 144 for the backward and 152 for the forward ("-" = that direction refuses the shape)
    t.append(_c("valu", "fp32", 1, 256, 2, 72, "gauss", "attn_valu", "attn_valu"))
    t.append(_c("valu", "fp32", 1, 144, 2, 128, "gauss", "attn_valu", "attn_valu"))
    t.append(_c("valu", "fp32", 1, 152, 2, 128, "gauss", "attn_valu", "-"))
    t.append(_c("valu", "fp32", 1, 256, 2, 73, "gauss", "attn_valu", "-"))
    t.append(_c("valu", "fp32", 1, 256, 2, 76, "gauss", "attn_valu", "-"))
    # ---- the _drop entry points (p = 0.3): one case per path and per key-tile instance ----------------------------------
    for T in (50, 127, 223, 255):
        t.append(_c("mfma1p", "bf16", 2, T, 2, 64, "gauss", "attn_mfma", "attn_mfma", drop=True, nt=_NT(T), two_pass=False))
    for B, H, T in ((32, 8, 65), (16, 8, 129), (16, 8, 225)):
        t.append(_c("mfma2p", "bf16", B, T, H, 64, "gauss", "attn_mfma_2p", "attn_mfma", drop=True, nt=_NT(T), two_pass=True))
    t.append(_c("valu", "bf16", 2, 50, 3, 32, "gauss", "attn_valu", "attn_valu", drop=True))
    t.append(_c("valu", "fp32", 2, 65, 3, 36, "gauss", "attn_valu", "attn_valu", drop=True))
    t.append(_c("mixed", "bf16", 2, 65, 2, 64, "gauss", "attn_mfma", "attn_valu", drop=True, misalign="dqkv"))
    return t


CASES = _build_table()


def group_of(c):
    """the test function of tests/test_attention_edges_gpu.py a case runs under (a partition of the table)"""
    if c.opt.get("drop"):
        return "dropout"
    if c.dt == "fp32":
        return "fp32_valu"
    if c.bwd == "attn_valu":
        return "bf16_valu"
    return "mfma_two_pass" if c.fwd == "attn_mfma_2p" else "mfma_one_pass"
BY_NAME = {c.name: c for c in CASES}

# shapes both directions must refuse ("-"), or only the backward: (dt, B, T, H, dh, forward, backward)
REFUSALS = [
    ("bf16", 1, 257, 1, 64, "-", "-"),
    ("fp32", 1, 257, 1, 8, "-", "-"),
    ("bf16", 1, 16, 1, 129, "-", "-"),
    ("fp32", 1, 16, 1, 129, "-", "-"),
    ("fp32", 1, 256, 1, 77, "-", "-"),
    ("fp32", 1, 153, 1, 128, "-", "-"),
    ("fp32", 1, 256, 1, 73, "attn_valu", "-"),
    ("fp32", 1, 256, 1, 76, "attn_valu", "-"),
]


# ---- the dispatch arithmetic of the two .hip files, restated -----------------------------------------------------------
def valu_lds(T, dh):
    """(forward, backward) dynamic LDS bytes of the VALU kernels"""
    kv = 2 * T * (dh + 1)
    return (kv + 4 * MAX_T + 4 * MAX_DH) * 4, (kv + 8 * MAX_T + 8 * MAX_DH + 2 * MAX_T) * 4


def dispatch(dt, B, T, H, dh, misalign=None):
    """what ib_attention_fwd / ib_attention_bwd do with a shape: {"fwd", "bwd": path names, "nt", "two_pass", "qsplit" of the
    MFMA forward, "lds_fwd", "lds_bwd": dynamic LDS bytes of the launched kernels}"""
    r = {"fwd": "-", "bwd": "-", "nt": None, "two_pass": None, "qsplit": None, "lds_fwd": None, "lds_bwd": None}
    if T > MAX_T or dh > MAX_DH:
        return r
    lf, lb = valu_lds(T, dh)
    mfma = dt == "bf16" and dh == 64
    if mfma and misalign != "qkv":                                   # forward: qkv and out 16-byte aligned
        nt = _NT(T)
        bh = B * H
        two = nt > 4 and bh * ((T + 127) // 128) >= 256
        groups = (T + 127) // 128 if two else (T + 63) // 64
        r.update(fwd="attn_mfma_2p" if two else "attn_mfma", nt=nt, two_pass=two,
                 qsplit=1 if bh >= 256 else min(groups, max(1, 256 // bh)), lds_fwd=2 * nt * 16 * 72 * 2)
    elif lf <= LDS_LIMIT:
        r.update(fwd="attn_valu", lds_fwd=lf)
    if mfma and misalign is None:                                    # backward: qkv, out, dout and dqkv aligned
        nt = _NT(T)
        r.update(bwd="attn_mfma", lds_bwd=4 * nt * 16 * 72 * 2 + 2 * nt * 16 * 4)
    elif lb <= LDS_LIMIT:
        r.update(bwd="attn_valu", lds_bwd=lb)
    return r


# ---- inputs ------------------------------------------------------------------------------------------------------------
Inputs = namedtuple("Inputs", "qkv dout H dh")


def make_inputs(dt, B, T, H, dh, family, seed):
    """seeded on the CPU and rounded to the storage dtype (the reference sees what the kernels see)
    gauss     N(0, 1)
    peaked    q and k scaled by 4: a near one-hot softmax and a large row maximum
    negative  q_i = c + 0.3 noise with one c ~ 1.5 N(0, 1) per (window, head), k_j = -mean_i(q_i) + 0.1 noise: every real
              score is near -1.5^2 sqrt(dh) << 0, so a zero-score padding key, or one left unmasked, would own the row
    offset    V = N(0, 1) + 8: dP is almost constant along a row and dS = P (dP - D) cancels"""
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, T, H, dh, generator=g, dtype=torch.float64) for _ in range(3))
    dout = torch.randn(B, T, H * dh, generator=g, dtype=torch.float64)
    if family == "peaked":
        q, k = 4 * q, 4 * k
    elif family == "negative":
        c = 1.5 * torch.randn(B, 1, H, dh, generator=g, dtype=torch.float64)
        q = c + 0.3 * q
        k = -q.mean(1, keepdim=True) + 0.1 * k
    elif family == "offset":
        v = v + 8
    elif family != "gauss":
        raise ValueError(family)
    qkv = torch.cat([x.reshape(B, T, H * dh) for x in (q, k, v)], -1).to(DT[dt])
    return Inputs(qkv, dout.to(DT[dt]), H, dh)


def case_inputs(c):
    return make_inputs(c.dt, c.B, c.T, c.H, c.dh, c.family, zlib.crc32(c.name.encode()))


def heads(x, H):
    """[B, T, H dh] -> float64 [B H, T, dh]"""
    B, T, d = x.shape
    return x.double().reshape(B, T, H, d // H).permute(0, 2, 1, 3).reshape(B * H, T, d // H)


def unheads(x, B):
    """[B H, T, dh] -> [B, T, H dh]"""
    N, T, dh = x.shape
    return x.reshape(B, N // B, T, dh).permute(0, 2, 1, 3).reshape(B, T, (N // B) * dh)


def ref_lse(x):
    """float64 [B, H, T]"""
    B, T, d3 = x.qkv.shape
    d = d3 // 3
    q, k = heads(x.qkv[..., :d], x.H), heads(x.qkv[..., d:2 * d], x.H)
    return torch.logsumexp((q @ k.transpose(1, 2)) / math.sqrt(x.dh), -1).reshape(B, x.H, T)


def evaluate(x, dt, up_fwd, up_bwd, mask=None, lse_used=()):
    """The float64 reference and the bounds of the module docstring.  up_fwd / up_bwd: u_P of the path each direction took;
    mask: [B, H, T, T] multipliers or None; lse_used: the lse tensors [B, H, T] a backward was run with.  Returns
    ref = {O, lse, dqkv} and bound = {O, lse, dqkv: [one per lse_used]}, in the kernels' layouts (float64)."""
    B, T, d3 = x.qkv.shape
    d, H, dh = d3 // 3, x.H, x.dh
    N = B * H
    u, scale = U[dt], 1.0 / math.sqrt(dh)
    Q, K, V = (heads(x.qkv[..., i * d:(i + 1) * d], H) for i in range(3))
    dO = heads(x.dout, H)
    M = None if mask is None else mask.double().reshape(N, T, T)
    lse_ref = torch.empty(N, T, dtype=torch.float64)
    ref = {k: torch.empty(N, T, dh, dtype=torch.float64) for k in ("O", "dQ", "dK", "dV")}
    bO, bl = torch.empty(N, T, dh, dtype=torch.float64), torch.empty(N, T, dtype=torch.float64)
    bb = [{k: torch.empty(N, T, dh, dtype=torch.float64) for k in ("dQ", "dK", "dV")} for _ in lse_used]
    used = [l.double().reshape(N, T) for l in lse_used]
    step = max(1, (1 << 21) // (T * T))                              # (window, head) pairs per chunk: ~16 MB per T x T array
    for n0 in range(0, N, step):
        s = slice(n0, min(N, n0 + step))
        q, k, v, do = Q[s], K[s], V[s], dO[s]
        S = scale * (q @ k.transpose(1, 2))
        lse = torch.logsumexp(S, -1)
        P = torch.exp(S - lse[..., None])
        Pm = P if M is None else P * M[s]
        dP = do @ v.transpose(1, 2)
        a = do.abs() @ v.abs().transpose(1, 2)
        if M is not None:
            dP, a = dP * M[s], a * M[s]
        dS = P * (dP - (P * dP).sum(-1, keepdim=True))
        lse_ref[s] = lse
        ref["O"][s], ref["dV"][s] = Pm @ v, Pm.transpose(1, 2) @ do
        ref["dQ"][s], ref["dK"][s] = scale * (dS @ k), scale * (dS.transpose(1, 2) @ q)
        e_s = dh * 2.0 ** -23 * scale * (q.abs() @ k.abs().transpose(1, 2)).amax(-1)          # [n, T]
        eps = 2 * e_s + T * 2.0 ** -23 + 2.0 ** -16
        rel_f = (1 + u) * (1 + up_fwd) * (1 + eps) - 1
        bO[s] = rel_f[..., None] * (Pm @ v.abs()) + FLOOR
        bl[s] = e_s + 2.0 ** -23 * lse.abs() + T * 2.0 ** -24 + 2.0 ** -16
        G = P * (a + (P * a).sum(-1, keepdim=True))
        for lu, b in zip(used, bb):
            eps_b = e_s + (lu[s] - lse).abs() + 2.0 ** -17
            eta = 2 * eps_b + (T + 2 * dh) * 2.0 ** -23
            rel_b = (1 + u) * (1 + up_bwd) * (1 + eps_b + T * 2.0 ** -24) - 1
            b["dV"][s] = (rel_b[..., None] * Pm).transpose(1, 2) @ do.abs() + FLOOR
            E = up_bwd * dS.abs() + (1 + up_bwd) * eta[..., None] * G
            b["dQ"][s] = u * ref["dQ"][s].abs() + (1 + u) * scale * (E @ k.abs()) + FLOOR
            b["dK"][s] = u * ref["dK"][s].abs() + (1 + u) * scale * (E.transpose(1, 2) @ q.abs()) + FLOOR
    pack = lambda r: torch.cat([unheads(r["dQ"], B), unheads(r["dK"], B), unheads(r["dV"], B)], -1)
    return ({"O": unheads(ref["O"], B), "lse": lse_ref.reshape(B, H, T), "dqkv": pack(ref)},
            {"O": unheads(bO, B), "lse": bl.reshape(B, H, T), "dqkv": [pack(b) for b in bb]})


def up_of(path):
    return U["bf16"] if path in ("attn_mfma", "attn_mfma_2p") else 0.0


def violations(what, got, ref, bound, H, path):
    """(None or a failure message, the largest error / bound).  got / ref / bound: [B, T, H dh], [B, T, 3 H dh] or [B, H, T]"""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    fin = torch.isfinite(got)
    if not fin.all():
        return f"{what}: {int((~fin).sum())} elements not finite (left unwritten, or poisoned by an out-of-range read); path {path}", math.inf
    err = (got - ref).abs()
    ratio = float((err / bound).max())
    bad = err > bound
    if not bad.any():
        return None, ratio
    i = tuple(bad.nonzero()[0].tolist())
    if what == "lse":
        where = f"(window {i[0]}, row {i[2]}, head {i[1]})"
    else:
        dh = got.shape[-1] // H // (3 if what == "dqkv" else 1)
        part = ("dQ", "dK", "dV")[i[2] // (H * dh)] + " " if what == "dqkv" else ""
        c = i[2] % (H * dh)
        where = f"{part}(window {i[0]}, row {i[1]}, head {c // dh}, column {c % dh})"
    return (f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bound, first at {where}: got {got[i].item()!r}, "
            f"reference {ref[i].item()!r}, bound {bound[i].item():.3e}, worst error / bound {ratio:.3g}; path {path}"), ratio
