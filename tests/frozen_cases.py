"""Shared by tests/test_frozen_kernels_gpu.py and tests/test_frozen_bounds_cpu.py: the case table of the frozen-weight layer
kernels (csrc/linln_panel.hip, the INFER form of csrc/ffn_chain.hip, ib_linear_ln_fwd of csrc/gemm.hip), their launch
geometry restated in Python, the seeded INTEGER inputs, the exact references, the float64 LayerNorm reference and the
ELEMENTWISE bound every LayerNorm output is held to, and the checks themselves (check: the GPU's outputs and the CPU
emulation's go through the same function).  The conventions are those of tests/batchnorm_cases.py and tests/rowops_cases.py:
u = U32 = 2^-24, the unit roundoff of fp32; UB16 = 2^-8 for a value stored as bf16; one untuned safety factor S = 2 on the
whole bound; a bound of exactly 0 admits only the exact value.

Families (every one at d = 512) and what is compared:
  linln_panel   ib_linear_ln_panel_fwd   y = LN(res + x W^T + bias)                       y: bound (two-pass, n = 13)
  linear_panel  ib_linear_panel_fwd      y = x W^T + bias, chunks x 512 columns            y: bit for bit
  ffn_infer     ib_ffn_infer_fwd         y = LN(x1 + relu(x1 W1^T + b1) W2^T + b2)         the fp32 slabs in the workspace bit for
                                         bit (slab c SUB + sb = hidden columns 512 c + (512 / SUB) sb ... of the product);
                                         y: bound (two-pass, n = 8)
  chain         ib_ffn_chain_fwd_infer   x1 = LN1(x + attn Wo^T + bo), y = LN2(x1 + FFN(x1)), qkv = y Wqkv^T + bqkv
                                         y: bound (ONE-pass, n = 13) on the exact s2; qkv: bound on the kernel's own y
  linear_ln     ib_linear_ln_fwd         y = LN(res + x W^T + bias), a_out, mean, rstd      the sum of the slabs and a_out bit for
                                         bit, the slab count; y, mean, rstd: bound (two-pass, n = 4 NCH - 1 + log2 LPR)

Integer inputs: rows (x, attn, res, x1) are small integers, weights are in {-1, 0, +1} with a density chosen per matrix
(every 16-column x 32-k block of every weight holds a nonzero: no MFMA operand block is dead), biases small integers.  Every
product and every partial sum is an integer below 2^24 (exact_gemm asserts |a| @ |b|^T < 2^24 over the WHOLE reduction, which
covers every order, split and slab), so the GEMMs are exact in fp32 on the CPU and on the GPU.  Every value a kernel keeps
as bf16 before a LayerNorm -- the hidden activation h, s1 and s2 of the chain, a_out -- is an integer (or, s1 and x of the
chain, a half-integer below 128) of magnitude <= 256: the store rounds nothing (assert_bf16_exact).  So the input v of
every LayerNorm is EXACT, and the bound below has no input term.

The chain saves nothing, so its LN1 is made bit-predictable: x is built so that s1 = x + attn Wo^T + bo is, per row, +-c
with exactly 256 columns of each sign, c = 1/2, 1, 2, 4 by row.  Then mean = 0 and E[v^2] = c^2 exactly, rstd = (1 - delta) / c
with delta ~ eps / (2 c^2) <= 2e-5 and a few ulp, and with ODD integer gamma1 and EVEN integer beta1
x1 = bf16(+-gamma1 (1 - delta) + beta1) = +-gamma1 + beta1 exactly (an odd integer: never a cancellation to a tiny nonzero).
From x1 on the feed-forward is exact as above.  One hidden unit (JSTAR) reads a fixed sign pattern that every seventh
row carries and feeds all 512 outputs: those rows of s2 carry a common offset of ~ 128.
Zero-variance rows of the ONE-pass kernel: every eleventh row of the chain (from row 3) has s1 = c in all 512 columns.  Its
mean is c and E[v^2] - mean^2 is 0 exactly under either contraction, so x1 = beta1 bit for bit, whatever rsq(eps) returns.
b1 = -beta1 W1^T silences every hidden unit but JSTAR on those rows, JSTAR adds CHAIN_ZV_H = 20 to every output and
b2 = 7 - beta1, so s2 = 27 in all columns: LN2 meets var = 0 at a nonzero mean, and y = beta.  An omitted eps gives NaN.
The two-pass kernels: zero-variance rows and rows offset by 200 are in the linln_panel and linear_ln tables (through res).
ffn_infer: the x1 = 0 rows are constant (b2 = 7 - relu(b1) W2^T: s = 7), and its own JSTAR unit offsets the rows that
carry twice its pattern by ~ 128 (x1 is also the GEMM input: an offset in x1 itself would push h past 256).

The LayerNorm bound, counted from the code (v exact, N columns, float64 reference mean, d = v - mean, var, rstd, y):
  row sums: n additions on the longest path, each on a partial sum no larger than the sum of the absolute terms
      linln_panel_kernel   ((v0 + v1) + (v2 + v3)) + ((v4 + v5) + (v6 + v7)) per lane, 6 DPP levels:        n = 7 + 6 = 13
      slab_ln_kernel<LPR, NCH>   (x + y) + (z + w) per chunk added to the lane's sum, log2 LPR shuffles:    n = 4 NCH - 1 + log2 LPR
      ff_ln_rows_fwd       two interleaved chains of 4, their sum, 6 DPP levels:                            n = 7 + 6 = 13
  e_mean = (n + 2) u sum|v| / N                       (1 / N rounded and multiplied; exact for these N, kept)
  two-pass (linln_panel_kernel, slab_ln_kernel; `1.f / sqrtf`), w = e_mean:
      e_var = (sum (2 |d| w + w^2 + 3 u d^2) + n u sum d^2) / N + 2 u var
  one-pass (ff_ln_rows_fwd: E[v^2] - mean^2, clamped at 0, hardware rsq taken as 1 ulp = 2 u):
      e_var = (n + 3) u sum v^2 / N + 2 |mean| e_mean + e_mean^2 + u mean^2 + u var
      the first term is the cancellation term: it scales with E[v^2], not with var.  u mean^2 + u var covers both
      contractions the compiler makes of it: fma(-mean, mean, E2) and fma(sq, 1 / N, -fl(mean^2))
  rstd: NOT first order (a zero-variance row has e_var ~ eps):  the computed variance lies in [max(var - e_var, 0), var + e_var],
      e_rstd = max(hi - rstd, rstd - lo) + 3 u hi,  hi = 1 / sqrt(max(var - e_var, 0) + eps),  lo = 1 / sqrt(var + e_var + eps)
      (3 u: the addition of eps, the square root, the division -- or the addition and the 1-ulp rsq)
  e_y = |gamma| (|d| e_rstd + w (rstd + e_rstd) + 3 u |d| rstd) + (u + UB16) |y|, and 0 where gamma = 0 (y = beta exactly; every
      beta is a bf16 value).  A zero-variance row is held to beta exactly too: its integer sums are exact, so mean = v, d = 0
  mean and rstd (ib_linear_ln_fwd) are held to e_mean and e_rstd.  All of it times S.
The QKV tail: against ref = y_kernel Wqkv^T + bqkv in float64 from the kernel's OWN y, bound S (512 u (|y| @ |W|^T) + UB16 |ref|).
No figure here is tuned to a GPU result."""
import functools
import math
import zlib
from collections import namedtuple

import torch

from tests.batchnorm_cases import S, U32, UB16, violations  # noqa: F401  (violations is re-exported)

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EPS = float(torch.tensor(1e-5, dtype=torch.float32))
D = 512
FF_ROWS, FF_CHUNK, FF_MAXCHUNK = 64, 512, 8
IB_OK, IB_E_ARG, IB_E_WORKSPACE, IB_E_UNSUPPORTED = 0, -1, -4, -5
IB_F32, IB_BF16 = 0, 1
PATH_NONE, PATH_LINLN, PATH_NT_SPLITK, PATH_FFN_CHAIN, PATH_LINLN_PANEL, PATH_FFN_INFER, PATH_LIN_PANEL = 0, 9, 13, 14, 15, 16, 17
JSTAR, JSTAR_COLS, CHAIN_OFFSET_EVERY, CHAIN_ZV_EVERY, CHAIN_ZV_H = 5, 64, 7, 11, 20.0


def cdiv(a, b):
    return -(-a // b)


# ---- launch geometry, restated from the C code ------------------------------------------------------------------------------
def linln_panel_workgroups(M, N=D, K=D):
    """ib_linear_ln_panel_workgroups -> (workgroups, rows per panel); (0, 0): unsupported"""
    if M <= 0 or N != D or K != D:
        return 0, 0
    P = cdiv(M, 256)
    if P > 32:
        return 0, 0
    return cdiv(M, P), P


def lin_panel_geometry(M, chunks):
    """lin_panel_geometry -> (panels, rows per panel, column blocks per chunk); panels = 0: unsupported"""
    if M <= 0 or chunks < 1 or chunks > 8 or M > 8192:
        return 0, 0, 1
    rows = min(max(cdiv(M, 256 // chunks), 16), FF_ROWS)
    panels = cdiv(M, rows)
    return panels, rows, (4 if rows == 16 and panels * chunks * 4 <= 320 else 1)


def linear_panel_workgroups(M, N, K):
    if K != D or N <= 0 or N % FF_CHUNK:
        return 0
    panels, _, subs = lin_panel_geometry(M, N // FF_CHUNK)
    return panels * (N // FF_CHUNK) * subs


def ffn_coop_geometry(M, d, ffn):
    """ffn_coop_geometry -> (panels, rows per panel, hidden chunks, sub-chunks per chunk); panels = 0: unsupported"""
    if M <= 0 or d != D or ffn <= 0 or ffn % FF_CHUNK or ffn // FF_CHUNK > FF_MAXCHUNK or M > 32768:
        return 0, 0, 0, 1
    nc = ffn // FF_CHUNK
    rows = min(max(cdiv(M, 256 // nc), 16), FF_ROWS)
    panels = cdiv(M, rows)
    sb = 1
    if rows == 16:
        sb = 4 if panels * nc * 4 <= 320 else 2 if panels * nc * 2 <= 320 else 1
    return panels, rows, nc, sb


def ffn_infer_workspace(M, d, ffn):
    panels, _, nc, sb = ffn_coop_geometry(M, d, ffn)
    return nc * sb * M * D * 4 if panels else 0


def ffn_geometry(M, d, ffn):
    """ffn_geometry with T_att = 0 -> (workgroups, rows per panel, hidden chunks); workgroups = 0: unsupported"""
    if d != D or ffn <= 0 or ffn % FF_CHUNK or ffn // FF_CHUNK > FF_MAXCHUNK or M <= 0:
        return 0, 0, 0
    rows = min(cdiv(M, 256), FF_ROWS)
    if rows < 16:
        rows = M if M < 16 else 16
    return cdiv(M, rows), rows, ffn // FF_CHUNK


def linear_ln_split(M, N, K):
    """linear_ln_split (gemm.hip, 128 x 128 tiles) -> (slabs of the ring producer, its k chunk)"""
    tiles = cdiv(M, 128) * cdiv(N, 128)
    want = max(min(cdiv(384, tiles), K // 128), 1)
    chunk = cdiv(cdiv(K, want), 32) * 32
    return cdiv(K, chunk), chunk


def nt_splitk_splits(M, N, K):
    """ib_gemm_nt_splitk_splits (gemm_nt.hip, 256 x 128 tiles, k steps of 64); 0: the ring producer"""
    if M < 640 or N < 128 or N % 8 or K % 64:
        return 0
    tiles = cdiv(M, 256) * cdiv(N, 128)
    best = 0
    for sp in range(2, 17):
        if K % (sp * 64) or K // sp < 4 * 64:
            continue
        if tiles * sp <= 256:
            best = sp
    return best


SLAB_LN = {64: (16, 1), 128: (16, 2), 256: (64, 1), 512: (64, 2), 1024: (64, 4)}     # N: (LPR, NCH), the switch of ib_linear_ln_fwd


def linear_ln_supported(M, N, K, dtype=IB_BF16):
    """ib_linear_ln_fwd's own check (bf16, N of the switch, K % 32 == 0) and ring_ok's red_len >= 64, which refuses K = 32
    behind it, still before any launch (M < 640: no NT producer)"""
    return dtype == IB_BF16 and N in SLAB_LN and K % 32 == 0 and K >= 64


def linear_ln_plan(M, N, K):
    """-> (producer, slabs written, slabs the workspace query asks for)"""
    split, _ = linear_ln_split(M, N, K)
    nts = nt_splitk_splits(M, N, K)
    return ("nt_splitk", nts, max(split, nts)) if nts >= 2 else ("ring", split, max(split, nts))


# ---- the case table --------------------------------------------------------------------------------------------------------
# kernel: the instantiation the case is in the table for; kernel_of re-derives it from the restated C predicates, and
# tests/test_frozen_bounds_cpu.py fails a case that lands elsewhere.  ld*: row pitches in elements (0: the entry point takes
# none).  tail: the chain's QKV tail.  saved: a_out, mean, rstd of ib_linear_ln_fwd.  cross: the chain's training form is run on
# the same inputs.
Case = namedtuple("Case", "fam name M N K ffn chunks bias res ldx ldres ldy tail saved cross kernel")
CASES = []


def _add(fam, M, kernel, N=D, K=D, ffn=0, chunks=0, bias=True, res=False, ldx=0, ldres=0, ldy=0, tail=False, saved=False,
         cross=False, tag=""):
    name = f"{fam}_{M}" + (f"_N{N}_K{K}" if fam == "linear_ln" else "") + (f"_ffn{ffn}" if ffn else "") \
        + (f"_chunks{chunks}" if chunks else "") + tag
    CASES.append(Case(fam, name, M, N, K, ffn, chunks, bias, res, ldx, ldres, ldy, tail, saved, cross, kernel))


# linln_panel: P = ceil(M / 256) goes 1 -> 2 at 256 / 257; MT 1 -> 2 (P <= 16) at 4096 / 4097; 4100: P = 17, the last panel has 3
# rows and its second row tile is empty.  x / res / y pitches 520 / 516 / 520; the option variants at 512.
for _M, _k in ((1, "linln_panel<1>"), (256, "linln_panel<1>"), (257, "linln_panel<1>"), (4096, "linln_panel<1>"),
               (4097, "linln_panel<2>"), (4100, "linln_panel<2>"), (8192, "linln_panel<2>")):
    _add("linln_panel", _M, _k, res=True, ldx=520, ldres=516, ldy=520)
for _M, _k in ((257, "linln_panel<1>"), (4100, "linln_panel<2>")):
    for _b, _r in ((True, False), (False, True), (False, False)):
        _add("linln_panel", _M, _k, bias=_b, res=_r, ldx=512, ldres=512, ldy=512,
             tag="_" + ("b" if _b else "") + ("r" if _r else "") + ("plain" if not (_b or _r) else ""))
# linear_panel, chunks = 3: 128-column blocks (subs 4) up to 26 panels = 416 rows; 16-row panels up to 85 x 16 = 1360 rows; two
# row tiles up to 2720, four beyond; the 64-row clamp at 5440 / 5441.  chunks = 1: subs 4 -> 1 at 1280 / 1281; chunks = 8: at 160 / 161.
for _M, _k in ((1, "linear_panel<1,1>"), (416, "linear_panel<1,1>"), (417, "linear_panel<1,4>"), (1360, "linear_panel<1,4>"),
               (1361, "linear_panel<2,4>"), (2720, "linear_panel<2,4>"), (2721, "linear_panel<4,4>"), (5440, "linear_panel<4,4>"),
               (5441, "linear_panel<4,4>"), (8192, "linear_panel<4,4>")):
    _add("linear_panel", _M, _k, N=3 * D, chunks=3, ldx=520, ldy=3 * D + 4)
_add("linear_panel", 417, "linear_panel<1,4>", N=3 * D, chunks=3, bias=False, ldx=512, ldy=3 * D, tag="_nobias")
_add("linear_panel", 1361, "linear_panel<2,4>", N=3 * D, chunks=3, bias=False, ldx=512, ldy=3 * D, tag="_nobias")
for _ch, _rows in ((1, ((1280, "linear_panel<1,1>"), (1281, "linear_panel<1,4>"), (1277, "linear_panel<1,1>"))),
                   (8, ((160, "linear_panel<1,1>"), (161, "linear_panel<1,4>"), (171, "linear_panel<1,4>")))):
    for _M, _k in _rows:
        _add("linear_panel", _M, _k, N=_ch * D, chunks=_ch, ldx=520, ldy=_ch * D + 4)
# ffn_infer, ffn = 2048: SUB 4 -> 2 at 320 / 321, 2 -> the 64-row kernel's 16-row panels at 640 / 641, rows 16 -> 17 at 1024 / 1025, a
# second round of workgroups (65 panels x 4 chunks) at 4097; one ragged M per regime.  ffn = 512: 1280 / 1281 and 2560 / 2561;
# ffn = 4096: 160 / 161 and 320 / 321.
for _ffn, _rows in ((2048, ((1, "coop_small<4>"), (307, "coop_small<4>"), (320, "coop_small<4>"), (321, "coop_small<2>"),
                            (631, "coop_small<2>"), (640, "coop_small<2>"), (641, "coop"), (1000, "coop"), (1024, "coop"),
                            (1025, "coop"), (2500, "coop"), (4096, "coop"), (4097, "coop"))),
                    (512, ((1280, "coop_small<4>"), (1281, "coop_small<2>"), (2560, "coop_small<2>"), (2561, "coop"))),
                    (4096, ((160, "coop_small<4>"), (161, "coop_small<2>"), (320, "coop_small<2>"), (321, "coop")))):
    for _M, _k in _rows:
        _add("ffn_infer", _M, _k + "+slab_ln<64,2>", ffn=_ffn)
# chain: panels of M (M < 16), 16, ceil(M / 256) rows, 64 beyond 16384; 8193 = the production edge (33-row panels, the last has 9)
for _ffn in (512, 2048):
    for _M in (1, 15, 16, 17, 4096, 4097, 8193, 16384, 16385):
        _add("chain", _M, "chain_infer", ffn=_ffn, cross=_M in (1, 17, 4097))
    for _M in (1, 15, 16, 17, 8193):
        _add("chain", _M, "chain_infer_qkv", ffn=_ffn, tail=True, cross=_M in (15, 16, 8193), tag="_tail")
# linear_ln: every width of the switch behind both producers, split counts 1 and > 1
for _M, _N, _K, _k, _saved in ((37, 64, 64, "ring/1+slab_ln<16,1>", False), (100, 128, 256, "ring/2+slab_ln<16,2>", True),
                               (300, 256, 512, "ring/4+slab_ln<64,1>", False), (639, 512, 512, "ring/4+slab_ln<64,2>", True),
                               (130, 1024, 160, "ring/1+slab_ln<64,4>", False), (640, 64, 128, "ring/1+slab_ln<16,1>", False),
                               (640, 128, 512, "nt_splitk/2+slab_ln<16,2>", False), (641, 256, 1024, "nt_splitk/4+slab_ln<64,1>", True),
                               (3200, 512, 2048, "nt_splitk/4+slab_ln<64,2>", False), (640, 1024, 512, "nt_splitk/2+slab_ln<64,4>", True)):
    _add("linear_ln", _M, _k, N=_N, K=_K, res=True, ldx=_K + 8, ldres=_N + 4, ldy=_N + 4, saved=_saved)
_add("linear_ln", 300, "ring/4+slab_ln<64,1>", N=256, K=512, bias=False, res=False, ldy=256, saved=True, tag="_plain")
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
FAMILIES = ("linln_panel", "linear_panel", "ffn_infer", "chain", "linear_ln")

# refusals: (what, arguments); every one must return IB_E_UNSUPPORTED with nothing launched
REFUSED = {
    "linln_panel": (("M = 8193", dict(M=8193)),),
    "linear_panel": (("M = 8193", dict(M=8193, chunks=3)), ("chunks = 9", dict(M=64, chunks=9))),
    "ffn_infer": (("M = 32769", dict(M=32769, d=D, ffn=2048)), ("d = 256", dict(M=64, d=256, ffn=2048)),
                  ("ffn = 4608", dict(M=64, d=D, ffn=4608))),
    "chain": (("d = 256", dict(M=64, d=256, ffn=512)), ("ffn = 4608", dict(M=64, d=D, ffn=4608)),
              ("ffn = 768", dict(M=64, d=D, ffn=768))),
    "linear_ln": (("N = 96", dict(N=96, K=128, dtype=IB_BF16)), ("N = 192", dict(N=192, K=128, dtype=IB_BF16)),
                  ("N = 2048", dict(N=2048, K=128, dtype=IB_BF16)), ("K = 48", dict(N=128, K=48, dtype=IB_BF16)),
                  ("fp32", dict(N=128, K=128, dtype=IB_F32))),
}


def case_id(c):
    return c.name


def kernel_of(c):
    """the instantiation a case reaches, from the restated C predicates"""
    if c.fam == "linln_panel":
        _, P = linln_panel_workgroups(c.M)
        return f"linln_panel<{1 if P <= 16 else 2}>"
    if c.fam == "linear_panel":
        _, P, subs = lin_panel_geometry(c.M, c.chunks)
        return "linear_panel<1,1>" if subs == 4 else f"linear_panel<{1 if P <= 16 else 2 if P <= 32 else 4},4>"
    if c.fam == "ffn_infer":
        sb = ffn_coop_geometry(c.M, D, c.ffn)[3]
        return ("coop" if sb == 1 else f"coop_small<{sb}>") + "+slab_ln<64,2>"
    if c.fam == "chain":
        return "chain_infer_qkv" if c.tail else "chain_infer"
    prod, used, _ = linear_ln_plan(c.M, c.N, c.K)
    return f"{prod}/{used}+slab_ln<{SLAB_LN[c.N][0]},{SLAB_LN[c.N][1]}>"


def expected_path(c):
    return {"linln_panel": PATH_LINLN_PANEL, "linear_panel": PATH_LIN_PANEL, "ffn_infer": PATH_FFN_INFER, "chain": PATH_FFN_CHAIN,
            "linear_ln": PATH_NT_SPLITK if c.kernel.startswith("nt") else PATH_LINLN}[c.fam]


def ln_adds(c):
    """(additions on the longest path of a row sum, form) of the LayerNorm a family runs last"""
    if c.fam in ("linln_panel", "chain"):
        return 13, ("two_pass" if c.fam == "linln_panel" else "one_pass")
    LPR, NCH = SLAB_LN[c.N]
    return 4 * NCH - 1 + int(math.log2(LPR)), "two_pass"


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def _gen(key):
    return torch.Generator().manual_seed(zlib.crc32(key.encode()))


def _ints(g, shape, k):
    return torch.randint(-k, k + 1, shape, generator=g).to(F32)


def _tern(g, N, K, p):
    """[N, K] in {-1, 0, +1}, density ~ p, at least one nonzero in every 16 x 32 block"""
    w = (torch.rand(N, K, generator=g) < p).to(F32) * (2 * torch.randint(0, 2, (N, K), generator=g) - 1).to(F32)
    nb, kb = N // 16, K // 32
    r = 16 * torch.arange(nb)[:, None] + torch.randint(0, 16, (nb, kb), generator=g)
    k = 32 * torch.arange(kb)[None, :] + torch.randint(0, 32, (nb, kb), generator=g)
    w[r, k] = (2 * torch.randint(0, 2, (nb, kb), generator=g) - 1).to(F32)
    return w


def _affine(g, N):
    """gamma ~ 1 + 0.5 N(0, 1) with gamma[0] < 0 and two exact zeros; beta: bf16 values"""
    gamma = (1 + 0.5 * torch.randn(N, generator=g)).to(F32)
    gamma[0] = -(0.25 + gamma[0].abs())
    gamma[N - 1] = 0.0
    gamma[N // 2 + 3] = 0.0
    return gamma, torch.randn(N, generator=g).to(BF).to(F32)


def dead_blocks(w):
    """the number of 16-column x 32-k blocks of a weight (= of its packed images) without a nonzero"""
    N, K = w.shape
    return int((w.view(N // 16, 16, K // 32, 32).abs().amax((1, 3)) == 0).sum())


@functools.lru_cache(maxsize=None)
def weights(fam, N=D, K=D, ffn=0):
    """the frozen parameters of a family: fp32 tensors holding the exact (bf16-representable) values"""
    g = _gen(f"weights/{fam}/{N}/{K}/{ffn}")
    if fam in ("linln_panel", "linear_ln", "linear_panel"):
        out = {"w": _tern(g, N, K, 1 / 8), "bias": _ints(g, (N,), 8)}
        if fam != "linear_panel":
            out["gamma"], out["beta"] = _affine(g, N)
        return out
    out = {"w1": _tern(g, ffn, D, 1 / 8 if fam == "ffn_infer" else 1 / 32), "b1": _ints(g, (ffn,), 4),
           "w2": _tern(g, D, ffn, (32 if fam == "ffn_infer" else 8) / ffn), "b2": _ints(g, (D,), 8)}
    out["gamma"], out["beta"] = _affine(g, D)
    if fam == "ffn_infer":
        # the offset unit: hidden unit JSTAR reads the pattern jpat on JSTAR_COLS columns and feeds every output; the rows
        # that carry 2 jpat there are offset by 128 + b1[JSTAR].  b2 makes the x1 = 0 rows constant: s = 7
        out["jcols"] = torch.randperm(D, generator=g)[:JSTAR_COLS]
        out["jpat"] = (2 * torch.randint(0, 2, (JSTAR_COLS,), generator=g) - 1).to(F32)
        out["w1"][JSTAR] = 0.0
        out["w1"][JSTAR, out["jcols"]] = out["jpat"]
        out["w2"][:, JSTAR] = 1.0
        _revive(out["w1"])
        out["b2"] = 7.0 - relu(out["b1"]) @ out["w2"].T
    if fam == "chain":
        out["wo"], out["bo"] = _tern(g, D, D, 1 / 8), _ints(g, (D,), 4)
        out["gamma1"] = (2 * torch.randint(0, 2, (D,), generator=g) + 1).to(F32) * (2 * torch.randint(0, 2, (D,), generator=g) - 1).to(F32)
        out["beta1"] = 2 * _ints(g, (D,), 1)
        out["wqkv"], out["bqkv"] = _tern(g, 3 * D, D, 1 / 8), _ints(g, (3 * D,), 8)
        # the offset unit: hidden unit JSTAR reads sigma* sign(gamma1) on JSTAR_COLS columns, feeds every output
        sig = chain_sigma_star()
        cols = torch.randperm(D, generator=g)[:JSTAR_COLS]
        out["w1"][JSTAR] = 0.0
        out["w1"][JSTAR, cols] = sig[cols] * out["gamma1"][cols].sign()
        out["w2"][:, JSTAR] = 1.0
        _revive(out["w1"])
        # the zero-variance rows have x1 = beta1 (s1 constant): b1 silences every hidden unit but JSTAR on them, JSTAR gives
        # CHAIN_ZV_H to every output, and b2 takes beta1 out again: s2 = CHAIN_ZV_H + 7 on those rows
        out["b1"] = -(out["beta1"] @ out["w1"].T)
        out["b1"][JSTAR] += CHAIN_ZV_H
        out["b2"] = 7.0 - out["beta1"]
    return out


def _revive(w1):
    """the rewritten row JSTAR may have held the only nonzero of its 16 x 32 blocks"""
    for kb in range(D // 32):
        if not w1[:16, 32 * kb:32 * kb + 32].any():
            w1[0, 32 * kb] = 1.0


def chain_sigma_star():
    g = _gen("chain/sigma*")
    return torch.where(torch.argsort(torch.rand(D, generator=g)) < D // 2, 1.0, -1.0).to(F32)


def exact_gemm(a, b):
    """a @ b^T in fp32, asserted exact: integers (or half-integers, hence the factor 2) whose absolute products sum below
    2^24 over the whole reduction; max|a| sum|b| is tried first: it is no smaller than |a| @ |b|^T"""
    worst = float((a.abs().amax(1, keepdim=True) * b.abs().sum(1)[None, :]).max())
    if 2 * worst >= 2.0 ** 24:
        worst = float((a.abs() @ b.abs().T).max())
    assert 2 * worst < 2.0 ** 24, "a partial sum could reach 2^24"
    assert bool((2 * a == (2 * a).round()).all()) and bool((b == b.round()).all())
    return a @ b.T


def assert_bf16_exact(t, what, limit=256.0):
    assert float(t.abs().max()) <= limit and torch.equal(t.to(BF).to(F32), t), f"{what}: not exact as bf16 (max {float(t.abs().max())})"


def special_rows(M):
    """(zero-variance rows, rows with a common offset) of the linln_panel, linear_ln and ffn_infer tables"""
    if M < 8:
        return [], []
    return [1, M - 2], [2, M - 1]


@functools.lru_cache(maxsize=3)
def make_inputs(c):
    """the rows of a case (fp32 tensors holding exact bf16 values); the parameters are weights(...)"""
    M = c.M
    if c.fam in ("linln_panel", "linear_ln"):
        g = _gen(f"rows/{c.fam}/{M}/{c.N}/{c.K}")
        W = weights(c.fam, c.N, c.K)
        x, res = _ints(g, (M, c.K), 2), _ints(g, (M, c.N), 3)
        zv, off = special_rows(M)
        if c.res:
            res[off] += 200.0
            x[zv] = 0.0
            res[zv] = 7.0 - (W["bias"] if c.bias else 0.0)
        elif not c.bias:
            x[zv] = 0.0
        return {"x": x, "res": res if c.res else None}
    if c.fam == "linear_panel":
        return {"x": _ints(_gen(f"rows/linear_panel/{M}"), (M, D), 2)}
    if c.fam == "ffn_infer":
        W = weights("ffn_infer", ffn=c.ffn)
        x1 = _ints(_gen(f"rows/ffn_infer/{M}"), (M, D), 2)
        zv, off = special_rows(M)
        x1[zv] = 0.0
        for r in off:
            x1[r, W["jcols"]] = 2.0 * W["jpat"]
        return {"x1": x1}
    g = _gen(f"rows/chain/{M}")
    W = weights("chain", ffn=c.ffn)
    attn = _ints(g, (M, D), 2)
    attn[attn == 0] = 1.0                                             # nonzero, as Wo and bo: every addend of s1 is live
    sigma = torch.where(torch.argsort(torch.rand(M, D, generator=g), 1) < D // 2, 1.0, -1.0).to(F32)
    sigma[CHAIN_OFFSET_EVERY - 1::CHAIN_OFFSET_EVERY] = chain_sigma_star()
    zv = torch.zeros(M, dtype=torch.bool)
    zv[3::CHAIN_ZV_EVERY] = True
    sigma[zv] = 1.0                                                   # s1 = c on the whole row: zero variance in LN1
    cvals = torch.tensor([0.5, 1.0, 2.0, 4.0])[torch.arange(M) % 4][:, None]
    x = sigma * cvals - (exact_gemm(attn, W["wo"]) + W["bo"])
    assert_bf16_exact(x, "chain x", 128.0)
    return {"x": x, "attn": attn, "sigma": sigma, "c": cvals, "zv": zv}


# ---- references ------------------------------------------------------------------------------------------------------------
def relu(t):
    return t.clamp_min(0)


@functools.lru_cache(maxsize=3)
def _reference(fam, M, N, K, ffn, bias, res):
    c = next(k for k in CASES if (k.fam, k.M, k.N, k.K, k.ffn, k.bias, k.res) == (fam, M, N, K, ffn, bias, res))
    inp = make_inputs(c)
    if fam in ("linln_panel", "linear_ln"):
        W = weights(fam, N, K)
        a = exact_gemm(inp["x"], W["w"]) + (W["bias"] if bias else 0.0)
        if fam == "linear_ln":
            assert_bf16_exact(a, "a_out")
        return {"a": a, "v": a + inp["res"] if res else a}
    if fam == "linear_panel":
        W = weights(fam, N, K)
        y = exact_gemm(inp["x"], W["w"])
        assert_bf16_exact(y + W["bias"], "y")
        assert_bf16_exact(y, "y without bias")
        return {"y_nobias": y, "y_bias": y + W["bias"]}
    W = weights(fam, ffn=ffn)
    if fam == "chain":
        s1 = inp["x"] + (exact_gemm(inp["attn"], W["wo"]) + W["bo"])
        zv = inp["zv"]
        assert torch.equal(s1, inp["sigma"] * inp["c"]) and bool(((s1 > 0).sum(1) == torch.where(zv, D, D // 2)).all())
        x1 = torch.where(zv[:, None], W["beta1"].expand(M, -1), s1.sign() * W["gamma1"] + W["beta1"])
        assert bool((x1[~zv] % 2 == 1).all())                         # odd: never a cancellation to a tiny nonzero
    else:
        s1, x1 = None, inp["x1"]
    h = relu(exact_gemm(x1, W["w1"]) + W["b1"])
    assert_bf16_exact(h, "h")
    f2 = exact_gemm(h, W["w2"])
    v = x1 + (f2 + W["b2"])
    out = {"x1": x1, "h": h, "v": v, "s1": s1}
    if fam == "chain":
        assert_bf16_exact(s1, "s1", 4.0)
        assert_bf16_exact(x1, "x1")
        assert_bf16_exact(v, "s2")
        off = torch.zeros(M, dtype=torch.bool)
        off[CHAIN_OFFSET_EVERY - 1::CHAIN_OFFSET_EVERY] = True
        off &= ~zv
        assert not off.any() or float(v[off].mean(1).min()) > 64.0, "the offset rows carry no offset"
        assert bool((v[zv] == CHAIN_ZV_H + 7.0).all()), "the zero-variance rows of s2 are not constant"
    else:
        zv, off = special_rows(M)
        assert bool((v[zv] == 7.0).all()) and (not off or float(v[off].mean(1).min()) > 64.0)
    return out


def reference(c):
    """the exact intermediate and output values of a case (fp32, CPU)"""
    return _reference(c.fam, c.M, c.N, c.K, c.ffn, c.bias, c.res)


def slab_reference(c, ref, W):
    """ffn_infer: [nc SUB, M, 512] fp32, slab c SUB + sb = h[:, chunk c, sub-chunk sb] @ W2[:, the same columns]^T"""
    _, _, nc, sb = ffn_coop_geometry(c.M, D, c.ffn)
    hc = FF_CHUNK // sb
    return torch.stack([exact_gemm(ref["h"][:, j * hc:(j + 1) * hc], W["w2"][:, j * hc:(j + 1) * hc]) for j in range(nc * sb)])


def ln_reference(v, gamma, beta, n, form):
    """(float64 {y, mean, rstd}, the module docstring's bound for each) of LayerNorm rows v (exact); any device"""
    v, g, bt = v.to(F64), gamma.to(v.device).to(F64), beta.to(v.device).to(F64)
    N, u = v.shape[1], U32
    mean = v.sum(1, keepdim=True) / N
    d = v - mean
    var = (d * d).sum(1, keepdim=True) / N
    rstd = 1 / torch.sqrt(var + EPS)
    y = d * rstd * g + bt
    w = (n + 2) * u * v.abs().sum(1, keepdim=True) / N
    if form == "two_pass":
        e_var = ((2 * d.abs() * w + w * w + 3 * u * d * d).sum(1, keepdim=True) + n * u * (d * d).sum(1, keepdim=True)) / N + 2 * u * var
    else:
        e_var = (n + 3) * u * (v * v).sum(1, keepdim=True) / N + 2 * mean.abs() * w + w * w + u * mean * mean + u * var
    hi, lo = 1 / torch.sqrt((var - e_var).clamp_min(0) + EPS), 1 / torch.sqrt(var + e_var + EPS)
    e_rstd = torch.maximum(hi - rstd, rstd - lo) + 3 * u * hi
    e_y = g.abs() * (d.abs() * e_rstd + w * (rstd + e_rstd) + 3 * u * d.abs() * rstd) + (u + UB16) * y.abs()
    e_y = torch.where((g == 0).expand_as(e_y), torch.zeros_like(e_y), e_y)
    return ({"y": y, "mean": mean[:, 0], "rstd": rstd[:, 0]}, {"y": S * e_y, "mean": S * w[:, 0], "rstd": S * e_rstd[:, 0]})


def qkv_reference(y, W):
    """(float64 reference of the QKV tail from the kernel's own y, its bound); on y's device"""
    y64, w64 = y.to(F64), W["wqkv"].to(y.device).to(F64)
    ref = y64 @ w64.T + W["bqkv"].to(y.device).to(F64)
    return ref, S * (D * U32 * (y64.abs() @ w64.abs().T) + UB16 * ref.abs())


# ---- the checks: the same function for the GPU's outputs and for the CPU emulation's -------------------------------------
def _exact(msgs, what, got, want):
    got, want = got.detach().cpu(), want
    if got.dtype != F32:
        got = got.to(F32)
    nan = torch.isnan(got)
    bad = (got != want) | nan
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        msgs.append(f"{what}: {int(bad.sum())} of {bad.numel()} elements are not the exact value, first at {i}: got "
                    f"{got[i].item()!r}, exact {want[i].item()!r}")


def check(c, got, device="cpu"):
    """got: the outputs of a case (see the family's keys below).  -> (failure messages, the largest error / bound)
    linln_panel {y};  linear_panel {y};  ffn_infer {slabs [nc SUB, M, 512], y};  chain {y, qkv (tail)};
    linear_ln {slab_sum, nslab, y, a_out, mean, rstd (saved)}"""
    ref = reference(c)
    msgs, worst = [], 0.0
    W = weights(c.fam, c.N, c.K, c.ffn)
    if c.fam == "linear_panel":
        _exact(msgs, f"{c.name} y", got["y"], ref["y_bias" if c.bias else "y_nobias"])
        return msgs, 0.0
    if c.fam == "ffn_infer":
        _exact(msgs, f"{c.name} slabs", got["slabs"], slab_reference(c, ref, W))
    if c.fam == "linear_ln":
        _exact(msgs, f"{c.name} sum of the slabs", got["slab_sum"], ref["a"] - (W["bias"] if c.bias else 0.0))
        used = linear_ln_plan(c.M, c.N, c.K)[1]
        if got["nslab"] != used:
            msgs.append(f"{c.name}: {got['nslab']} slabs written, {used} expected")
        if c.saved:
            _exact(msgs, f"{c.name} a_out", got["a_out"], ref["a"])
    n, form = ln_adds(c)
    lref, lbnd = ({k: t.cpu() for k, t in d.items()} for d in ln_reference(ref["v"].to(device), W["gamma"], W["beta"], n, form))
    keys = ("y", "mean", "rstd") if c.fam == "linear_ln" and c.saved else ("y",)
    for k in keys:
        msg, r = violations(f"{c.name} {k}", got[k], lref[k], lbnd[k])
        worst = max(worst, r)
        if msg:
            msgs.append(msg)
    zero_g = W["gamma"] == 0
    yz = got["y"].detach().cpu().to(F32)[:, zero_g]
    if not torch.equal(yz, W["beta"][zero_g].expand(c.M, -1)):
        msgs.append(f"{c.name}: gamma = 0 columns must give exactly beta")
    const = (ref["v"] == ref["v"][:, :1]).all(1)                      # exact integer sums: mean = v, d = 0, y = 0 rstd gamma + beta
    if const.any() and not torch.equal(got["y"].detach().cpu().to(F32)[const], W["beta"].expand(int(const.sum()), -1)):
        msgs.append(f"{c.name}: the zero-variance rows must give exactly beta")
    if c.fam == "chain" and c.tail:
        qref, qbnd = (t.cpu() for t in qkv_reference(got["y"].to(device), W))
        msg, r = violations(f"{c.name} qkv", got["qkv"], qref, qbnd)
        worst = max(worst, r)
        if msg:
            msgs.append(msg)
    return msgs, worst
