"""Shared by tests/test_chain_edges_gpu.py and tests/test_chain_bounds_cpu.py: the case table of the fused MLP-denoiser chain
kernel (csrc/chain.hip: ib_mlp_chain_train, ib_mlp_chain_pack), its launch geometry restated in Python, the seeded inputs, the
stage-held float64 references, the ELEMENTWISE bound every output is held to, and check() -- the GPU's outputs and the CPU
emulation's go through the same function.  Conventions of tests/batchnorm_cases.py / tests/frozen_cases.py: u = U32 = 2^-24
per fp32 operation on the magnitude of the partial sums it acts on, UB16 = 2^-8 on a value stored as bf16, one untuned safety
factor S = 2 on the whole bound, every bound in absolute form (a cancellation is covered by the sum of the absolute terms), a
bound of exactly 0 admits only the exact value.  A hardware transcendental (v_exp_f32, v_rcp_f32, v_rsq_f32) is 1 ulp = 2 u.

Geometry (restated from chain_shape, ib_mlp_chain_workgroups, chain_layout, ib_mlp_chain_partial_width and the kernel head):
  chain_shape(D, H) -> (nth, ntd, kbd): H = 128 nth; D <= 128 ntd, D <= 32 kbd, the smallest instantiated pair; None: refused
  workgroups(M) -> (workgroups, P): P = ceil(M / 256) clamped to 16 .. 64, P = M below 16 rows
  packed image: forward blocks 0 .. L-1, head, transposed blocks 1 .. L-1, head^T; block (nt, kb) of a matrix with NTOT
      n-tiles is 512 elements at ((kb NTOT + nt) 64 + lane) 8: W_eff[16 nt + lane % 16][32 kb + 8 (lane / 16) + 0 .. 7], zero
      beyond the matrix (expected_pack)
  partial row of a workgroup: per block dgamma | dbeta | dbias (3 H), then 128 ntd head-bias sums, then the squared-error sum
      at 3 L H + 128 ntd; width = that + 4 (the three floats behind the sum are never written and never read)
  panel j: r0 = j P, nrows = min(P, M - r0), w0 = r0 / T, nwin = (r0 + nrows - 1) / T - w0 + 1; the e rows of its tokens come
      from registers (nwin == 1, "one"), from the LDS image (2 .. 8, "staged") or from HBM (> 8, "unstaged")

Inputs (make_inputs; seeded in float64, cast to the stored type: after the cast they are the exact operands): x0, eps ~ N(0, 1);
W ~ N(0, 1 / K), so the GEMM term is ~ 1; e rows ~ N(0, 1), distinct per window and per block; biases ~ 0.5 N(0, 1) ROUNDED TO
bf16; gamma = 1 + 0.3 N(0, 1) and beta = 0.5 N(0, 1) per column; a schedule table of 10 rows; t holds 0, 9, -3 and 13 (B >= 4;
one out-of-range value at B == 1).  The zero rows: one whole window (B >= 2; else the last row, M >= 2) has x0 = eps = 0 and
e[w, block 0] = -bias[0], so x_t = 0, the GEMM gives 0 and u_0 = (0 + bias) + (-bias) = 0 EXACTLY; SiLU(0) = 0, the block-0
LayerNorm meets a zero-variance row and h_0 must be bf16(beta_0) bit for bit (an omitted eps gives NaN).  check() asserts both.

References are STAGE-HELD (every case passes u buffers): each stage in float64 from the kernel's OWN previous stage as stored
in HBM, so a flipped bf16 rounding upstream is not amplified downstream:
  x_t      x0, eps, the clamped t, the tables                      u_i   kernel's h_{i-1} (x_t), W_i, bias_i, e row of the window
  h_i      kernel's u_i: exact SiLU, LayerNorm                      dpred kernel's h_{L-1}: (bf16(pred) - eps) 2 / (M D)
  loss     the same pred, over the panel's rows, columns < D       dz_i  kernel's dz_{i+1} (dpred) W, kernel's u_i (statistics
  dbias_i, head-bias rows   column sums over the panel of the            recomputed in float64 from it)
           kernel's own dz_i / dpred as stored                     dgamma_i, dbeta_i   the reference dh and xh of that panel
  de_lp    bf16 of the kernel's dbias partial row, bit for bit

The bounds, as counted from csrc/chain.hip (all times S):
  x_t    c.x x + c.y e: two products, one sum (or one fma): 3 u (|c.x x| + |c.y e|) + UB16 |x_t|
  u_i    chain_gemm adds K products into the accumulator (K = 32 kbd for block 0 -- the zero padding adds exact zeros, kept --
         else H), then bias, then e:  (K + 2) u (|in| @ |W|^T + |bias| + |e|) + UB16 |u|
  SiLU   fast_sigmoid(x) = rcp(1 + __expf(-x)); __expf scales the argument by log2 e (the constant and the product round:
         2 u |x| log2 e in the argument = 2 u |x| relative in the result) and v_exp_f32 is 1 ulp: rel_exp = (2 |x| + 2) u;
         the sum 1 + E rounds (u), rcp is 1 ulp (2 u):  e_sg = sg ((1 - sg) rel_exp + 3 u),  v = x sg: e_v = |x| e_sg + u |v|
  row sums (fwd_layer): per lane a0 = ((v0 + v2) + v4) + v6, a1 likewise, a0 + a1: 4 additions; group_sum<LPR>: log2 LPR DPP
         levels (row16_sum 4, row_bcast15, row_bcast31): n = 4 + log2(H / 8); the squares round once more
         e_mean = (n + 2) u sum|v| / H + sum e_v / H                     (the input term: v is no longer exact)
         one-pass variance E[v^2] - mean^2 clamped at 0, as in tests/frozen_cases.py plus the input term:
         e_var = (n + 3) u sum v^2 / H + 2 |mean| e_mean + e_mean^2 + u mean^2 + u var + sum (2 |v| e_v + e_v^2) / H
  rstd   NOT first order (a zero-variance row has var ~ e_var ~ 0 against eps): the computed variance lies in
         [max(var - e_var, 0), var + e_var]: e_rstd = max(hi - rstd, rstd - lo) + 3 u hi   (the sum with eps, rsq 1 ulp)
  h_i    (v - mean) rstd gamma + beta:  |gamma| (|d| e_rstd + (e_mean + e_v) (rstd + e_rstd) + 3 u |d| rstd) + (u + UB16) |h|
  dpred  pred = acc + bias in fp32 (H products and the bias: e_p = (H + 1) u (|h| @ |W|^T + |bias|)), rounded to bf16, then
         d = pr - eps, d gscale rounded to bf16 again.  The double rounding: the kernel rounds its own fp32 pred, the
         reference rounds the float64 one; the two bf16 values differ by at most e_p plus half an ulp on either side, and
         half an ulp is up to UB16 |pred|:  e_d = e_p + 2 UB16 |pred|.  gscale = 2.f / ((float) M (float) D): a product and a division, 2 u; the subtraction and
         the product with gscale another 2 u:   gscale e_d + 4 u |dpred| + UB16 |dpred|
  loss   per lane 16 ntd terms in sequence, group_sum<64> 6 levels, 8 waves in sequence: n_l = 16 ntd + 14;
         sum (2 |d| e_d + e_d^2) + (n_l + 1) u sum d^2
  head-bias sums   per lane 4 m-tiles, row16_sum 4 levels: 8 u sum|dpred| over the panel; the columns D .. 128 ntd - 1 are 0
  dz_i   dh = g @ W over K = H (32 kbd for the head^T GEMM): e_dh = K u (|g| @ |W|); the kernel's own mean / rstd (kept in
         LDS, not stored) carry e_mean / e_rstd of the forward; xh = (v - mean) rstd:
         e_xh = (e_v + e_mean) (rstd + e_rstd) + |d| e_rstd + 2 u |xh|;  silu' = sg (1 + x (1 - sg)): e_ds as e_f of
         tests/batchnorm_cases.py with e_sg from above;  dxh = dh gamma: e_dxh = |gamma| e_dh + u |dxh|;
         sa, sb: 8 terms per lane in sequence, then the tree: n_b = 8 + log2(H / 8):
         e_ma = ((n_b + 1) u sum|dxh| + sum e_dxh) / H,  e_mb = ((n_b + 2) u sum|dxh xh| + sum (|xh| e_dxh + |dxh| e_xh)) / H
         the three terms on their absolute values, A = |dxh| + |ma| + |xh mb|:
         e_in = e_dxh + e_ma + |xh| e_mb + |mb| e_xh + u |xh mb| + 2 u A
         dz = rstd (dxh - ma - xh mb) silu':  |silu'| (rstd e_in + e_rstd A) + rstd A e_ds + 2 u rstd A |silu'| + UB16 |dz|
  column sums of a block (dgamma | dbeta | dbias): per lane over its NJ = H / 64 rows in sequence, log2(512 / H) shuffles
         across the row groups of a wave, 8 waves in sequence: n_c = H / 64 + log2(512 / H) + 8
         dbias  n_c u sum|dz| (of the stored dz);  dbeta  sum e_dh + n_c u sum|dh|;
         dgamma sum (|xh| e_dh + |dh| e_xh) + (n_c + 1) u sum|dh xh|
No figure here is tuned to a GPU result, and no element is excluded from any comparison.

What must not be written: every output lives in a buffer filled with the sentinel SENT, GR guard rows before and after and
guard columns where the pitch allows; check() requires the sentinel everywhere outside rows < M, outside columns < D of x_t,
outside columns < D of dpred (< D rounded up to 8 in the 16-byte store form, whose pad columns must hold zeros) and outside
the partial width.

The cases (name: B x T, D, H, L -> instantiation <nth, ntd, kbd, KEEP>; M, P; what it is there for):
  h512_d4_m1       1x1    D=4   H=512 L=1 <4,1,2,keep>   M=1 (P=M=1); D=4; pitch D with D % 8 == 4 (8-byte dpred); panel == window (de_lp)
  h512_d64_m15     1x15   D=64  L=3 <4,1,2,->            M=15 (P=M); D edge 64; panel == window (de_lp); KEEP off
  h512_d68_m16     8x2    D=68  L=2 <4,1,4,keep>         M=16; D edge 68; staged, exactly 8 windows; pitch rounded up to 8 (zero pad columns)
  h512_d128_m17    17x1   D=128 L=4 <4,1,4,->            M=17 (last panel 1 row); D edge 128; unstaged 16 windows; L=4 at H=512
  h512_d132_m39    3x13   D=132 L=1 <4,2,8,keep>         D edge 132; staged 2 windows, boundary off the m-tile; dpred base offset 8 bytes
  h512_d256_m48    3x16   D=256 L=3 <4,2,8,->            D edge 256; panel == window at P=16 (de_lp); ld_part wider than the width
  h512_d260_m40    2x20   D=260 L=2 <4,3,10,keep>        D edge 260; pitch D % 8 == 4; window longer than the panel and staged 2
  h512_d320_m33    11x3   D=320 L=4 <4,3,10,->           D edge 320; staged 6 windows; last panel 1 row; L=4
  h512_d324_m20    4x5    D=324 L=1 <4,3,12,keep>        D edge 324; in_slots (the direct arguments hold other data); all four t edges
  h512_d384_m32    2x16   D=384 L=3 <4,3,12,->           D edge 384; ld_e > L H; de_lp
  h512_d388_m18    18x1   D=388 L=2 <4,4,16,keep>        D edge 388; unstaged 16 and staged 2 in one launch; last panel 2 rows
  h512_d512_m50    1x50   D=512 L=4 <4,4,16,->           D edge 512 (DP and DN filled exactly); window much longer than the panel
  h512_p64_full    256x64 D=300 L=2 <4,3,10,keep>        M=16384: P=64, 256 full panels, panel == window at P=64 (de_lp); the one large H=512 case
  h256_d320_m17    17x1   D=320 H=256 L=2 <2,3,10,keep>  D edge 320 at H=256; last panel 1 row; unstaged 16
  h256_d4_m18      9x2    D=4   L=3 <2,3,10,->           last panel 2 rows (one row group of a wave-instruction exactly); staged 8 and nwin 1
  h256_m19         1x19   D=300 L=1                      last panel 3 rows (just past a row group)
  h256_m21         3x7    D=100 L=4 <2,3,10,->           last panel 5 rows; staged 3 windows (panel 0: rows 0 .. 15 of windows 0 .. 2)
  h256_m4114       242x17 D=36  L=1                      P=17, every panel 17 rows (last too): panel == window (de_lp)
  h256_m8217       747x11 D=300 L=2                      P=33 (crosses the 32-row half), last panel 33 rows; staged 3 (a panel is three windows)
  h128_d64_m17     1x17   D=64  H=128 L=1 <1,1,2,keep>   D edge 64 at H=128; last panel 1 row; window longer than the panel
  h128_d68_m18     2x9    D=68  L=2 <1,1,4,keep>         D edge 68; last panel 2 rows; staged 2
  h128_d128_m19    19x1   D=128 L=3 <1,1,4,->            D edge 128 at H=128; last panel 3 rows; unstaged 16 and staged 3 in one launch
  h128_d4_m21      7x3    D=4   L=4 <1,1,2,->            last panel 5 rows; L=4 at H=128; staged 6
  h128_m4114       2057x2 D=64  L=2                      P=17, last panel 17 rows; unstaged 9 windows
  h128_m8217       913x9  D=128 L=3                      P=33, last panel 33 rows; staged 4 .. 5
  h128_m4096       1x4096 D=64  L=1                      M=4096: 256 full panels of 16; one window much longer than the panel
  h128_m4100       1025x4 D=40  L=2                      P=17 with a ragged last panel (3 rows); staged 5
  h128_m8208       513x16 D=36  L=2                      P=33, T=16: staged 3 (last panel 2); the boundaries of panel 0 fall on m-tile rows 16 and 32, the others' do not
  h128_mix         1878x3 D=20  L=1                      M=5634, P=23, T=3: panels of 8 (staged) and 9 (unstaged) windows in one launch.
                                                         (P=64 with T=9 always spans exactly 8 windows, so it cannot mix; P=23 is the smallest P that can)
  h128_p64_last1   16129x1 D=4  L=1 <1,1,2,keep>         M=16129: P=64, last panel 1 row; unstaged 64 windows
  h128_p64_t8      2048x8 D=60  L=1 <1,1,2,keep>         M=16384: P=64, last panel full; staged exactly 8 at P=64
Refusals (REFUSED): D=132 at H=128, D=324 at H=256, D=516 at H=512, D=6, H=64, H=1024, L=0, L=5."""
import math
import zlib
from collections import namedtuple

import torch

from tests.batchnorm_cases import S, U32, UB16, violations  # noqa: F401  (violations is re-exported)

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
IB_OK, IB_E_ARG, IB_E_UNSUPPORTED = 0, -1, -5
PATH_CHAIN2 = 10
LN_EPS = float(torch.tensor(1e-5, dtype=torch.float32))
CH_ROWS, CH_WAVES, CH_MAXL, CH_NWIN = 64, 8, 4, 8
SENT = 1536.0                      # exact in bf16 and fp32
GR = 2                             # guard rows before and after every output
TABLE_ROWS = 10


def cdiv(a, b):
    return -(-a // b)


def up8(n):
    return cdiv(n, 8) * 8


# ---- geometry, restated from the C code ------------------------------------------------------------------------------------
GEO = ((1, 2), (1, 4), (2, 8), (3, 10), (3, 12), (4, 16))


def chain_shape(D, H):
    """chain_shape -> (nth, ntd, kbd), or None: refused"""
    if H not in (128, 256, 512) or D <= 0 or D % 4 or D > 512:
        return None
    kb_need, nt_need = cdiv(D, 32), cdiv(cdiv(D, 16), 8)
    for j, (nt, kb) in enumerate(GEO):
        if nt < nt_need or kb < kb_need:
            continue
        if H == 512 or (H == 256 and j == 3) or (H == 128 and j < 2):
            return H // 128, nt, kb
    return None


def supported(D, H, L):
    return 1 <= L <= CH_MAXL and chain_shape(D, H) is not None


def workgroups(M):
    """ib_mlp_chain_workgroups -> (workgroups, P)"""
    P = min(cdiv(M, 256), CH_ROWS)
    if P < 16:
        P = M if M < 16 else 16
    return cdiv(M, P), P


def packed_layout(D, H, L):
    """chain_layout -> ([(what, index, transposed, N, K, n_tiles, KB, offset)], total elements); () and 0: refused"""
    if not supported(D, H, L):
        return (), 0
    _, ntd, kbd = chain_shape(D, H)
    kbh, nth8, ntd8 = H // 32, H // 16, 8 * ntd
    out, off = [], 0
    for i in range(L):
        kb = kbd if i == 0 else kbh
        out.append(("fwd", i, False, H, D if i == 0 else H, nth8, kb, off))
        off += nth8 * kb * 512
    out.append(("fwd", L, False, D, H, ntd8, kbh, off))
    off += ntd8 * kbh * 512
    for i in range(1, L):
        out.append(("bwd", i, True, H, H, nth8, kbh, off))
        off += nth8 * kbh * 512
    out.append(("bwd", L, True, H, D, nth8, kbd, off))
    off += nth8 * kbd * 512
    return out, off


def packed_elems(D, H, L):
    return packed_layout(D, H, L)[1]


def partial_width(D, H, L):
    return 3 * L * H + 128 * chain_shape(D, H)[1] + 4 if supported(D, H, L) else 0


def partial_columns(D, H, L):
    """-> {dgamma / dbeta / dbias: [first column per block], head: first column, head_end, loss: column}"""
    ntd = chain_shape(D, H)[1]
    return {"dgamma": [3 * i * H for i in range(L)], "dbeta": [3 * i * H + H for i in range(L)],
            "dbias": [3 * i * H + 2 * H for i in range(L)], "head": 3 * L * H, "head_end": 3 * L * H + 128 * ntd,
            "loss": 3 * L * H + 128 * ntd}


def expected_pack(W, D, H, L):
    """the image ib_mlp_chain_pack must write, from the row-major bf16 weights (blocks 0 .. L-1, then the head)"""
    lay, total = packed_layout(D, H, L)
    img = torch.zeros(total, dtype=BF)
    for _, i, tr, N, K, n_tiles, KB, off in lay:
        w = W[i].t() if tr else W[i]                                  # W_eff [N, K]
        assert tuple(w.shape) == (N, K)
        pad = torch.zeros(16 * n_tiles, 32 * KB, dtype=BF)
        pad[:N, :K] = w
        # [nt, lane % 16, kb, lane / 16, 8] -> [kb, nt, lane / 16, lane % 16, 8]
        blk = pad.view(n_tiles, 16, KB, 4, 8).permute(2, 0, 3, 1, 4).reshape(-1)
        img[off:off + blk.numel()] = blk
    return img


def panel_info(M, T, j):
    """panel j -> (r0, nrows, w0, nwin, e path)"""
    _, P = workgroups(M)
    r0 = j * P
    nrows = min(P, M - r0)
    w0 = r0 // T
    nwin = (r0 + nrows - 1) // T - w0 + 1
    return r0, nrows, w0, nwin, ("one" if nwin == 1 else "staged" if nwin <= CH_NWIN else "unstaged")


# ---- the case table ----------------------------------------------------------------------------------------------------------
# xt / dp: the row pitch of x_t / dpred: "D" (pitch D), "up8" (rounded up to 8, plus 8 guard columns), dp "off8": the same with
# the base 8 bytes in (16-byte store form off).  geom = (nth, ntd, kbd, KEEP), P, last = rows of the last panel, paths = the e
# paths the launch takes, nwins = the window counts the case is there for: all checked against the restated geometry.
Case = namedtuple("Case", "name B T D H L xt dp ld_e_extra ld_part_extra de_lp slots geom P last paths nwins")


def _c(name, B, T, D, H, L, geom, P, last, paths, nwins, xt="up8", dp="up8", lde=0, ldp=0, de_lp=False, slots=False):
    return Case(name, B, T, D, H, L, xt, dp, lde, ldp, de_lp, slots, geom, P, last, frozenset(paths.split()), frozenset(nwins))


CASES = [
    _c("h512_d4_m1", 1, 1, 4, 512, 1, (4, 1, 2, True), 1, 1, "one", {1}, xt="D", dp="D", de_lp=True),
    _c("h512_d64_m15", 1, 15, 64, 512, 3, (4, 1, 2, False), 15, 15, "one", {1}, de_lp=True),
    _c("h512_d68_m16", 8, 2, 68, 512, 2, (4, 1, 4, True), 16, 16, "staged", {8}),
    _c("h512_d128_m17", 17, 1, 128, 512, 4, (4, 1, 4, False), 16, 1, "one unstaged", {16, 1}, dp="D"),
    _c("h512_d132_m39", 3, 13, 132, 512, 1, (4, 2, 8, True), 16, 7, "one staged", {2}, dp="off8"),
    _c("h512_d256_m48", 3, 16, 256, 512, 3, (4, 2, 8, False), 16, 16, "one", {1}, ldp=12, de_lp=True),
    _c("h512_d260_m40", 2, 20, 260, 512, 2, (4, 3, 10, True), 16, 8, "one staged", {1, 2}, xt="D", dp="D"),
    _c("h512_d320_m33", 11, 3, 320, 512, 4, (4, 3, 10, False), 16, 1, "one staged", {6}),
    _c("h512_d324_m20", 4, 5, 324, 512, 1, (4, 3, 12, True), 16, 4, "one staged", {4}, slots=True),
    _c("h512_d384_m32", 2, 16, 384, 512, 3, (4, 3, 12, False), 16, 16, "one", {1}, lde=16, de_lp=True),
    _c("h512_d388_m18", 18, 1, 388, 512, 2, (4, 4, 16, True), 16, 2, "staged unstaged", {16, 2}, dp="off8"),
    _c("h512_d512_m50", 1, 50, 512, 512, 4, (4, 4, 16, False), 16, 2, "one", {1}, xt="D", dp="D"),
    _c("h512_p64_full", 256, 64, 300, 512, 2, (4, 3, 10, True), 64, 64, "one", {1}, de_lp=True),
    _c("h256_d320_m17", 17, 1, 320, 256, 2, (2, 3, 10, True), 16, 1, "one unstaged", {16}),
    _c("h256_d4_m18", 9, 2, 4, 256, 3, (2, 3, 10, False), 16, 2, "one staged", {8, 1}, xt="D", dp="D"),
    _c("h256_m19", 1, 19, 300, 256, 1, (2, 3, 10, True), 16, 3, "one", {1}, xt="D"),
    _c("h256_m21", 3, 7, 100, 256, 4, (2, 3, 10, False), 16, 5, "one staged", {3}, dp="off8"),
    _c("h256_m4114", 242, 17, 36, 256, 1, (2, 3, 10, True), 17, 17, "one", {1}, de_lp=True),
    _c("h256_m8217", 747, 11, 300, 256, 2, (2, 3, 10, True), 33, 33, "staged", {3}),
    _c("h128_d64_m17", 1, 17, 64, 128, 1, (1, 1, 2, True), 16, 1, "one", {1}),
    _c("h128_d68_m18", 2, 9, 68, 128, 2, (1, 1, 4, True), 16, 2, "one staged", {2}),
    _c("h128_d128_m19", 19, 1, 128, 128, 3, (1, 1, 4, False), 16, 3, "staged unstaged", {16, 3}),
    _c("h128_d4_m21", 7, 3, 4, 128, 4, (1, 1, 2, False), 16, 5, "staged", {6, 2}, xt="D", dp="D"),
    _c("h128_m4114", 2057, 2, 64, 128, 2, (1, 1, 2, True), 17, 17, "unstaged", {9}, lde=8),
    _c("h128_m8217", 913, 9, 128, 128, 3, (1, 1, 4, False), 33, 33, "staged", {4, 5}),
    _c("h128_m4096", 1, 4096, 64, 128, 1, (1, 1, 2, True), 16, 16, "one", {1}),
    _c("h128_m4100", 1025, 4, 40, 128, 2, (1, 1, 2, True), 17, 3, "one staged", {5}, ldp=4),
    _c("h128_m8208", 513, 16, 36, 128, 2, (1, 1, 2, True), 33, 24, "staged", {3, 2}, xt="D", dp="D"),
    _c("h128_mix", 1878, 3, 20, 128, 1, (1, 1, 2, True), 23, 22, "staged unstaged", {8, 9}, xt="D", dp="D"),
    _c("h128_p64_last1", 16129, 1, 4, 128, 1, (1, 1, 2, True), 64, 1, "one unstaged", {64}, xt="D", dp="D"),
    _c("h128_p64_t8", 2048, 8, 60, 128, 1, (1, 1, 2, True), 64, 64, "staged", {8}, dp="off8"),
]
BY_NAME = {c.name: c for c in CASES}
LARGE = ("h512_p64_full", "h128_p64_last1", "h128_p64_t8")          # the P = 64 cases
REFUSED = [(132, 128, 1), (324, 256, 2), (516, 512, 1), (6, 512, 1), (64, 64, 1), (64, 1024, 1), (64, 512, 0), (64, 512, 5)]


def case_id(c):
    return c.name


def geometry(c):
    """everything check(), the emulation and the launcher need of a case's launch"""
    M = c.B * c.T
    nth, ntd, kbd = chain_shape(c.D, c.H)
    nwg, P = workgroups(M)
    return namedtuple("Geom", "M nth ntd kbd nwg P width DN DP keep")(M, nth, ntd, kbd, nwg, P, partial_width(c.D, c.H, c.L),
                                                                       128 * ntd, 32 * kbd, c.L <= 2)


def panels_of(c):
    M = c.B * c.T
    return [panel_info(M, c.T, j) for j in range(workgroups(M)[0])]


def emulated_panels(c):
    """the panels the CPU emulation runs: all, but the first, one middle and the last of a P = 64 case"""
    nwg = workgroups(c.B * c.T)[0]
    return [0, nwg // 2, nwg - 1] if c.name in LARGE else None


def dp16_form(c):
    """the 16-byte dpred store: pitch % 8 == 0 and a 16-byte base (every buffer of layout() starts 16-byte aligned)"""
    _, c0, _, ld = layout(c)["dpred"]
    return ld % 8 == 0 and c0 % 8 == 0


def layout(c):
    """output name -> (rows, first column, columns, pitch): the data sit at rows GR .. GR + rows - 1 of a [rows + 2 GR, pitch]
    buffer whose first element is 16-byte aligned"""
    g = geometry(c)
    pitch = lambda mode: c.D if mode == "D" else up8(c.D) + 8
    lay = {"xt": (g.M, 0, c.D, pitch(c.xt)), "dpred": (g.M, 4 if c.dp == "off8" else 0, c.D, pitch(c.dp) + (8 if c.dp == "off8" else 0)),
           "partial": (g.nwg, 0, g.width, g.width + c.ld_part_extra)}
    for i in range(c.L):
        for n in ("u", "h", "dz"):
            lay[f"{n}{i}"] = (g.M, 0, c.H, c.H)
    if c.de_lp:
        lay["de_lp"] = (c.B, 0, c.L * c.H, c.L * c.H + 8)
    return lay


def alloc(c, device="cpu"):
    """the sentinel-filled output buffers, name -> [rows + 2 GR, pitch]"""
    out = {}
    for name, (rows, _, _, ld) in layout(c).items():
        out[name] = torch.full((rows + 2 * GR, ld), SENT, dtype=F32 if name == "partial" else BF, device=device)
    return out


def body(c, outs, name):
    rows, c0, n, _ = layout(c)[name]
    return outs[name][GR:GR + rows, c0:c0 + n]


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def zero_rows(c):
    """(the window whose e row cancels bias[0], the rows with x0 = eps = 0) -- (None, empty) at M == 1"""
    M = c.B * c.T
    if c.B >= 2:
        w = c.B // 2
        return w, torch.arange(w * c.T, (w + 1) * c.T)
    if M >= 2:
        return 0, torch.tensor([M - 1])
    return None, torch.zeros(0, dtype=torch.int64)


def make_inputs(c):
    """-> dict: x0, eps [B, T, D] bf16; t [B] int64; sab, s1m [TABLE_ROWS] fp32; e [B, L H + ld_e_extra] bf16 (the pad columns
    hold NaN); W: L + 1 bf16 matrices; bias: L + 1 fp32 (bf16 values); gamma, beta: L fp32; for a slots case also x0_decoy,
    eps_decoy, t_decoy: what the direct arguments hold while the kernel must read the slots"""
    g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    B, T, D, H, L = c.B, c.T, c.D, c.H, c.L
    x0, eps = rn(B, T, D), rn(B, T, D)
    dims = [D] + [H] * L
    W = [(rn(dims[i + 1], dims[i]) * dims[i] ** -0.5).to(BF) for i in range(L)] + [(rn(D, H) * H ** -0.5).to(BF)]
    bias = [(0.5 * rn(H)).to(BF).to(F32) for _ in range(L)] + [(0.5 * rn(D)).to(BF).to(F32)]
    gamma = [(1 + 0.3 * rn(H)).to(F32) for _ in range(L)]
    beta = [(0.5 * rn(H)).to(F32) for _ in range(L)]
    e = torch.full((B, L * H + c.ld_e_extra), float("nan"), dtype=F64)
    e[:, :L * H] = rn(B, L * H)
    t = torch.randint(0, TABLE_ROWS, (B,), generator=g)
    if B == 1:
        t[0] = TABLE_ROWS + 5 if T % 2 else -2
    else:
        t[0], t[B - 1] = 0, TABLE_ROWS - 1
    if B >= 4:
        t[1], t[2] = -3, TABLE_ROWS + 3
    w, zr = zero_rows(c)
    if w is not None:
        x0.view(-1, D)[zr] = 0
        eps.view(-1, D)[zr] = 0
        e[w, :H] = -bias[0].double()
    ab = torch.linspace(0.999, 0.01, TABLE_ROWS, dtype=F64)
    inp = {"x0": x0.to(BF), "eps": eps.to(BF), "t": t, "sab": ab.sqrt().to(F32), "s1m": (1 - ab).sqrt().to(F32), "e": e.to(BF),
           "W": W, "bias": bias, "gamma": gamma, "beta": beta}
    if c.slots:
        inp.update(x0_decoy=rn(B, T, D).to(BF), eps_decoy=rn(B, T, D).to(BF),
                   t_decoy=torch.randint(0, TABLE_ROWS, (B,), generator=g))
    return inp


def gscale32(M, D):
    """2.f / ((float) M * (float) D), as the launcher computes it"""
    return float(torch.tensor(2.0, dtype=F32) / (torch.tensor(float(M), dtype=F32) * torch.tensor(float(D), dtype=F32)))


# ---- the stage references and bounds -----------------------------------------------------------------------------------------
def silu_parts(x):
    """float64 x -> (sg, v = x sg, e_sg, e_v)"""
    sg = torch.sigmoid(x)
    e_sg = sg * ((1 - sg) * (2 * x.abs() + 2) * U32 + 3 * U32)
    v = x * sg
    return sg, v, e_sg, x.abs() * e_sg + U32 * v.abs()


def ln_stats(v, e_v, H):
    """-> (mean, rstd, e_mean, e_rstd), [rows, 1] each, of the one-pass LayerNorm statistics of fwd_layer"""
    n = 4 + int(math.log2(H // 8))
    mean = v.mean(-1, keepdim=True)
    var = ((v - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1 / torch.sqrt(var + LN_EPS)
    e_mean = ((n + 2) * U32 * v.abs().sum(-1, keepdim=True) + e_v.sum(-1, keepdim=True)) / H
    e_var = ((n + 3) * U32 * (v * v).sum(-1, keepdim=True) / H + 2 * mean.abs() * e_mean + e_mean ** 2 + U32 * mean ** 2
             + U32 * var + (2 * v.abs() * e_v + e_v ** 2).sum(-1, keepdim=True) / H)
    hi = 1 / torch.sqrt((var - e_var).clamp_min(0) + LN_EPS)
    lo = 1 / torch.sqrt(var + e_var + LN_EPS)
    return mean, rstd, e_mean, torch.maximum(hi - rstd, rstd - lo) + 3 * U32 * hi


def check(c, inp, outs, panels=None):
    """Every output of one launch against its stage-held reference and bound, and the sentinel everywhere the launch must not
    write.  outs: the buffers of alloc() after the launch (any device).  panels: the panels that were run (the emulation of a
    P = 64 case); everything belonging to another panel must still hold the sentinel.  Returns {stage: worst error / bound};
    raises AssertionError listing every violated stage."""
    g = geometry(c)
    M, D, H, L, T, P = g.M, c.D, c.H, c.L, c.T, g.P
    dev = outs["xt"].device
    pan = list(range(g.nwg)) if panels is None else sorted(set(panels))
    ridx = torch.cat([torch.arange(j * P, min((j + 1) * P, M)) for j in pan]).to(dev)
    pid = torch.cat([torch.full((min((j + 1) * P, M) - j * P,), k, dtype=torch.int64) for k, j in enumerate(pan)]).to(dev)
    pan_t = torch.tensor(pan, device=dev)
    lay = layout(c)
    msgs, worst = [], {}

    def hold(stage, what, got, ref, bound):
        msg, w = violations(f"{c.name} {what}", got, ref.cpu(), bound.cpu())
        worst[stage] = max(worst.get(stage, 0.0), w)
        if msg:
            msgs.append(msg)

    def exact(stage, what, got, want):
        worst.setdefault(stage, 0.0)
        if not torch.equal(got, want):
            bad = (got != want) | (got != got)
            msgs.append(f"{c.name} {what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact value")
            worst[stage] = math.inf

    def segsum(x):
        return torch.zeros(len(pan), x.shape[1], dtype=F64, device=dev).index_add_(0, pid, x)

    # ---- what must not be written
    dpw = up8(D) if dp16_form(c) else D
    for name, (rows, c0, n, ld) in lay.items():
        written = torch.zeros(outs[name].shape, dtype=torch.bool, device=dev)
        sel = pan_t if name in ("partial", "de_lp") else ridx
        ncols = dpw if name == "dpred" else n
        written[GR + sel, c0:c0 + ncols] = True
        worst.setdefault("untouched", 0.0)
        rest = outs[name][~written]
        if not bool((rest == SENT).all()):
            where = ((outs[name] != SENT) & ~written).nonzero()[0].tolist()
            msgs.append(f"{c.name} {name}: {int((rest != SENT).sum())} elements written outside the output, first at buffer "
                        f"row {where[0]} (data rows {GR} .. {GR + rows - 1}), column {where[1]} (data columns {c0} .. {c0 + ncols - 1})")
            worst["untouched"] = math.inf
    get = lambda name: body(c, outs, name)[ridx].double()
    d64 = lambda x: x.to(dev).double()

    # ---- q_sample
    x0, eps = d64(inp["x0"]).view(M, D)[ridx], d64(inp["eps"]).view(M, D)[ridx]
    win = ridx // T
    k = inp["t"].to(dev)[win].clamp(0, TABLE_ROWS - 1)
    cx, cy = d64(inp["sab"])[k][:, None], d64(inp["s1m"])[k][:, None]
    ref = cx * x0 + cy * eps
    xt = get("xt")
    hold("xt", "x_t", xt, ref, S * (3 * U32 * ((cx * x0).abs() + (cy * eps).abs()) + UB16 * ref.abs()))

    # ---- forward
    W = [d64(w) for w in inp["W"]]
    bias, gamma, beta = ([d64(a) for a in inp[n]] for n in ("bias", "gamma", "beta"))
    e = d64(inp["e"])
    zr = zero_rows(c)[1].to(dev)
    zsel = torch.isin(ridx, zr)
    us, hs, parts = [], [], []
    cur = xt
    for i in range(L):
        K = g.DP if i == 0 else H
        er = e[win, i * H:(i + 1) * H]
        ref = cur @ W[i].T + bias[i] + er
        mag = cur.abs() @ W[i].abs().T + bias[i].abs() + er.abs()
        u = get(f"u{i}")
        hold("u", f"u{i}", u, ref, S * ((K + 2) * U32 * mag + UB16 * ref.abs()))
        sg, v, e_sg, e_v = silu_parts(u)
        mean, rstd, e_mean, e_rstd = ln_stats(v, e_v, H)
        d = v - mean
        ref = d * rstd * gamma[i] + beta[i]
        h = get(f"h{i}")
        hold("h", f"h{i}", h, ref, S * (gamma[i].abs() * (d.abs() * e_rstd + (e_mean + e_v) * (rstd + e_rstd) + 3 * U32 * d.abs() * rstd)
                                        + (U32 + UB16) * ref.abs()))
        if i == 0 and bool(zsel.any()):
            exact("zero_rows", "u0 of the zero rows", u[zsel], torch.zeros_like(u[zsel]))
            exact("zero_rows", "h0 of the zero-variance rows (bf16(beta))", h[zsel],
                  beta[0].to(BF).double().expand_as(h[zsel]))
        us.append(u)
        hs.append(h)
        parts.append((sg, v, e_sg, e_v, mean, rstd, e_mean, e_rstd))
        cur = h

    # ---- head, loss, dpred
    cols = partial_columns(D, H, L)
    prow = body(c, outs, "partial")[pan_t].double()
    pred = cur @ W[L].T + bias[L]
    e_p = (H + 1) * U32 * (cur.abs() @ W[L].abs().T + bias[L].abs())
    dd = pred.to(BF).double() - eps
    gs = gscale32(M, D)
    ref = dd * gs
    e_d = e_p + 2 * UB16 * pred.abs()
    dp = get("dpred")
    hold("dpred", "dpred", dp, ref, S * (gs * e_d + (4 * U32 + UB16) * ref.abs()))
    if dpw > D:
        _, c0, _, _ = lay["dpred"]
        padc = outs["dpred"][GR + ridx, c0 + D:c0 + dpw].double()
        exact("dpred", "dpred pad columns of the 16-byte store (zeros)", padc, torch.zeros_like(padc))
    n_l = 16 * g.ntd + 14
    hold("loss", "squared-error sum", prow[:, cols["loss"]:cols["loss"] + 1], segsum((dd * dd).sum(-1, keepdim=True)),
         S * segsum((2 * dd.abs() * e_d + e_d ** 2 + (n_l + 1) * U32 * dd * dd).sum(-1, keepdim=True)))
    hold("headbias", "head-bias sums", prow[:, cols["head"]:cols["head"] + D], segsum(dp), S * 8 * U32 * segsum(dp.abs()))
    padc = prow[:, cols["head"] + D:cols["head_end"]]
    exact("headbias", "head-bias sums of the columns D .. 128 ntd - 1 (zeros)", padc, torch.zeros_like(padc))

    # ---- backward
    n_b = 8 + int(math.log2(H // 8))
    n_c = H // 64 + int(math.log2(512 // H)) + 8
    gk = dp
    for i in range(L - 1, -1, -1):
        Wm, K = (W[L], g.DP) if i == L - 1 else (W[i + 1], H)
        sg, v, e_sg, e_v, mean, rstd, e_mean, e_rstd = parts[i]
        x = us[i]
        dh = gk @ Wm
        e_dh = K * U32 * (gk.abs() @ Wm.abs())
        d = v - mean
        xh = d * rstd
        e_xh = (e_v + e_mean) * (rstd + e_rstd) + d.abs() * e_rstd + 2 * U32 * xh.abs()
        hf = 1 + x * (1 - sg)
        ds = sg * hf
        e_ds = hf.abs() * e_sg + sg * (x.abs() * (e_sg + 2 * U32 * (1 - sg)) + U32 * hf.abs()) + U32 * ds.abs()
        dxh = dh * gamma[i]
        e_dxh = gamma[i].abs() * e_dh + U32 * dxh.abs()
        ma = dxh.mean(-1, keepdim=True)
        mb = (dxh * xh).mean(-1, keepdim=True)
        e_ma = ((n_b + 1) * U32 * dxh.abs().sum(-1, keepdim=True) + e_dxh.sum(-1, keepdim=True)) / H
        e_mb = ((n_b + 2) * U32 * (dxh * xh).abs().sum(-1, keepdim=True)
                + (xh.abs() * e_dxh + dxh.abs() * e_xh).sum(-1, keepdim=True)) / H
        A = dxh.abs() + ma.abs() + (xh * mb).abs()
        e_in = e_dxh + e_ma + xh.abs() * e_mb + mb.abs() * e_xh + U32 * (xh * mb).abs() + 2 * U32 * A
        ref = rstd * (dxh - ma - xh * mb) * ds
        dz = get(f"dz{i}")
        hold("dz", f"dz{i}", dz, ref, S * (ds.abs() * (rstd * e_in + e_rstd * A) + rstd * A * e_ds + 2 * U32 * rstd * A * ds.abs()
                                           + UB16 * ref.abs()))
        hold("dbias", f"dbias{i} partial rows", prow[:, cols["dbias"][i]:cols["dbias"][i] + H], segsum(dz),
             S * n_c * U32 * segsum(dz.abs()))
        hold("dbeta", f"dbeta{i} partial rows", prow[:, cols["dbeta"][i]:cols["dbeta"][i] + H], segsum(dh),
             S * segsum(e_dh + n_c * U32 * dh.abs()))
        hold("dgamma", f"dgamma{i} partial rows", prow[:, cols["dgamma"][i]:cols["dgamma"][i] + H], segsum(dh * xh),
             S * segsum(xh.abs() * e_dh + dh.abs() * e_xh + (n_c + 1) * U32 * (dh * xh).abs()))
        if c.de_lp:
            exact("de_lp", f"de_lp of block {i} (bf16 of the dbias partial row)",
                  body(c, outs, "de_lp")[pan_t, i * H:(i + 1) * H].double(),
                  body(c, outs, "partial")[pan_t, cols["dbias"][i]:cols["dbias"][i] + H].to(BF).double())
        gk = dz
    assert not msgs, "\n".join(msgs)
    return worst
