"""Shared by tests/test_rowops_kernels_gpu.py and tests/test_rowops_bounds_cpu.py: the case table of the LayerNorm kernels
(csrc/rowops.hip), their dispatch and launch geometry restated in Python (ln_dispatch, ln_geometry), the seeded inputs, the
float64 reference (reference_fwd / reference_bwd) and the ELEMENTWISE error bound every output is held to (bound_fwd /
bound_bwd); and the addition count of ib_segment_colsum (colsum_adds).  The conventions are those of
tests/batchnorm_cases.py: u = U32 = 2^-24, the unit roundoff of fp32; u_store = U[dt] (2^-24, or UB16 = 2^-8 for bf16); one
untuned safety factor S = 2 on the whole first-order bound; a bound of exactly 0 admits only the exact value.

Layouts: x, res, y, dy, dx, dres [M, N] contiguous rows in the storage dtype; add_div [ceil(M / seg), N] rows of pitch
ld_add; gamma, beta, dgamma, dbeta [N] fp32; mean, rstd [M] fp32.  LPR lanes share a row, a lane owns CH chunks of 8
consecutive columns: chunk c of lane l is the columns (c LPR + l) 8 ... + 7.

Reference (float64, on the STORED inputs; eps is the fp32 value the kernel receives, widened):
  forward:  z = x + a[row // seg], v = act(z) + res, mean = sum v / N, var = sum (v - mean)^2 / N,
            rstd = 1 / sqrt(var + eps), y = (v - mean) rstd gamma + beta
  backward: with the fp32 mean / rstd THE KERNEL IS HANDED, widened (so the bound covers the backward's own arithmetic):
            h = (v - mean) rstd, g = dy gamma, c1 = sum g / N, c2 = sum g h / N, dv = (g - c1 - h c2) rstd, dres = dv,
            dx = dv act'(z), dgamma = sum_rows dy h, dbeta = sum_rows dy

The bound, counted from the code.  A row sum is 8 CH serial additions in a lane and the combining levels of group_sum:
four DPP levels, and for LPR = 64 three more scalar additions ((r0 + r1) + r2) + r3: n = 8 CH + 4 (+ 3).  Each rounding acts
on a partial sum no larger than the sum of the absolute terms.  1 / N is rounded to fp32 and multiplied: 2 u where a
division would cost one.  The fast kernels (bf16, N = 512) are LPR = 64, CH = 1 in this count.
Prologue (both directions), e_z = u |z| when add_div is given (the addition), else 0:
  e_h = e_act(z) + |act'(z)| e_z;  e_v = e_h + u |v| when res is given (the addition), else e_h
  e_d = e_act'(z) + e_z for tanh, sigmoid, silu and elu (|act''| <= 1 for all four); 0 for none and relu, whose fl(z) has
        the sign of z
  the activations, t = the function value, E = exp(-z) or exp(z), rel(.) a relative error:
    libm's expf and tanhf are taken as within ULP_LIBM = 2 ulp (1 ulp = 2 u), the figure tests/batchnorm_cases.py assumes
    for the same functions of the ROCm device library; the hardware v_exp_f32 and v_rcp_f32 behind __expf and __frcp_rn as
    within ULP_HW_EXP = ULP_HW_RCP = 1 ulp (the ISA manual's figure for both), and __expf multiplies its argument by
    log2(e) first: two more roundings on the argument, 2 u |z| on the result.
    tanh:    e_t = 2 ULP_LIBM u |t|;  act' = 1 - t^2: e = 2 |t| e_t + u t^2 + u |act'|
    sigmoid: rel(E) = 2 ULP_LIBM u;  e_s = s (rel(E) (1 - s) + 2 u)   the addition of 1, the division
             act' = s (1 - s): e = e_s + 2 u |act'|
    silu:    fp32 storage as sigmoid; bf16 storage (ln_sigmoid): rel(E) = 2 ULP_HW_EXP u + 2 u |z|,
             e_s = s (rel(E) (1 - s) + u + 2 ULP_HW_RCP u);  t = z s: e_t = |z| e_s + u |t|
             act' = s (1 + z (1 - s)) = s k: e = |k| e_s + s (|z| (e_s + 2 u (1 - s)) + u |k|) + u |act'|   (batchnorm_cases)
    elu:     z > 0: 0 and 0;  else t = E - 1: e_t = 2 ULP_LIBM u E + u |t|, act' = E: e = 2 ULP_LIBM u E
Forward:
  e_mean = (sum e_v + (n + 2) u sum|v|) / N
  d = v - mean is off by w = e_v + e_mean (and u |d| for the subtraction):
  e_q    = sum (2 |d| w + w^2 + 3 u d^2) + n u sum d^2;   e_var = e_q / N + 2 u var
  e_rstd = rstd (0.5 e_var / (var + eps) + 3 u)               the addition of eps, the square root, the division
  e_y    = |gamma| (|d| e_rstd + w rstd + 3 u |d| rstd) + (u + u_store) |y|, and 0 where gamma = 0
      the subtraction and two products; the addition of beta; the storage rounding.  gamma = 0: y = fl(0 + beta) = beta
      (every beta of the table is a bf16 value, so that this holds for bf16 storage too)
  mean and rstd are held to e_mean and e_rstd.
Backward:
  e_hh = e_v rstd + 2 u |h|                                   h^ = fl(fl(v^ - mean) rstd)
  e_c1 = (n + 3) u sum|g| / N                                 the product dy gamma, n additions, 1 / N, the product
  e_c2 = (sum (|g| e_hh + 2 u |g h|) + (n + 2) u sum|g h|) / N
  e_dv = rstd (u |g| + e_c1 + u |g - c1| + |c2| e_hh + |h| e_c2 + u |h c2| + u |g - c1 - h c2|) + u |dv|
  e_dres = e_dv + u_store |dv|;   e_dx = |act'| e_dv + |dv| e_d + (u + u_store) |dx|
  dgamma, dbeta: the kernel's chain is the rows of one lane over the block's trips (T, or 4 T in the fast kernel, which takes
  four rows per trip), log2(64 / LPR) shuffle levels, 8 waves through LDS (16 in the fast kernel), then the segmented
  column sum over the `parts` partial rows: ceil(parts / RL) additions per lane in its 4-way grouped order and RL through
  LDS (RL = 16 for parts > 32, else 4): n_col of them (ln_col_adds).
  e_dgamma = sum_rows (|dy| e_hh + u |dy h|) + n_col u sum_rows |dy h|;  e_dbeta = n_col u sum_rows |dy|
  accumulate adds u |old + value|.
dy = 0 or gamma = 0 make every term of e_dx (and of e_dgamma, e_dbeta for dy = 0) vanish: exactly 0 is required."""
import math
import zlib
from collections import namedtuple

import torch

from tests.batchnorm_cases import S, U, U32, UB16, violations  # noqa: F401  (UB16 = U["bf16"]; violations is re-exported)

DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
EPS = float(torch.tensor(1e-5, dtype=torch.float32))
ACTS = ("none", "silu", "relu", "tanh", "sigmoid", "elu")
ULP_LIBM, ULP_HW_EXP, ULP_HW_RCP = 2, 1, 1                       # see the module docstring
LN_MAX_N, LN_FWD_GRID_CAP, LN_BWD_WPB, LN_MAX_PARTS = 2048, 2048, 8, 256
LNF_N, LNF_MIN_M, LNF_WAVES, LNF_ROWS = 512, 4096, 16, 4
BF16_OFFSET, BF16_STEP, BF16_K = 127.0, 0.5, 1                   # as tests/batchnorm_cases.py


# ---- dispatch and geometry, restated from csrc/rowops.hip ---------------------------------------------------------------
def ln_table(direction, N):
    """(LPR, CH) of LN_DISPATCH / LN_DISPATCH_BWD"""
    if N <= 128:
        return 16, 1
    if N <= 256:
        return 16, 2
    if N <= 512:
        return (16, 4) if direction == "fwd" else (64, 1)
    if N <= 1024:
        return 64, 2
    return 64, 4


def ln_bwd_parts(M):
    return max(1, min((M + 15) // 16, LN_MAX_PARTS))


def ln_dispatch(direction, dtype, M, N, act="none", aligned_x=True, aligned_params=True, has_add=False, ld_add=0,
                has_dres=False):
    """-> (kernel, LPR, CH, act_template, vec, vecp); kernel: "generic" or "fast512".  aligned_x: every row tensor handed over
    (x, res, y | dy, dx, dres, add_div) begins on 16 bytes; aligned_params: gamma (and the forward's beta) do."""
    assert direction in ("fwd", "bwd") and dtype in DT
    if N > LN_MAX_N:
        raise ValueError("IB_E_UNSUPPORTED")
    width = 4 if dtype == "fp32" else 8
    vec = int(N % width == 0 and aligned_x and (ld_add if has_add else 0) % width == 0)
    vecp = int(N % 4 == 0 and aligned_params)
    tmpl = {"none": 0, "silu": 4}.get(act, -1)
    fast = (dtype == "bf16" and N == LNF_N and vec and vecp and act == "none" and not has_add and M >= LNF_MIN_M
            and not (direction == "bwd" and has_dres))
    if fast:
        return "fast512", 64, 1, tmpl, vec, vecp
    return ("generic",) + ln_table(direction, N) + (tmpl, vec, vecp)


def ln_geometry(direction, kernel, LPR, M):
    """-> dict(blocks, rows_per_trip, trips, idle): the launch and the trips of a block's row loop; idle = blocks that own no
    row (the backward's must still write zeros into their partial rows)"""
    if direction == "fwd":
        rpb = 4 * LNF_ROWS if kernel == "fast512" else 4 * (64 // LPR)
        blocks = -(-M // rpb) if kernel == "fast512" else min(-(-M // rpb), LN_FWD_GRID_CAP)
        own = rpb
    else:
        blocks = ln_bwd_parts(M)
        own = LNF_WAVES if kernel == "fast512" else LN_BWD_WPB * (64 // LPR)
        rpb = own * LNF_ROWS if kernel == "fast512" else own
    per_trip = blocks * rpb
    return {"blocks": blocks, "rows_per_trip": per_trip, "trips": -(-M // per_trip),
            "idle": sum(1 for b in range(blocks) if b * own >= M)}


def colsum_rl(rows_per_seg):
    return 16 if rows_per_seg > 32 else 4


def colsum_adds(cnt, rows_per_seg=None):
    """additions on the longest path of one ib_segment_colsum output of cnt rows: the lane's rows in the 4-way grouped order,
    then RL (chosen by the launch's longest segment, rows_per_seg; default: cnt itself)"""
    rl = colsum_rl(rows_per_seg or cnt)
    return -(-cnt // rl) + rl


def row_adds(LPR, CH):
    return 8 * CH + 4 + (3 if LPR == 64 else 0)


def ln_col_adds(kernel, LPR, M):
    g = ln_geometry("bwd", kernel, LPR, M)
    if kernel == "fast512":
        return LNF_ROWS * g["trips"] + LNF_WAVES + colsum_adds(g["blocks"])
    return g["trips"] + int(math.log2(64 // LPR)) + LN_BWD_WPB + colsum_adds(g["blocks"])


# ---- the case table ----------------------------------------------------------------------------------------------------
# add: None, "vec" (a column slice of a wider matrix whose pitch keeps 16-byte rows) or "odd" (an odd pitch: vec is lost).
# mis: the tensors that begin one element into their buffer.  values: normal | offset | const | gamma0 | dy0.
# pins: what the case is in the table for, checked against ln_dispatch / ln_geometry by tests/test_rowops_bounds_cpu.py:
#   fwd, bwd = (LPR, CH);  kernel = the bf16 kernel of both directions;  vec32, vec16, vecp = the flags in fp32 / bf16;
#   fwd_trips, bwd_trips, bwd_blocks, bwd_idle = the generic geometry (fast_bwd_trips: the fast kernel's)
Case = namedtuple("Case", "name M N dts act res dres add seg mis values pins")
BOTH = ("fp32", "bf16")


def _case(name, M, N, pins, dts=BOTH, act="none", res=False, dres=False, add=None, seg=0, mis=(), values="normal"):
    return Case(name, M, N, tuple(dts), act, res, dres, add, seg, frozenset(mis), values, pins)


WIDTH_PINS = {   # N: (forward (LPR, CH), backward (LPR, CH), vec fp32, vec bf16)
    1: ((16, 1), (16, 1), 0, 0), 7: ((16, 1), (16, 1), 0, 0), 8: ((16, 1), (16, 1), 1, 1), 9: ((16, 1), (16, 1), 0, 0),
    12: ((16, 1), (16, 1), 1, 0), 127: ((16, 1), (16, 1), 0, 0), 128: ((16, 1), (16, 1), 1, 1),
    129: ((16, 2), (16, 2), 0, 0), 132: ((16, 2), (16, 2), 1, 0), 256: ((16, 2), (16, 2), 1, 1),
    257: ((16, 4), (64, 1), 0, 0), 260: ((16, 4), (64, 1), 1, 0), 264: ((16, 4), (64, 1), 1, 1),
    512: ((16, 4), (64, 1), 1, 1), 513: ((64, 2), (64, 2), 0, 0), 516: ((64, 2), (64, 2), 1, 0),
    520: ((64, 2), (64, 2), 1, 1), 1024: ((64, 2), (64, 2), 1, 1), 1025: ((64, 4), (64, 4), 0, 0),
    1032: ((64, 4), (64, 4), 1, 1), 2048: ((64, 4), (64, 4), 1, 1)}
FLAG_N = {40: ((16, 1), (16, 1)), 264: ((16, 4), (64, 1)), 520: ((64, 2), (64, 2))}

CASES = []
for _N, (_f, _b, _v32, _v16) in WIDTH_PINS.items():                # one live sub-row in the second wave-group (LPR 16)
    CASES.append(_case(f"width_{_N}", 5, _N, dict(fwd=_f, bwd=_b, vec32=_v32, vec16=_v16, vecp=int(_N % 4 == 0)), res=True))
for _M, _bl, _idle in ((1, 1, 0), (3, 1, 0), (4, 1, 0), (15, 1, 0), (16, 1, 0), (17, 2, 1), (33, 3, 1)):
    CASES.append(_case(f"rows_lpr16_{_M}", _M, 24, dict(fwd=(16, 1), bwd=(16, 1), bwd_blocks=_bl, bwd_idle=_idle, bwd_trips=1),
                       res=True, dres=True))
for _M, _bl, _tr in ((1, 1, 1), (8, 1, 1), (9, 1, 2), (16, 1, 2), (17, 2, 2)):
    CASES.append(_case(f"rows_lpr64_{_M}", _M, 264, dict(bwd=(64, 1), bwd_blocks=_bl, bwd_trips=_tr), res=True, dres=True))
CASES += [
    _case("trips_fwd_lpr16_past_grid_cap", 32771, 8, dict(fwd=(16, 1), fwd_trips=2)),
    _case("trips_fwd_lpr64", 8195, 520, dict(fwd=(64, 2), fwd_trips=2), dts=("bf16",)),
    _case("trips_bwd_generic_lpr16", 8195, 8, dict(bwd=(16, 1), bwd_trips=2, bwd_blocks=256), res=True, dres=True),
    _case("trips_bwd_generic_lpr64", 2051, 264, dict(bwd=(64, 1), bwd_trips=2, bwd_blocks=129), res=True, dres=True),
]
for _M, _tr in ((4096, 1), (4097, 1), (4099, 1), (16387, 2)):      # 16387: the fast backward's outer loop, second trip partial
    for _res in (False, True):
        CASES.append(_case(f"fast_{_M}" + ("_res" if _res else ""), _M, 512,
                           dict(kernel="fast512", fast_bwd_trips=_tr), dts=("bf16",), res=_res))
CASES += [   # the ways of NOT qualifying, at M = 4096: the generic kernel, the same bound
    _case("notfast_dres", 4096, 512, dict(kernel_fwd="fast512", kernel_bwd="generic"), dts=("bf16",), res=True, dres=True),
    _case("notfast_gamma_misaligned", 4096, 512, dict(kernel="generic", vecp=0, vec16=1), dts=("bf16",), res=True,
          mis=("gamma", "beta")),
    _case("notfast_silu", 4096, 512, dict(kernel="generic"), dts=("bf16",), act="silu", res=True),
    _case("notfast_add_div", 4096, 512, dict(kernel="generic", vec16=1), dts=("bf16",), res=True, add="vec", seg=64),
]
for _N, (_f, _b) in FLAG_N.items():
    for _act in ACTS:
        for _res in (False, True):
            for _dres in (False, True):
                CASES.append(_case(f"flags_{_N}_{_act}" + ("_res" if _res else "") + ("_dres" if _dres else ""), 13, _N,
                                   dict(fwd=_f, bwd=_b, act_template={"none": 0, "silu": 4}.get(_act, -1)), act=_act,
                                   res=_res, dres=_dres))
    for _add, _v in (("vec", 1), ("odd", 0)):                       # seg 5, M 13: a ragged last window, 3 rows of add_div
        CASES.append(_case(f"add_div_{_add}_{_N}", 13, _N, dict(fwd=_f, bwd=_b, vec32=_v, vec16=_v), act="silu", res=True,
                           dres=True, add=_add, seg=5))
for _mis in (("x",), ("res",), ("y",), ("dy",), ("dx",), ("x", "res", "y", "dy", "dx", "dres")):
    CASES.append(_case("misaligned_" + ("all_rows" if len(_mis) > 1 else _mis[0]), 13, 264,
                       dict(fwd=(16, 4), bwd=(64, 1), **({"vec32": 0, "vec16": 0} if len(_mis) > 1 else {}), vecp=1),
                       res=True, dres=True, mis=_mis))
CASES += [
    _case("misaligned_gamma_beta", 13, 264, dict(vec32=1, vec16=1, vecp=0), res=True, dres=True, mis=("gamma", "beta")),
    _case("offset_40", 13, 40, dict(fwd=(16, 1)), values="offset"),
    _case("offset_520", 13, 520, dict(fwd=(64, 2)), values="offset", res=True),
    _case("const_row_256", 5, 256, dict(fwd=(16, 2)), values="const"),
    _case("const_row_1024", 5, 1024, dict(fwd=(64, 2)), values="const"),
    _case("gamma_zero", 13, 264, dict(bwd=(64, 1)), values="gamma0", act="tanh", res=True, dres=True),
    _case("dy_zero", 13, 264, dict(bwd=(64, 1)), values="dy0", act="silu", res=True, dres=True),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
PARAMS = [(c, dt) for c in CASES for dt in c.dts]
CONST_VALUE = 4.0


def case_id(p):
    return f"{p[0].name}-{p[1]}"


def ld_add_of(c):
    return 0 if c.add is None else c.N + (16 if c.add == "vec" else 9)


def add_col0(c):
    """the first column of the add_div slice inside its wider matrix: 8 elements = 16 bytes in bf16, 32 in fp32"""
    return 8 if c.add == "vec" else 0


def dispatch_of(c, direction, dt):
    """ln_dispatch for a case.  The forward sees the alignment of x, res, y (and add_div), the backward that of x, res, dy,
    dx, dres; the forward looks at gamma and beta, the backward at gamma."""
    rows = {"fwd": {"x", "y"} | ({"res"} if c.res else set()),
            "bwd": {"x", "dy", "dx"} | ({"res"} if c.res else set()) | ({"dres"} if c.dres else set())}[direction]
    par = {"fwd": {"gamma", "beta"}, "bwd": {"gamma"}}[direction]
    return ln_dispatch(direction, dt, c.M, c.N, c.act, not (rows & c.mis), not (par & c.mis), c.add is not None, ld_add_of(c),
                       c.dres)


def pinned(c, dt):
    """what the restated dispatch gives for the keys a case may pin"""
    f, b = dispatch_of(c, "fwd", dt), dispatch_of(c, "bwd", dt)
    gf = ln_geometry("fwd", f[0], f[1], c.M)
    gb = ln_geometry("bwd", b[0], b[1], c.M)
    out = {"fwd": f[1:3], "bwd": b[1:3], "act_template": f[3], "vecp": f[5], "fwd_trips": gf["trips"], "bwd_trips": gb["trips"],
           "bwd_blocks": gb["blocks"], "bwd_idle": gb["idle"], "kernel_fwd": f[0], "kernel_bwd": b[0]}
    out["vec32" if dt == "fp32" else "vec16"] = f[4]
    assert f[4] == b[4] or c.mis, c.name
    if f[0] == b[0]:
        out["kernel"] = f[0]
    if b[0] == "fast512":
        out["fast_bwd_trips"] = gb["trips"]
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------
Inputs = namedtuple("Inputs", "x res dy add gamma beta dgamma_old dbeta_old")


def make_inputs(c, dt):
    """Seeded in float64, then cast to the storage dtype (x, res, dy, add) or fp32 (the vectors): after the cast they are the
    exact operands.  x[0, 0] > 0 > x[0, 1] (both branches of relu and elu).  gamma ~ 1 + 0.5 N(0, 1) with gamma[0] < 0 and
    gamma[N - 1] = 0 exactly; every beta is a bf16 value."""
    g = torch.Generator().manual_seed(zlib.crc32(f"{c.name}/{dt}".encode()))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    M, N = c.M, c.N
    if c.values == "offset" and dt == "bf16":
        x = BF16_OFFSET + BF16_STEP * torch.randint(-BF16_K, BF16_K + 1, (M, N), generator=g).double()
    elif c.values == "offset":
        x = 100.0 + 0.01 * rn(M, N)
    elif c.values == "const":
        x = torch.full((M, N), CONST_VALUE, dtype=torch.float64)
    else:
        x = 1.5 * rn(M, N)
        x[0, 0] = 0.75
        if N > 1:
            x[0, 1] = -0.75
    gamma = 1 + 0.5 * rn(N)
    gamma[0] = -(0.25 + gamma[0].abs())
    gamma[N - 1] = 0.0
    if c.values == "gamma0":
        gamma.zero_()
    dy = rn(M, N)
    if c.values == "dy0":
        dy.zero_()
    res = (0.01 if c.values == "offset" else 1.0) * rn(M, N) if c.res else None
    add = 0.5 * rn(-(-M // c.seg), N) if c.add else None
    st = lambda t: None if t is None else t.to(DT[dt])
    f32 = lambda t: t.to(torch.float32)
    return Inputs(x=st(x), res=st(res), dy=st(dy), add=st(add), gamma=f32(gamma), beta=f32(rn(N).to(torch.bfloat16)),
                  dgamma_old=f32(rn(N)), dbeta_old=f32(rn(N)))


# ---- activations (float64): value, derivative at the pre-activation, and the first-order fp32 error of each -------------
def act_model(act, z, dt):
    """-> (t = act(z), f = act'(z), e_t, e_f) as rowops.hip computes them for storage dtype dt (ln_act_both / act_bwd_pre)"""
    u = U32
    zero, one = torch.zeros_like(z), torch.ones_like(z)
    if act == "none":
        return z, one, zero, zero
    if act == "relu":
        return z.clamp_min(0), (z > 0).double(), zero, zero
    if act == "tanh":
        t = torch.tanh(z)
        f = 1 - t * t
        e_t = 2 * ULP_LIBM * u * t.abs()
        return t, f, e_t, 2 * t.abs() * e_t + u * t * t + u * f.abs()
    if act in ("sigmoid", "silu"):
        s = torch.sigmoid(z)
        if act == "silu" and dt == "bf16":
            e_s = s * ((2 * ULP_HW_EXP * u + 2 * u * z.abs()) * (1 - s) + u + 2 * ULP_HW_RCP * u)
        else:
            e_s = s * (2 * ULP_LIBM * u * (1 - s) + 2 * u)
        if act == "sigmoid":
            f = s * (1 - s)
            return s, f, e_s, e_s + 2 * u * f.abs()
        t, k = z * s, 1 + z * (1 - s)
        f = s * k
        return t, f, z.abs() * e_s + u * t.abs(), k.abs() * e_s + s * (z.abs() * (e_s + 2 * u * (1 - s)) + u * k.abs()) + u * f.abs()
    if act == "elu":
        E = torch.exp(z.clamp_max(0))
        t = torch.where(z > 0, z, torch.expm1(z.clamp_max(0)))
        e_E = 2 * ULP_LIBM * u * E
        return t, torch.where(z > 0, one, E), torch.where(z > 0, zero, e_E + u * t.abs()), torch.where(z > 0, zero, e_E)
    raise KeyError(act)


def _prologue(c, inp, dt):
    """float64 (z, v, f = act'(z), e_v, e_f)"""
    u = U32
    z = inp.x.double()
    e_z = torch.zeros_like(z)
    if inp.add is not None:
        rows = torch.arange(c.M, device=z.device) // c.seg
        z = z + inp.add.double()[rows]
        e_z = u * z.abs()
    t, f, e_t, e_f = act_model(c.act, z, dt)
    e_h = e_t + f.abs() * e_z
    if c.act not in ("none", "relu"):
        e_f = e_f + e_z
    v = t
    if inp.res is not None:
        v = t + inp.res.double()
        e_h = e_h + u * v.abs()
    return z, v, f, e_h, e_f


# ---- forward -----------------------------------------------------------------------------------------------------------
def _fwd(c, inp, dt, kernel_lpr_ch):
    _, LPR, CH = kernel_lpr_ch
    u, n, N = U32, row_adds(LPR, CH), c.N
    _, v, _, e_v, _ = _prologue(c, inp, dt)
    g, bt = inp.gamma.double(), inp.beta.double()
    mean = v.sum(1, keepdim=True) / N
    d = v - mean
    var = (d * d).sum(1, keepdim=True) / N
    rstd = 1 / torch.sqrt(var + EPS)
    y = d * rstd * g + bt
    e_mean = (e_v.sum(1, keepdim=True) + (n + 2) * u * v.abs().sum(1, keepdim=True)) / N
    w = e_v + e_mean
    e_q = (2 * d.abs() * w + w * w + 3 * u * d * d).sum(1, keepdim=True) + n * u * (d * d).sum(1, keepdim=True)
    e_var = e_q / N + 2 * u * var
    e_rstd = rstd * (0.5 * e_var / (var + EPS) + 3 * u)
    e_y = g.abs() * (d.abs() * e_rstd + w * rstd + 3 * u * d.abs() * rstd) + (u + U[dt]) * y.abs()
    e_y = torch.where((g == 0).expand_as(e_y), torch.zeros_like(e_y), e_y)
    return ({"y": y, "mean": mean[:, 0], "rstd": rstd[:, 0]}, {"y": S * e_y, "mean": S * e_mean[:, 0], "rstd": S * e_rstd[:, 0]})


def reference_fwd(c, inp, dt):
    """float64 {y, mean, rstd}; dt picks nothing but the error model, which the reference does not use"""
    return _fwd(c, inp, dt, ("generic", 16, 1))[0]


def bound_fwd(c, inp, dt, dispatch=None):
    """the module docstring's forward bound; dispatch: ln_dispatch's answer (default: the case's own)"""
    return _fwd(c, inp, dt, (dispatch or dispatch_of(c, "fwd", dt))[:3])[1]


def saved_stats(c, inp, dt):
    """the reference's mean and rstd rounded to fp32: what a correct forward hands the backward, up to its own bound"""
    r = reference_fwd(c, inp, dt)
    return r["mean"].float(), r["rstd"].float()


# ---- backward ----------------------------------------------------------------------------------------------------------
def _bwd(c, inp, dt, mean, rstd, accumulate, kernel_lpr_ch):
    kernel, LPR, CH = kernel_lpr_ch
    assert mean.dtype == rstd.dtype
    u, n, N = U32, row_adds(LPR, CH), c.N
    n_col = ln_col_adds(kernel, LPR, c.M)
    _, v, f, e_v, e_f = _prologue(c, inp, dt)
    D, g64 = inp.dy.double(), inp.gamma.double()
    mu, rs = mean.double()[:, None], rstd.double()[:, None]
    h = (v - mu) * rs
    g = D * g64
    gh = g * h
    c1, c2 = g.sum(1, keepdim=True) / N, gh.sum(1, keepdim=True) / N
    t = g - c1 - h * c2
    dv = t * rs
    dx = dv * f
    e_hh = e_v * rs + 2 * u * h.abs()
    e_c1 = (n + 3) * u * g.abs().sum(1, keepdim=True) / N
    e_c2 = ((g.abs() * e_hh + 2 * u * gh.abs()).sum(1, keepdim=True) + (n + 2) * u * gh.abs().sum(1, keepdim=True)) / N
    e_dv = rs * (u * g.abs() + e_c1 + u * (g - c1).abs() + c2.abs() * e_hh + h.abs() * e_c2 + u * (h * c2).abs() + u * t.abs()) \
        + u * dv.abs()
    e_dx = f.abs() * e_dv + dv.abs() * e_f + (u + U[dt]) * dx.abs()
    dh = D * h
    dg, db = dh.sum(0), D.sum(0)
    e_dg = (D.abs() * e_hh + u * dh.abs()).sum(0) + n_col * u * dh.abs().sum(0)
    e_db = n_col * u * D.abs().sum(0)
    if accumulate:
        dg, db = inp.dgamma_old.double() + dg, inp.dbeta_old.double() + db
        e_dg, e_db = e_dg + u * dg.abs(), e_db + u * db.abs()
    return ({"dx": dx, "dres": dv, "dgamma": dg, "dbeta": db},
            {"dx": S * e_dx, "dres": S * (e_dv + U[dt] * dv.abs()), "dgamma": S * e_dg, "dbeta": S * e_db})


def reference_bwd(c, inp, dt, mean, rstd, accumulate=False):
    """float64 {dx, dres, dgamma, dbeta}; mean / rstd: the fp32 vectors handed to the kernel"""
    return _bwd(c, inp, dt, mean, rstd, accumulate, ("generic", 16, 1))[0]


def bound_bwd(c, inp, dt, mean, rstd, accumulate=False, dispatch=None):
    return _bwd(c, inp, dt, mean, rstd, accumulate, (dispatch or dispatch_of(c, "bwd", dt))[:3])[1]


def inputs_to(inp, device):
    return Inputs(*(None if t is None else t.to(device) for t in inp))
