"""Shared by tests/test_batchnorm_kernels_gpu.py and tests/test_batchnorm_bounds_cpu.py: the case table of the BatchNorm1d
kernels (csrc/batchnorm.hip), their launch geometry restated in Python, the seeded inputs, the float64 reference
(reference_fwd / reference_bwd) and the ELEMENTWISE error bound every output is held to (bound_fwd / bound_bwd).

Layouts: x, y, dy, dx, aux [B, C] rows of pitch ld >= C in the storage dtype (fp32 or bf16); gamma, beta, the running
statistics, save_mean, save_rstd, dgamma, dbeta [C] fp32.  A workgroup owns 64 columns; its 4 waves take the rows
w, w + 4, w + 8, ... and their partial sums are combined as ((w0 + w1) + w2) + w3.

Reference (float64, on the STORED inputs; m = momentum and eps are the fp32 values the kernel receives, widened):
  training: mean = sum x / B, ss = sum (x - mean)^2, var = ss / B, rstd = 1 / sqrt(var + eps),
            y = (x - mean) rstd gamma + beta, running_mean' = (1 - m) running_mean + m mean,
            running_var' = (1 - m) running_var + m ss / (B - 1)            (torch's unbiased update)
  eval:     mean = running_mean, var = running_var; nothing is updated
  backward: xh = (x - save_mean) save_rstd with the fp32 save_mean / save_rstd THE KERNEL IS HANDED, widened (so the bound
            covers the backward's own arithmetic only), tg = dgamma = sum dy xh, tb = dbeta = sum dy, k = gamma save_rstd,
            training: v = k (dy - (tb + xh tg) / B), eval: v = k dy, dx = v act'(aux).  aux is what ib_act_bwd of
            csrc/ib_common.h reads: the OUTPUT of the activation below for relu, tanh, sigmoid and elu, its
            PRE-ACTIVATION for silu.

The bound.  u = 2^-24 is the unit roundoff of fp32, |fl(a) - a| <= u |a|; u_store is that of the storage dtype (2^-24, or
2^-8 for bf16; see tests/attention_cases.py for why not 2^-9).  A column sum of the kernel is at most ceil(B / 4) additions
in a wave and 3 to combine the waves: n = ceil(B / 4) + 3 roundings, each on a partial sum no larger than the sum of the
absolute terms.  First-order propagation of every rounding, and one safety factor S = 2 on the whole for the second-order
terms (a rounding acts on a value that already carries the earlier errors; products of two errors).  S is the only
constant and it is not tuned: tests/test_batchnorm_bounds_cpu.py shows that an fp32 emulation in the kernel's summation
order stays inside (at most half of it), and that nine one-line bugs fall outside: the one-pass variance by a factor of
7 on the bf16 offset inputs, where sum x^2 is exact and only B mean^2 rounds, every other by 1e4 or more.
Forward, training:
  e_mean = (n + 1) u sum|x| / B                               n additions and the division
  e_ss   = (n + 4) u ss + 2 e_mean sum|x - mean| + B e_mean^2
      d = fl(x - mean^) is off by e_mean + u |d|, so d^2 by 2 |d| e_mean + 2 u d^2 + e_mean^2 and one more u d^2 for the
      product; n u ss for the additions; one u ss for the division by B that follows
  e_var  = e_ss / B
  e_rstd = rstd (0.5 e_var / (var + eps) + 3 u)               the addition of eps, the square root, the division
  e_y    = |gamma| (|x - mean| e_rstd + e_mean rstd + 4 u |x - mean| rstd) + u_store |y|
      the subtraction and two products on the first term; the addition of beta (fp32) or the storage rounding on |y|
  running_mean': m e_mean + u (2 (1 - m) |running_mean| + m |mean| + |running_mean'|)
      (1 - m) rounds, both products round, the sum rounds
  running_var':  m e_ss / (B - 1) + u (2 m ss / (B - 1) + 2 (1 - m) running_var + running_var')
Forward, eval: e_mean = e_var = 0 (save_mean IS running_mean, bit for bit), the rest as above.
Backward, xh^ = fl(fl(x - save_mean) save_rstd) is off by 2 u |xh|:
  e_tg = (n + 3) u sum|dy xh|,   e_tb = n u sum|dy|           dgamma and dbeta; accumulate adds u |old + value|
  training, q = (tb + xh tg) / B:
    e_q = (e_tb + |xh| e_tg + 3 u |xh tg| + 3 u (|tb| + |xh tg|)) / B
        xh^ tg^: the error of tg, 2 u of xh^, the product; then the sum, 1 / B rounded to fp32, the product with it
    e_v = |k| (e_q + u |dy - q|) + 2 u |v|                    the subtraction; k = fl(gamma save_rstd), the product
  eval: e_v = 2 u |v|
  the activation factor f = act'(aux), e_f:
    none, relu 0;  tanh (1 - a^2) u (a^2 + |f|);  sigmoid (a (1 - a)) 2 u |f|;  elu 0 for a > 0, else u |f|
    silu, sg = 1 / (1 + exp(-a)): the hardware exponential is within 2 ulp = 4 u, the addition and the division round:
      e_sg = 6 u sg, and f = sg (1 + a (1 - sg)):
      e_f = |1 + a (1 - sg)| e_sg + sg (|a| (e_sg + 2 u (1 - sg)) + u |1 + a (1 - sg)|) + u |f|
  e_dx = |f| e_v + |v| e_f + u |dx| + u_store |dx|            the product with f, the storage rounding
A bound of exactly 0 (gamma = 0: dx is 0 and y is beta, whatever x holds) admits only the exact value."""
import math
import zlib
from collections import namedtuple

import torch

DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
U32, UB16 = 2.0 ** -24, 2.0 ** -8
U = {"bf16": UB16, "fp32": U32}
S = 2.0
MOMENTUM = float(torch.tensor(0.1, dtype=torch.float32))             # what the kernel receives: the fp32 nearest to 0.1
EPS = float(torch.tensor(1e-5, dtype=torch.float32))
ACTS = ("none", "relu", "tanh", "sigmoid", "elu", "silu")
BN_COLS, BN_WAVES = 64, 4

# geom = what the case pins, as (workgroups, live columns of the last one, rows per wave): checked against geometry()
Case = namedtuple("Case", "name B C ld offset spread geom")
CASES = [
    Case("two_rows", 2, 5, 5, 0.25, 1.0, (1, 5, (1, 1, 0, 0))),             # waves 2, 3 idle; unbiased factor B / (B - 1) = 2
    Case("three_rows", 3, 64, 64, 0.25, 1.0, (1, 64, (1, 1, 1, 0))),        # one full column block, one idle wave
    Case("ragged_waves", 6, 48, 56, 0.25, 1.0, (1, 48, (2, 2, 1, 1))),      # column tail inside a block; pitched
    Case("block_plus_one", 7, 65, 72, 0.25, 1.0, (2, 1, (2, 2, 2, 1))),     # second workgroup with one live column
    Case("mid", 37, 130, 136, 0.25, 1.0, (3, 2, (10, 9, 9, 9))),            # three blocks, B % 4 == 1
    Case("long", 1030, 70, 72, 0.25, 1.0, (2, 6, (258, 258, 257, 257))),    # ~258 additions per wave
    Case("offset", 37, 20, 24, 100.0, 0.01, (1, 20, (10, 9, 9, 9))),        # positions near a metre, millimetre spread
    Case("offset_small_B", 6, 8, 8, 100.0, 0.01, (1, 8, (2, 2, 1, 1))),     # the same at B = 6
    Case("eval_one_row", 1, 5, 8, 0.25, 1.0, (1, 5, (1, 0, 0, 0))),         # eval only: training refuses B = 1
]
BY_NAME = {c.name: c for c in CASES}
TRAIN_CASES = [c for c in CASES if c.B > 1]
# bf16 cannot hold 100 +- 0.01 (it collapses to one value): its offset cases use 127 + 0.5 k, k in {-1, 0, 1}, the largest
# offset against the spread that 8 significant bits hold (the spacing of bf16 is 0.5 from 64 to 128)
BF16_OFFSET, BF16_STEP, BF16_K = 127.0, 0.5, 1


def is_offset(c):
    return c.offset > 16 * c.spread


def n_adds(B):
    return (B + BN_WAVES - 1) // BN_WAVES + 3


def geometry(B, C):
    """the launch of ib_batchnorm_fwd / _bwd: (workgroups, live columns of the last one, rows per wave)"""
    blocks = (C + BN_COLS - 1) // BN_COLS
    return blocks, C - (blocks - 1) * BN_COLS, tuple(len(range(w, B, BN_WAVES)) for w in range(BN_WAVES))


# ---- activations (float64) ---------------------------------------------------------------------------------------------
def act64(act, z):
    if act == "relu":
        return z.clamp_min(0)
    if act == "tanh":
        return torch.tanh(z)
    if act == "sigmoid":
        return torch.sigmoid(z)
    if act == "elu":
        return torch.where(z > 0, z, torch.expm1(z.clamp_max(0)))
    if act in ("silu", "none"):                                      # silu hands its pre-activation down
        return z
    raise KeyError(act)


def act_grad64(act, a, u=U32):
    """(f = act'(.) from aux as ib_act_bwd reads it, e_f = the first-order fp32 error of computing it) in float64"""
    zero = torch.zeros_like(a)
    if act == "none":
        return torch.ones_like(a), zero
    if act == "relu":
        return (a > 0).double(), zero
    if act == "tanh":
        f = 1 - a * a
        return f, u * (a * a + f.abs())
    if act == "sigmoid":
        f = a * (1 - a)
        return f, 2 * u * f.abs()
    if act == "elu":
        f = torch.where(a > 0, torch.ones_like(a), a + 1)
        return f, torch.where(a > 0, zero, u * f.abs())
    if act == "silu":
        sg = torch.sigmoid(a)
        h = 1 + a * (1 - sg)
        f = sg * h
        e_sg = 6 * u * sg
        return f, h.abs() * e_sg + sg * (a.abs() * (e_sg + 2 * u * (1 - sg)) + u * h.abs()) + u * f.abs()
    raise KeyError(act)


# ---- inputs ------------------------------------------------------------------------------------------------------------
Inputs = namedtuple("Inputs", "x dy aux gamma beta running_mean running_var dgamma_old dbeta_old")


def make_inputs(c, dt):
    """Seeded in float64, then cast to the storage dtype (x, dy, aux) or fp32 (the vectors): after the cast they are the
    exact operands.  aux[act] = act(z) of one pre-activation z ~ 1.5 N(0, 1) (z itself for silu; z[0, 0] > 0 > z[0, 1]).  gamma ~ 1 + 0.5 N(0, 1)
    with gamma[0] < 0 and gamma[C - 1] = 0 exactly; the running statistics start near the data's, not at 0 and 1."""
    g = torch.Generator().manual_seed(zlib.crc32(f"{c.name}/{dt}".encode()))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    B, C = c.B, c.C
    if is_offset(c) and dt == "bf16":
        k = torch.randint(-BF16_K, BF16_K + 1, (B, C), generator=g).double()
        x, loc, scale = BF16_OFFSET + BF16_STEP * k, BF16_OFFSET, BF16_STEP * 0.8
    else:
        x, loc, scale = c.offset + c.spread * rn(B, C), c.offset, c.spread
    gamma = 1 + 0.5 * rn(C)
    gamma[0] = -(0.25 + gamma[0].abs())
    gamma[C - 1] = 0.0
    z = 1.5 * rn(B, C)
    z[0, 0], z[0, 1] = 0.75, -0.75                                   # both branches of relu and elu, at any size
    f32 = lambda t: t.to(torch.float32)
    return Inputs(x=x.to(DT[dt]), dy=rn(B, C).to(DT[dt]), aux={a: act64(a, z).to(DT[dt]) for a in ACTS if a != "none"},
                  gamma=f32(gamma), beta=f32(rn(C)), running_mean=f32(loc + 0.3 * scale * rn(C)),
                  running_var=f32(scale * scale * (0.5 + torch.rand(C, generator=g, dtype=torch.float64))),
                  dgamma_old=f32(rn(C)), dbeta_old=f32(rn(C)))


# ---- forward -----------------------------------------------------------------------------------------------------------
def reference_fwd(inp, training):
    """float64 {y, save_mean, save_rstd, running_mean, running_var} (the running statistics AFTER the call)"""
    X, g, bt = inp.x.double(), inp.gamma.double(), inp.beta.double()
    rm, rv = inp.running_mean.double(), inp.running_var.double()
    B = X.shape[0]
    if training:
        mean = X.sum(0) / B
        ss = ((X - mean) ** 2).sum(0)
        var = ss / B
        new_rm = (1 - MOMENTUM) * rm + MOMENTUM * mean
        new_rv = (1 - MOMENTUM) * rv + MOMENTUM * ss / (B - 1)
    else:
        mean, var, new_rm, new_rv = rm, rv, rm, rv
    rstd = 1 / torch.sqrt(var + EPS)
    return {"y": (X - mean) * rstd * g + bt, "save_mean": mean, "save_rstd": rstd, "running_mean": new_rm, "running_var": new_rv}


def bound_fwd(inp, dt, training):
    """the module docstring's forward bound, for the same keys as reference_fwd"""
    X, g = inp.x.double(), inp.gamma.double()
    rm, rv = inp.running_mean.double(), inp.running_var.double()
    B = X.shape[0]
    r = reference_fwd(inp, training)
    mean, rstd = r["save_mean"], r["save_rstd"]
    d = (X - mean).abs()
    u, n = U32, n_adds(B)
    zero = torch.zeros_like(mean)
    if training:
        ss = (d * d).sum(0)
        var = ss / B
        e_mean = (n + 1) * u * X.abs().sum(0) / B
        e_ss = (n + 4) * u * ss + 2 * e_mean * d.sum(0) + B * e_mean ** 2
        e_var = e_ss / B
        b_rm = MOMENTUM * e_mean + u * (2 * (1 - MOMENTUM) * rm.abs() + MOMENTUM * mean.abs() + r["running_mean"].abs())
        b_rv = MOMENTUM * e_ss / (B - 1) + u * (2 * MOMENTUM * ss / (B - 1) + 2 * (1 - MOMENTUM) * rv + r["running_var"])
    else:
        var, e_mean, e_var, b_rm, b_rv = rv, zero, zero, zero, zero
    e_rstd = rstd * (0.5 * e_var / (var + EPS) + 3 * u)
    e_y = g.abs() * (d * e_rstd + e_mean * rstd + 4 * u * d * rstd) + U[dt] * r["y"].abs()
    return {"y": S * e_y, "save_mean": S * e_mean, "save_rstd": S * e_rstd, "running_mean": S * b_rm, "running_var": S * b_rv}


# ---- backward ----------------------------------------------------------------------------------------------------------
def _bwd(inp, dt, training, act, save_mean, save_rstd, accumulate):
    X, D, g = inp.x.double(), inp.dy.double(), inp.gamma.double()
    sm, sr = save_mean.double(), save_rstd.double()
    assert save_mean.dtype == save_rstd.dtype == torch.float32
    B = X.shape[0]
    u, n = U32, n_adds(B)
    xh = (X - sm) * sr
    tg, tb = (D * xh).sum(0), D.sum(0)
    e_tg, e_tb = (n + 3) * u * (D * xh).abs().sum(0), n * u * D.abs().sum(0)
    k = g * sr
    if training:
        q = (tb + xh * tg) / B
        v = k * (D - q)
        xt = (xh * tg).abs()
        e_q = (e_tb + xh.abs() * e_tg + 3 * u * xt + 3 * u * (tb.abs() + xt)) / B
        e_v = k.abs() * (e_q + u * (D - q).abs()) + 2 * u * v.abs()
    else:
        v = k * D
        e_v = 2 * u * v.abs()
    if act == "none":
        f, e_f = torch.ones_like(v), torch.zeros_like(v)
    else:
        f, e_f = act_grad64(act, inp.aux[act].double())
    dx = v * f
    e_dx = f.abs() * e_v + v.abs() * e_f + (u + U[dt]) * dx.abs()
    if accumulate:
        tg, tb = inp.dgamma_old.double() + tg, inp.dbeta_old.double() + tb
        e_tg, e_tb = e_tg + u * tg.abs(), e_tb + u * tb.abs()
    return ({"dx": dx, "dgamma": tg, "dbeta": tb}, {"dx": S * e_dx, "dgamma": S * e_tg, "dbeta": S * e_tb})


def reference_bwd(inp, training, act, save_mean, save_rstd, accumulate=False):
    """float64 {dx, dgamma, dbeta}; save_mean / save_rstd: the fp32 vectors handed to the kernel.  accumulate: dgamma and
    dbeta are added to inp.dgamma_old / inp.dbeta_old"""
    return _bwd(inp, "fp32", training, act, save_mean, save_rstd, accumulate)[0]      # the dtype enters the bound only


def bound_bwd(inp, dt, training, act, save_mean, save_rstd, accumulate=False):
    return _bwd(inp, dt, training, act, save_mean, save_rstd, accumulate)[1]


def saved_stats(inp, training):
    """the reference's mean and rstd rounded to fp32: what a correct forward hands the backward, up to its own bound"""
    r = reference_fwd(inp, training)
    return r["save_mean"].float(), r["save_rstd"].float()


# ---- the comparison ----------------------------------------------------------------------------------------------------
def violations(what, got, ref, bound):
    """(None or a failure message, the largest error / bound).  A non-finite output is a violation; where the bound is 0
    only the exact value passes."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    fin = torch.isfinite(got)
    if not fin.all():
        return f"{what}: {int((~fin).sum())} of {got.numel()} elements not finite", math.inf
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    bad = err > bound
    if not bad.any():
        return None, worst
    i = tuple(bad.nonzero()[0].tolist())
    return (f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bound, first at {i}: got {got[i].item()!r}, reference "
            f"{ref[i].item()!r}, bound {bound[i].item():.3e}, worst error / bound {worst:.3g}"), worst
