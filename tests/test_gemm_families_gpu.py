"""Exact parity for every kernel family of csrc/gemm.hip, csrc/gemm_small.hip and csrc/gemm_f32_small.hip, on both sides of
each dispatch edge.

Every case of CASES names an entry point, a dtype, a shape, an operand layout, its epilogue options and the kernel family the
dispatch must pick (hip.PATH_NAMES, read from ib_debug_last_path() right after the call); "-" marks a shape the entry point
must refuse without launching anything.  A shape that lands on another family fails: re-derive the case from the C predicate.

Operands are small integers (bf16: x in [-3, 3], w in [-2, 2]; fp32: x in [-2047, 2047], w in [-2, 2] -- 12 significant bits,
so an fp32 path that narrows its inputs fails), bias in [-4, 4], row-broadcast addends and the dgrad addend in [-5, 5], and
the dgrad activation operand from {-1, -1/2, 0, 1/2, 1}, where relu' / tanh' / sigmoid' / elu' are exact dyadics.  Every
product and partial sum is then exact in fp32, so the float64 reference rounded ONCE to the storage dtype (RNE, like the
kernels' static_cast) is the kernels' result bit for bit:
  forward  z = bf16(acc + bias + add_div + add_mod),  y = bf16(act(fp32 pre-activation))
  dgrad    dx = bf16(acc * act'(aux) + addend)                     (one rounding)
  wgrad    dw (+)= fp32 dz^T x,  dbias (+)= column sums of dz     (exact)
Outputs of tanh / sigmoid / silu / elu (and the silu derivative, which is not dyadic) may differ by one bf16 ulp, and by
anything below 2^-120 (sigmoid / silu of a pre-activation below -88.7, where the fp32 exp overflows and they return 0).
The NT dgrad with a transposed weight (linear_dgrad_wt, csrc/gemm_nt.hip) rounds the product to bf16 BEFORE the activation
factor and the addend -- two roundings -- which test_gemm_nt_gpu.py pins; the kernels here round once.

Memory hygiene: destinations are prefilled with NaN (an element left unwritten fails), pitched destinations carry a sentinel
in their padding columns that must survive, and pitched operands hold nonzero junk in their padding (7 in the first operand,
-5 in the second), so a read past the reduction length multiplies junk by junk and cannot cancel."""
import zlib
from collections import namedtuple

import pytest
import torch

DEV = "cuda"
SENT = 1536.0                          # exact in bf16 and fp32
AJUNK, BJUNK = 7.0, -5.0
DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
C_ENTRY = {"fwd": "ib_linear_fwd", "dgrad": "ib_linear_dgrad", "wgrad": "ib_linear_wgrad",
           "wgrad_bias": "ib_linear_wgrad_bias", "wgrad_slabs": "ib_linear_wgrad_slabs",
           "multi": "ib_linear_wgrad_slabs_multi", "skinny": "ib_linear_dgrad_skinny"}
ULP_ACTS = ("tanh", "sigmoid", "silu", "elu")

# Shapes in each wrapper's own terms -- fwd: x [M, K], w [N, K], y [M, N];  dgrad / skinny: dz [M, N], w [N, K], dx [M, K]
# (reduction N);  wgrad*: dz [M, N], x [M, K], dw [N, K] (reduction M).
# Options: act, bias (fwd, default on), z, seg (both row-broadcast addends), addend, dbias, acc (accumulate), a_off / a_pad
# (first operand placed at column a_off of a row with a_pad more columns), b_pad (second operand), c_pad (destination).
Case = namedtuple("Case", "name entry dt M N K family opt")


def _c(name, entry, dt, M, N, K, family, **opt):
    return Case(name, entry, dt, M, N, K, family, opt)


CASES = [
    # ---- bf16 forward: smallm (<= 64 tiles of 128 x 128, K >= 64, even pitches, 4-byte rows, no z) ----------------------
    _c("fwd_smallm_64_tiles", "fwd", "bf16", 512, 2048, 512, "smallm", act="relu"),
    _c("fwd_ring_80_tiles", "fwd", "bf16", 513, 2048, 512, "ring128", act="relu"),
    _c("fwd_smallm_k64", "fwd", "bf16", 100, 300, 64, "smallm"),
    _c("fwd_generic_k62", "fwd", "bf16", 100, 300, 62, "generic"),
    _c("fwd_smallm_k67_in_pitch72", "fwd", "bf16", 100, 300, 67, "smallm", a_pad=5, b_pad=5, c_pad=4),
    _c("fwd_generic_x_2byte_aligned", "fwd", "bf16", 100, 300, 64, "generic", a_off=1, a_pad=7),
    _c("fwd_smallm_seg_addends", "fwd", "bf16", 200, 512, 512, "smallm", seg=50, act="relu"),
    _c("fwd_smallm_seg_addends_tanh", "fwd", "bf16", 130, 200, 96, "smallm", seg=20, act="tanh"),
    _c("fwd_smallm_ragged_130x129x67", "fwd", "bf16", 130, 129, 67, "smallm", a_pad=5, b_pad=5, c_pad=3),
    _c("fwd_smallm_ragged_sigmoid", "fwd", "bf16", 190, 200, 96, "smallm", act="sigmoid"),
    _c("fwd_smallm_elu_no_bias", "fwd", "bf16", 77, 48, 128, "smallm", act="elu", bias=False),
    # ---- bf16 forward: NT takes over at 640 rows ------------------------------------------------------------------------
    _c("fwd_ring_639_rows", "fwd", "bf16", 639, 2048, 512, "ring128"),
    _c("fwd_nt_640_rows", "fwd", "bf16", 640, 2048, 512, "nt256x128"),
    # ---- bf16 forward: ring128 (16-byte aligned operands, K % 32 == 0) -------------------------------------------------
    _c("fwd_ring_z_silu_seg", "fwd", "bf16", 600, 512, 256, "ring128", z=True, act="silu", seg=100, c_pad=8),
    _c("fwd_ring_z_ragged", "fwd", "bf16", 300, 136, 96, "ring128", z=True, act="relu"),
    _c("fwd_ring_x_offset8", "fwd", "bf16", 600, 2048, 512, "ring128", a_off=8, a_pad=8),
    _c("fwd_generic_x_offset4", "fwd", "bf16", 600, 2048, 512, "generic", a_off=4, a_pad=4),
    _c("fwd_generic_z_k62", "fwd", "bf16", 300, 136, 62, "generic", z=True, act="sigmoid", seg=30),
    # ---- fp32 forward: f32-small (<= 16 tiles, M <= 1024, K >= 64 and even) vs generic ---------------------------------
    _c("f32_fwd_small_1024_rows", "fwd", "fp32", 1024, 256, 512, "smallm", act="relu"),
    _c("f32_fwd_generic_1025_rows", "fwd", "fp32", 1025, 256, 512, "generic", act="relu"),
    _c("f32_fwd_small_16_tiles", "fwd", "fp32", 256, 1024, 512, "smallm"),
    _c("f32_fwd_generic_18_tiles", "fwd", "fp32", 256, 1032, 512, "generic"),
    _c("f32_fwd_small_k64_z", "fwd", "fp32", 100, 300, 64, "smallm", z=True, act="relu", c_pad=3),
    _c("f32_fwd_generic_k62", "fwd", "fp32", 100, 300, 62, "generic"),
    _c("f32_fwd_generic_k65", "fwd", "fp32", 100, 300, 65, "generic", a_pad=3, b_pad=1),
    _c("f32_fwd_generic_seg", "fwd", "fp32", 60, 100, 128, "generic", seg=7, act="relu"),
    _c("f32_fwd_small_reference_shape", "fwd", "fp32", 64, 512, 1470, "smallm", act="relu"),
    # ---- bf16 dgrad: smallm (reduction 64 .. 1024, output columns % 16, no addend) -------------------------------------
    _c("dgrad_smallm_red1024", "dgrad", "bf16", 256, 1024, 512, "smallm", act="relu"),
    _c("dgrad_ring_red1056", "dgrad", "bf16", 256, 1056, 512, "ring128", act="relu"),
    _c("dgrad_smallm_cols304", "dgrad", "bf16", 256, 512, 304, "smallm"),
    _c("dgrad_ring_cols296", "dgrad", "bf16", 256, 512, 296, "ring128"),
    _c("dgrad_generic_cols300", "dgrad", "bf16", 256, 512, 300, "generic", act="tanh", addend=True),
    _c("dgrad_ring_addend", "dgrad", "bf16", 256, 512, 512, "ring128", act="sigmoid", addend=True),
    _c("dgrad_smallm_64_tiles", "dgrad", "bf16", 512, 512, 2048, "smallm"),
    _c("dgrad_ring_80_tiles", "dgrad", "bf16", 513, 512, 2048, "ring128", act="elu", addend=True),
    _c("dgrad_smallm_relu", "dgrad", "bf16", 200, 256, 128, "smallm", act="relu"),
    _c("dgrad_smallm_tanh", "dgrad", "bf16", 200, 256, 128, "smallm", act="tanh"),
    _c("dgrad_smallm_sigmoid", "dgrad", "bf16", 200, 256, 128, "smallm", act="sigmoid"),
    _c("dgrad_smallm_silu", "dgrad", "bf16", 200, 256, 128, "smallm", act="silu"),
    _c("dgrad_smallm_elu", "dgrad", "bf16", 200, 256, 128, "smallm", act="elu"),
    _c("dgrad_smallm_ragged_red", "dgrad", "bf16", 77, 100, 48, "smallm", act="relu"),
    # ---- fp32 dgrad: f32-small vs generic ------------------------------------------------------------------------------
    _c("f32_dgrad_small_1024_rows", "dgrad", "fp32", 1024, 512, 256, "smallm", act="tanh", addend=True),
    _c("f32_dgrad_generic_1025_rows", "dgrad", "fp32", 1025, 512, 256, "generic", act="tanh", addend=True),
    _c("f32_dgrad_small_red64", "dgrad", "fp32", 100, 64, 300, "smallm", act="sigmoid"),
    _c("f32_dgrad_generic_red62", "dgrad", "fp32", 100, 62, 300, "generic", act="sigmoid"),
    _c("f32_dgrad_generic_red65", "dgrad", "fp32", 100, 65, 300, "generic", act="elu", addend=True),
    _c("f32_dgrad_small_16_tiles", "dgrad", "fp32", 256, 300, 1024, "smallm", act="relu", addend=True),
    _c("f32_dgrad_generic_18_tiles", "dgrad", "fp32", 256, 300, 1040, "generic", act="relu"),
    # ---- weight gradients: wgrad_small (M <= 1024 bf16) / split-M ring128 / generic ------------------------------------
    _c("wgrad_small_1024_rows", "wgrad", "bf16", 1024, 256, 192, "wgrad_small"),
    _c("wgrad_generic_1025_rows", "wgrad", "bf16", 1025, 256, 192, "generic"),
    _c("wgrad_ring_1056_rows", "wgrad", "bf16", 1056, 256, 192, "ring128"),
    _c("wgrad_ring_ragged_chunk_4064", "wgrad", "bf16", 4064, 128, 128, "ring128"),
    _c("wgrad_generic_4063", "wgrad", "bf16", 4063, 128, 128, "generic"),
    _c("wgrad_ring_split1_direct_accumulate", "wgrad", "bf16", 2048, 2048, 2048, "ring128", acc=True),
    _c("wgrad_ring_k66_scalar_reduce", "wgrad", "bf16", 4064, 64, 66, "ring128", a_pad=8, b_pad=6, c_pad=2),
    _c("wgrad_ring_strided_dw_accumulate", "wgrad", "bf16", 3008, 128, 64, "ring128", acc=True, c_pad=6),
    _c("wgrad_small_strided_accumulate", "wgrad", "bf16", 300, 300, 200, "wgrad_small", acc=True, c_pad=6),
    _c("f32_wgrad_generic", "wgrad", "fp32", 512, 300, 200, "generic"),
    _c("f32_wgrad_generic_strided_accumulate", "wgrad", "fp32", 1000, 128, 66, "generic", acc=True, c_pad=6),
    _c("wgrad_bias_small", "wgrad_bias", "bf16", 256, 512, 200, "wgrad_small", acc=True, c_pad=6),
    _c("wgrad_bias_small_1024_rows", "wgrad_bias", "bf16", 1024, 100, 72, "wgrad_small"),
    _c("wgrad_bias_refused_1025_rows", "wgrad_bias", "bf16", 1025, 100, 72, "-"),
    _c("f32_wgrad_bias_small_256_rows", "wgrad_bias", "fp32", 256, 300, 200, "wgrad_small", acc=True, c_pad=3),
    _c("f32_wgrad_bias_refused_257_rows", "wgrad_bias", "fp32", 257, 300, 200, "-"),
    _c("wgrad_slabs_small", "wgrad_slabs", "bf16", 512, 256, 192, "wgrad_small"),
    # slabs past the one-pass kernel: M % 64 != 0 (or M < 4096 alone) keeps the TN kernels out; chunk 64, reduction % 32
    _c("wgrad_slabs_ring_1056_rows", "wgrad_slabs", "bf16", 1056, 256, 192, "ring128"),
    _c("wgrad_slabs_generic_1025_rows", "wgrad_slabs", "bf16", 1025, 256, 192, "generic"),
    # K % 4 != 0 fails the one-slab branch, a pitch of 190 the ring's 16-byte pieces; scalar slab stores
    _c("wgrad_slabs_generic_k190", "wgrad_slabs", "bf16", 512, 256, 190, "generic"),
    _c("f32_wgrad_slabs_generic", "wgrad_slabs", "fp32", 512, 300, 200, "generic"),
    # ---- grouped weight gradients on the ring kernel: M % 64 != 0, so the TN kernels decline ----------------------------
    _c("multi_ring_m4000", "multi", "bf16", 4000, 0, 0, "ring_multi", probs=[(300, 512, 4, 0), (512, 512, 0, 0),
                                                                            (512, 300, 0, 4)]),
    # ---- skinny dgrad (M <= 256, N % 128 == 0 and <= 1024, K % 16 == 0) --------------------------------------------------
    _c("skinny_256_rows", "skinny", "bf16", 256, 1024, 512, "skinny", act="relu", dbias=True),
    _c("skinny_refused_257_rows", "skinny", "bf16", 257, 1024, 512, "-", act="relu", dbias=True),
    _c("skinny_red896", "skinny", "bf16", 64, 896, 256, "skinny", act="tanh"),
    _c("skinny_red1024_silu", "skinny", "bf16", 70, 1024, 256, "skinny", act="silu"),
    _c("skinny_refused_red1152", "skinny", "bf16", 64, 1152, 256, "-", act="tanh"),
    _c("skinny_k16_one_workgroup", "skinny", "bf16", 100, 512, 16, "skinny", act="sigmoid", dbias=True, acc=True),
    _c("skinny_dbias_accumulate", "skinny", "bf16", 200, 1024, 128, "skinny", dbias=True, acc=True),
]

# every (entry point, dtype, family) the GEMM dispatch can produce outside the NT / TN kernels, plus the NT forward edge
FAMILIES = {
    ("ib_linear_fwd", "bf16", "smallm"), ("ib_linear_dgrad", "bf16", "smallm"),
    ("ib_linear_fwd", "bf16", "ring128"), ("ib_linear_dgrad", "bf16", "ring128"), ("ib_linear_wgrad", "bf16", "ring128"),
    ("ib_linear_fwd", "bf16", "generic"), ("ib_linear_dgrad", "bf16", "generic"), ("ib_linear_wgrad", "bf16", "generic"),
    ("ib_linear_fwd", "fp32", "generic"), ("ib_linear_dgrad", "fp32", "generic"), ("ib_linear_wgrad", "fp32", "generic"),
    ("ib_linear_dgrad_skinny", "bf16", "skinny"),
    ("ib_linear_wgrad", "bf16", "wgrad_small"), ("ib_linear_wgrad_bias", "bf16", "wgrad_small"),
    ("ib_linear_wgrad_slabs", "bf16", "wgrad_small"), ("ib_linear_wgrad_slabs", "bf16", "ring128"),
    ("ib_linear_wgrad_slabs", "bf16", "generic"), ("ib_linear_wgrad_slabs", "fp32", "generic"),
    ("ib_linear_wgrad_slabs_multi", "bf16", "ring_multi"),
    ("ib_linear_fwd", "fp32", "smallm"), ("ib_linear_dgrad", "fp32", "smallm"), ("ib_linear_wgrad_bias", "fp32", "wgrad_small"),
    ("ib_linear_fwd", "bf16", "nt256x128"),
}


def test_case_table_covers_every_gemm_family():
    """CPU: the table above may not lose a family, and its names are unique"""
    got = {(C_ENTRY[c.entry], c.dt, c.family) for c in CASES if c.family != "-"}
    assert got == FAMILIES, (sorted(FAMILIES - got), sorted(got - FAMILIES))
    assert len({c.name for c in CASES}) == len(CASES)
    from inferbiomechanics_amd import hip
    assert {f for _, _, f in FAMILIES} <= set(hip.PATH_NAMES.values())


# ---- operands / references ---------------------------------------------------------------------------------------------
def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _dyadic(g, shape):
    return torch.randint(-2, 3, shape, generator=g).double() / 2


def _first(g, dt, shape):
    return _ints(g, shape, -3, 3) if dt == "bf16" else _ints(g, shape, -2047, 2047)


def _place(vals, dt, junk, off=0, pad=0):
    """vals [R, C] at column `off` of a device buffer [R, off + C + pad] whose other entries hold `junk`"""
    R, C = vals.shape
    buf = torch.full((R, off + C + pad), junk, dtype=DT[dt], device=DEV)
    view = buf[:, off:off + C]
    view.copy_(vals.to(DT[dt]))
    return view


class _Dest:
    """a destination [R, C] in a buffer with `pad` sentinel columns; the elements themselves start as `fill`"""

    def __init__(self, R, C, dtype, pad=0, fill=None):
        self.C = C
        self.buf = torch.full((R, C + pad), SENT, dtype=dtype, device=DEV)
        self.view = self.buf[:, :C]
        if fill is None:
            self.view.fill_(float("nan"))
        else:
            self.view.copy_(fill.to(dtype))

    def padding_intact(self):
        return bool((self.buf[:, self.C:] == SENT).all())


def _act(name, v):
    if name == "relu":
        return v.clamp(min=0)
    if name == "tanh":
        return torch.tanh(v)
    if name == "sigmoid":
        return torch.sigmoid(v)
    if name == "silu":
        return v * torch.sigmoid(v)
    if name == "elu":
        return torch.where(v > 0, v, torch.expm1(v))
    return v


def _act_bwd(name, a):
    """act' in terms of the operand the kernels get: the layer's output (the pre-activation for silu)"""
    if name == "relu":
        return (a > 0).double()
    if name == "tanh":
        return 1 - a * a
    if name == "sigmoid":
        return a * (1 - a)
    if name == "elu":
        return torch.where(a > 0, torch.ones_like(a), a + 1)
    if name == "silu":
        s = torch.sigmoid(a)
        return s * (1 + a * (1 - s))
    return torch.ones_like(a)


def _same(out, ref64, dtype, what, ulp1=False):
    got = out.detach().cpu()
    exp = ref64.to(dtype)
    assert torch.isfinite(got.float()).all(), f"{what}: {int((~torch.isfinite(got.float())).sum())} elements unwritten"
    if not ulp1:
        bad = got != exp
        if bad.any():
            i = tuple(bad.nonzero()[0].tolist())
            raise AssertionError(f"{what}: {int(bad.sum())} elements differ, first at {list(i)}: {got[i].item()} vs "
                                 f"{exp[i].item()}, max |diff| {(got.double() - exp.double()).abs().max().item()}")
        return
    assert dtype == torch.bfloat16
    g, e = got.double(), exp.double()
    _, ex = torch.frexp(torch.maximum(g.abs(), e.abs()))
    # bf16 has 8 significant bits.  Past v = -88.7 the kernels' fp32 exp(-v) overflows and sigmoid / silu return 0, where
    # the true value is below 88.8 e^-88.7 < 2^-120
    ulp = torch.ldexp(torch.ones_like(g), ex - 8).clamp(min=2.0 ** -120)
    bad = (g - e).abs() > ulp
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} elements beyond 1 bf16 ulp, first at {list(i)}: "
                             f"{g[i].item()} vs {e[i].item()}")


def _call(hip, fn):
    """run fn and return (its result, the family the dispatch stamped on this thread)"""
    lib = hip.lib()
    lib.ib_debug_last_path()                                   # read-and-clear
    ret = fn()
    path = hip.PATH_NAMES[int(lib.ib_debug_last_path())]
    torch.cuda.synchronize()
    return ret, path


# ---- one runner per entry point --------------------------------------------------------------------------------------------
def _run_fwd(hip, c, g):
    o, dt = c.opt, DT[c.dt]
    M, N, K = c.M, c.N, c.K
    x64, w64 = _first(g, c.dt, (M, K)), _ints(g, (N, K), -2, 2)
    x = _place(x64, c.dt, AJUNK, o.get("a_off", 0), o.get("a_pad", 0))
    w = _place(w64, c.dt, BJUNK, 0, o.get("b_pad", 0))
    pre = x64 @ w64.t()
    b = None
    if o.get("bias", True):
        b64 = _ints(g, (N,), -4, 4)
        b = b64.float().to(DEV)
        pre = pre + b64
    ad = am = None
    seg = o.get("seg", 0)
    if seg:
        ad64, am64 = _ints(g, (-(-M // seg), N), -5, 5), _ints(g, (seg, N), -5, 5)
        ad, am = ad64.to(DEV, dt), am64.to(DEV, dt)
        rows = torch.arange(M)
        pre = pre + ad64[rows // seg] + am64[rows % seg]
    act = o.get("act", "none")
    y = _Dest(M, N, dt, o.get("c_pad", 0))
    z = _Dest(M, N, dt, o.get("c_pad", 0)) if o.get("z") else None
    _, path = _call(hip, lambda: hip.linear_fwd(x, w, b, y.view, act=act, z=None if z is None else z.view,
                                                add_div=ad, add_mod=am, seg=seg))
    assert path == c.family, (c.name, path)
    _same(y.view, _act(act, pre), dt, "y", ulp1=act in ULP_ACTS)
    assert y.padding_intact(), "y padding written"
    if z is not None:
        _same(z.view, pre, dt, "z (pre-activation)")
        assert z.padding_intact(), "z padding written"


def _run_dgrad(hip, c, g):
    o, dt = c.opt, DT[c.dt]
    M, N, K = c.M, c.N, c.K
    dz64, w64 = _first(g, c.dt, (M, N)), _ints(g, (N, K), -2, 2)
    dz = _place(dz64, c.dt, AJUNK, o.get("a_off", 0), o.get("a_pad", 0))
    w = _place(w64, c.dt, BJUNK, 0, o.get("b_pad", 0))
    act = o.get("act", "none")
    aux64 = _dyadic(g, (M, K))
    aux = aux64.to(DEV, dt) if act != "none" else None
    ref = (dz64 @ w64) * _act_bwd(act, aux64)
    add = None
    if o.get("addend"):
        add64 = _ints(g, (M, K), -5, 5)
        add = add64.to(DEV, dt)
        ref = ref + add64
    dx = _Dest(M, K, dt, o.get("c_pad", 0))
    _, path = _call(hip, lambda: hip.linear_dgrad(dz, w, dx.view, act_below=act, aux=aux, addend=add))
    assert path == c.family, (c.name, path)
    _same(dx.view, ref, dt, "dx", ulp1=act == "silu")
    assert dx.padding_intact(), "dx padding written"


def _wgrad_operands(c, g):
    o = c.opt
    dz64, x64 = _first(g, c.dt, (c.M, c.N)), _ints(g, (c.M, c.K), -2, 2)
    dz = _place(dz64, c.dt, AJUNK, o.get("a_off", 0), o.get("a_pad", 0))
    x = _place(x64, c.dt, BJUNK, 0, o.get("b_pad", 0))
    pre = _ints(g, (c.N, c.K), -9, 9) if o.get("acc") else None
    dw = _Dest(c.N, c.K, torch.float32, o.get("c_pad", 0), pre)
    ref = dz64.t() @ x64 + (pre if pre is not None else 0)
    return dz64, dz, x, dw, ref


def _run_wgrad(hip, c, g):
    _, dz, x, dw, ref = _wgrad_operands(c, g)
    ws = torch.full((max(1, hip.linear_wgrad_workspace_bytes(c.M, c.N, c.K)),), 0x7F, dtype=torch.uint8, device=DEV)
    _, path = _call(hip, lambda: hip.linear_wgrad(dz, x, dw.view, ws, accumulate=bool(c.opt.get("acc"))))
    assert path == c.family, (c.name, path)
    _same(dw.view, ref, torch.float32, "dw")
    assert dw.padding_intact(), "dw padding written"


def _run_wgrad_bias(hip, c, g):
    dz64, dz, x, dw, ref = _wgrad_operands(c, g)
    acc = bool(c.opt.get("acc"))
    pre_b = _ints(g, (c.N,), -9, 9) if acc else torch.full((c.N,), float("nan"), dtype=torch.float64)
    db = pre_b.float().to(DEV)
    taken, path = _call(hip, lambda: hip.linear_wgrad_bias(dz, x, dw.view, db, accumulate=acc))
    assert path == c.family, (c.name, path)
    if c.family == "-":                                        # refused: nothing launched, nothing written
        assert not acc and not taken and dw.view.isnan().all() and db.isnan().all()
        return
    assert taken
    _same(dw.view, ref, torch.float32, "dw")
    _same(db, dz64.sum(0) + (pre_b if acc else 0), torch.float32, "dbias")
    assert dw.padding_intact(), "dw padding written"


def _run_wgrad_slabs(hip, c, g):
    _, dz, x, _, ref = _wgrad_operands(c, g)
    ws = torch.full((int(hip.lib().ib_linear_wgrad_slabs_workspace(c.M, c.N, c.K)),), 0x7F, dtype=torch.uint8, device=DEV)
    ns, path = _call(hip, lambda: hip.linear_wgrad_slabs(dz, x, ws))
    assert path == c.family, (c.name, path)
    slabs = ws[:ns * c.N * c.K * 4].view(torch.float32).view(ns, c.N, c.K)
    _same(slabs.double().sum(0), ref, torch.float32, f"sum of {ns} slabs")


def _run_multi(hip, c, g):
    M = c.M
    probs, parts, refs = [], [], []
    for N, K, pad_n, pad_k in c.opt["probs"]:
        dz64, x64 = _ints(g, (M, N), -3, 3), _ints(g, (M, K), -2, 2)
        dz = _place(dz64, "bf16", AJUNK, 0, pad_n)
        x = _place(x64, "bf16", BJUNK, 0, pad_k)
        ws = torch.full((int(hip.lib().ib_linear_wgrad_slabs_workspace(M, N, K)),), 0x7F, dtype=torch.uint8, device=DEV)
        probs.append((dz, x, ws))
        parts.append(torch.full((32, N), float("nan"), device=DEV))
        refs.append((dz64.t() @ x64, dz64.sum(0)))
    ns, path = _call(hip, lambda: hip.linear_wgrad_slabs_multi(probs, bias_parts=parts))
    assert path == c.family and ns is not None, (c.name, path, ns)
    for (dz, x, ws), n, part, (rw, rb) in zip(probs, ns, parts, refs):
        N, K = dz.shape[1], x.shape[1]
        slabs = ws[:n * N * K * 4].view(torch.float32).view(n, N, K)
        _same(slabs.double().sum(0), rw, torch.float32, f"[{N}, {K}]: sum of {n} slabs")
        _same(part[:n].double().sum(0), rb, torch.float32, f"[{N}, {K}]: bias partials")
        assert part[n:].isnan().all(), "bias partial rows past the split count written"


def _run_skinny(hip, c, g):
    o, dt = c.opt, DT[c.dt]
    M, N, K = c.M, c.N, c.K
    dz64, w64 = _first(g, c.dt, (M, N)), _ints(g, (N, K), -2, 2)
    dz, w = _place(dz64, c.dt, AJUNK), _place(w64, c.dt, BJUNK)
    act = o.get("act", "none")
    aux64 = _dyadic(g, (M, K))
    aux = aux64.to(DEV, dt) if act != "none" else None
    acc = bool(o.get("acc"))
    db = pre_b = None
    if o.get("dbias"):
        pre_b = _ints(g, (K,), -9, 9) if acc else torch.full((K,), float("nan"), dtype=torch.float64)
        db = pre_b.float().to(DEV)
    dx = _Dest(M, K, dt, o.get("c_pad", 0))
    taken, path = _call(hip, lambda: hip.linear_dgrad_skinny(dz, w, dx.view, act_below=act, aux=aux, dbias=db,
                                                             accumulate=acc))
    assert path == c.family, (c.name, path)
    if c.family == "-":
        assert not taken and dx.view.isnan().all()
        return
    assert taken
    ref = ((dz64 @ w64) * _act_bwd(act, aux64)).to(dt)
    _same(dx.view, ref.double(), dt, "dx", ulp1=act == "silu")
    if db is not None:          # the bias gradient is the column sum of the STORED dx (bf16 values: exact in fp32 here)
        _same(db, ref.double().sum(0) + (pre_b if acc else 0), torch.float32, "dbias")


RUN = {"fwd": _run_fwd, "dgrad": _run_dgrad, "wgrad": _run_wgrad, "wgrad_bias": _run_wgrad_bias,
       "wgrad_slabs": _run_wgrad_slabs, "multi": _run_multi, "skinny": _run_skinny}


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from inferbiomechanics_amd import hip as h
    h.lib()
    return h


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_gemm_family_exact(hip, c):
    g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
    RUN[c.entry](hip, c, g)
