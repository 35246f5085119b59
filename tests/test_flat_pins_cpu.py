"""tests/exact_fp32.py, the rational restatement the GPU pin tests compare against, reproduces the forms csrc/sampler_elem.h
spells: the header's return statements are read from the source, restated here with numpy float32 products (one IEEE
rounding each) and libm's fmaf (one rounding), and held equal to the rational version on random fp32 and bf16-valued
operands, ties and cancellations included."""
import ctypes
import ctypes.util
import os
import re

import numpy as np
import pytest

from tests.exact_fp32 import fused, mixed, pinned

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "inferbiomechanics_amd", "csrc",
                      "sampler_elem.h")
F = np.float32


@pytest.fixture(scope="module")
def fmaf():
    name = ctypes.util.find_library("m")
    if name is None:
        pytest.skip("no libm to take fmaf from")
    f = ctypes.CDLL(name).fmaf
    f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float] * 3
    return lambda a, b, c: F(f(float(a), float(b), float(c)))


def test_the_header_spells_the_forms_restated_here():
    src = re.sub(r"\s+", " ", open(HEADER).read())
    for form in ("if constexpr (V == 1) return cx * a + ce * e;",
                 "else if constexpr (sizeof(T) == 4) return __builtin_fmaf(cx, a, ce * e);",
                 "else return (k & 1) ? __builtin_fmaf(cx, a, ce * e) : __builtin_fmaf(ce, e, cx * a);",
                 "float obs_pin1(float ox, float a, float oz, float b) { #pragma clang fp contract(off) return ox * a + oz * b; }",
                 "return k == 1 ? __builtin_fmaf(oz, b, ox * a) : __builtin_fmaf(ox, a, oz * b);"):
        assert form in src, form
    assert src.count("#pragma clang fp contract(off)") == 3


def test_rational_restatement_equals_float32_arithmetic(fmaf):
    rng = np.random.default_rng(11)
    n = 4000
    vals = (rng.standard_normal((n, 4)) * np.exp2(rng.integers(-6, 6, (n, 4)))).astype(F)
    vals[: n // 2] = (vals[: n // 2].view(np.uint32) & 0xFFFF0000).view(F)        # bf16-valued operands: more ties
    vals[::7, 2:] = -vals[::7, :2]                                                # cancelling products
    for i, (p, a, q, b) in enumerate(vals):
        k = i & 7
        assert pinned(p, a, q, b, k, False) == F(p * a) + F(q * b)
        assert pinned(p, a, q, b, k, True) == (fmaf(q, b, F(p * a)) if k == 1 else fmaf(p, a, F(q * b)))
        assert mixed(p, a, q, b, k, False, False) == F(p * a) + F(q * b) == mixed(p, a, q, b, k, False, True)
        assert mixed(p, a, q, b, k, True, False) == fmaf(p, a, F(q * b))
        assert mixed(p, a, q, b, k, True, True) == (fmaf(p, a, F(q * b)) if k & 1 else fmaf(q, b, F(p * a)))
        assert fused(p, a, b) == fmaf(p, a, b)
