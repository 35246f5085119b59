"""Exact restatement of the sampler updates' spelled fp32 forms (csrc/sampler_elem.h) in rational arithmetic: every product
and sum is formed exactly as a Fraction and rounded to float32 where the kernel rounds.  Shared by
tests/test_stitch_kernels_gpu.py and tests/test_flat_pins_gpu.py; tests/test_flat_pins_cpu.py holds it to a float32 /
math.fma restatement of the same forms."""
from fractions import Fraction

import numpy as np


def rn32(fr):
    """the float32 nearest to a Fraction, ties to even"""
    x = np.float32(float(fr))
    cands = [x, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))]
    return min(cands, key=lambda c: (abs(Fraction(float(c)) - fr), int(np.float32(c).view(np.uint32)) & 1))


def pinned(ox, a, oz, b, k, vec):
    """the observed value ox a + oz b in the kernel's fp32 arithmetic, exactly: alone the sum of two rounded products
    (obs_pin1); at element k of an 8-vector oz b is rounded and ox a fused into it, the other way round at k == 1 (obs_pin8)"""
    ox, a, oz, b = (Fraction(float(v)) for v in (ox, a, oz, b))
    if not vec:
        return rn32(Fraction(float(rn32(ox * a))) + Fraction(float(rn32(oz * b))))
    if k == 1:
        return rn32(oz * b + Fraction(float(rn32(ox * a))))
    return rn32(ox * a + Fraction(float(rn32(oz * b))))


def mixed(cx, a, ce, e, k, vec, bf16):
    """the free value cx a + ce e (ddim_mix): alone the sum of two rounded products; at element k of an 8-vector ce e is
    rounded and cx a fused into it -- for bf16 states at odd k only, at even k it is the other way round"""
    cx, a, ce, e = (Fraction(float(v)) for v in (cx, a, ce, e))
    if not vec:
        return rn32(Fraction(float(rn32(cx * a))) + Fraction(float(rn32(ce * e))))
    if bf16 and k % 2 == 0:
        return rn32(ce * e + Fraction(float(rn32(cx * a))))
    return rn32(cx * a + Fraction(float(rn32(ce * e))))


def fused(c, h, o):
    """one more fused multiply-add on a float32 value o: fmaf(c, h, o) (the history term C h of DPM-Solver++(2M))"""
    return rn32(Fraction(float(c)) * Fraction(float(h)) + Fraction(float(o)))
