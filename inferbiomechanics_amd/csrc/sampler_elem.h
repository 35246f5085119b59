// Element helpers of every sampler update: the flat kernels of diffusion.hip, the stitched family (stitch_step.h, included by
// stitch.hip, sde.hip and resample.hip) and cfg.hip.  The vector load / store and the three rounding forms below are the
// DEFINITION of the updates' arithmetic: each spells which product is rounded and which is fused, under `fp contract(off)`,
// so a result never depends on how the compiler would contract an expression in one kernel or another, and two kernels
// that go through the same form agree bit for bit (tests/test_flat_pins_gpu.py and tests/test_stitch_kernels_gpu.py restate
// the observed forms in exact rational arithmetic).  The forms are what the bare expressions compiled to for gfx950 when the
// kernels were written; results are pinned to them, so whoever changes one changes every sampler's output.
#pragma once
#include "ib_common.h"

namespace {

// 8 elements per thread (16-byte bf16 / 2 x 16-byte fp32 accesses)
template <typename T, int V>
__device__ __forceinline__ void ldv(const T* p, float (&v)[V]) {
  if constexpr (V == 1) { v[0] = ib_to_f32(p[0]); }
  else if constexpr (sizeof(T) == 2) {
    bf16x8_t t = *reinterpret_cast<const bf16x8_t*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (float)t[e];
  } else {
    float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
}
template <typename T, int V>
__device__ __forceinline__ void stv(T* p, const float (&v)[V]) {
  if constexpr (V == 1) { p[0] = ib_from_f32<T>(v[0]); }
  else if constexpr (sizeof(T) == 2) {
    bf16x8_t o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (bf16_t)v[e];
    *reinterpret_cast<bf16x8_t*>(p) = o;
  } else {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
  }
}

// One element k of the DDIM update x' = cx * x + ce * eps of a vector of V: one lone element sums two rounded products;
// fp32 x 8 fuses cx * x into the rounded ce * eps; bf16 x 8 alternates which of the two products is rounded first.  The
// unmasked updates and the free elements of the masked ones all go through it, so they agree bit for bit.
template <typename T, int V>
__device__ __forceinline__ float ddim_mix(int k, float cx, float a, float ce, float e) {
#pragma clang fp contract(off)
  if constexpr (V == 1) return cx * a + ce * e;
  else if constexpr (sizeof(T) == 4) return __builtin_fmaf(cx, a, ce * e);
  else return (k & 1) ? __builtin_fmaf(cx, a, ce * e) : __builtin_fmaf(ce, e, cx * a);
}

// the pinned value ox * a + oz * b of a lone observed element: the sum of two rounded products
__device__ __forceinline__ float obs_pin1(float ox, float a, float oz, float b) {
#pragma clang fp contract(off)
  return ox * a + oz * b;
}

// the same value at element k of a vector of 8, either dtype, start state and step alike: oz * b is rounded and ox * a
// fused into it, except at element 1, where it is the other way round
__device__ __forceinline__ float obs_pin8(int k, float ox, float a, float oz, float b) {
#pragma clang fp contract(off)
  return k == 1 ? __builtin_fmaf(oz, b, ox * a) : __builtin_fmaf(ox, a, oz * b);
}

}  // namespace
