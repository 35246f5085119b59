// The stitched sampler updates' one kernel template, its arguments, its noise draw and its launch: included by stitch.hip
// (MODE 0, 1, 2), sde.hip (MODE 3) and resample.hip (trial_noise and the COND x BLK choice).  stitch.hip's head comment
// states the layout, the INVARIANT, the width and rounding rule and the draw; nothing in this family is copied.
#pragma once
#include <type_traits>

#include "ib_common.h"
#include "launch.h"
#include "philox.h"
#include "sampler_elem.h"
#include "../../include/ib_hip_stitch.h"

namespace {

constexpr int KMAX = IB_STITCH_KMAX;

// the kernel's arguments: MODE 0 and 1 take StitchArgs, MODE 2 StitchNoiseArgs (no hist; obs_noise, the trial ids, the key
// and D on top), MODE 3 SdeArgs (both).  Three structs and not one: the kernarg segment of the deterministic kernels stays
// three 64-byte lines, and every kernel keeps the argument offsets it was compiled with
struct StitchArgs {
  void* x; const void* eps; float* hist; const void* x0; void* z; const uint8_t* mask;
  const float* coef; const float* obs_coef; const int64_t* timesteps; int64_t num_steps; int step;
  const int32_t* step_dev; int64_t* t_out;
  const int32_t* start; const int32_t* cover; const float* wn;
  int64_t N, W, T, F, ld; int mix8;
};
struct StitchNoiseArgs {
  void* x; const void* eps; const void* x0; void* z; const uint8_t* mask;
  const float* coef; const float* obs_coef; const float* obs_noise; const int64_t* timesteps; int64_t num_steps; int step;
  const int32_t* step_dev; int64_t* t_out;
  const int32_t* start; const int32_t* cover; const float* wn;
  const int64_t* trial_id; uint32_t k0, k1;
  int64_t N, W, T, F, ld; int D; int mix8;
};
struct SdeArgs {
  void* x; const void* eps; float* hist; const void* x0; void* z; const uint8_t* mask;
  const float* coef; const float* obs_coef; const float* obs_noise; const int64_t* timesteps; int64_t num_steps; int step;
  const int32_t* step_dev; int64_t* t_out;
  const int32_t* start; const int32_t* cover; const float* wn;
  const int64_t* trial_id; uint32_t k0, k1;
  int64_t N, W, T, F, ld; int D; int mix8;
};
template <int MODE>
using stitch_args = std::conditional_t<MODE == 3, SdeArgs, std::conditional_t<MODE == 2, StitchNoiseArgs, StitchArgs>>;

// the normals of the V elements from column c (a multiple of V) of trial row f, at word `s` (the step, or the jump's visit)
// of Philox domain DOMAIN; bit k of the result: element k is a logical column.  V = 8, BLK (D % 4 == 0; ld % 8 == 0 holds
// for every 8-wide launch): the vector is two whole Philox blocks, each made once or -- in the pad columns -- not at all.
// Otherwise an element looks its block up, and neighbours that share a block share the call.
template <int V, bool BLK, uint32_t DOMAIN = kDomainStep>
__device__ __forceinline__ unsigned trial_noise(uint32_t k0, uint32_t k1, uint32_t s, uint32_t tid, int f, int c, int D,
                                                float (&z)[V]) {
#pragma unroll
  for (int k = 0; k < V; ++k) z[k] = 0.f;
  if constexpr (V == 8 && BLK) {
    const unsigned ok = (c + 4 <= D ? 0x0fu : 0u) | (c + 8 <= D ? 0xf0u : 0u);
    const uint32_t q = ((uint32_t)f * (uint32_t)D + (uint32_t)c) >> 2;
    if (ok & 0x0fu) {
      const U4 w = philox4x32_10(U4{q, s, tid, DOMAIN}, k0, k1);
      box_muller(w.x, w.y, z[0], z[1]); box_muller(w.z, w.w, z[2], z[3]);
    }
    if (ok & 0xf0u) {
      const U4 w = philox4x32_10(U4{q + 1u, s, tid, DOMAIN}, k0, k1);
      box_muller(w.x, w.y, z[4], z[5]); box_muller(w.z, w.w, z[6], z[7]);
    }
    return ok;
  } else {
    unsigned ok = 0;
    uint32_t cur = 0xffffffffu;                  // no block has this index: F * D / 4 < 2^29
    U4 w{};
#pragma unroll
    for (int k = 0; k < V; ++k) {
      if (c + k < D) {
        const int l = f * D + c + k;
        const uint32_t q = (uint32_t)l >> 2;
        if (q != cur) { w = philox4x32_10(U4{q, s, tid, DOMAIN}, k0, k1); cur = q; }
        float za, zb;
        if ((l & 2) == 0) box_muller(w.x, w.y, za, zb); else box_muller(w.z, w.w, za, zb);
        z[k] = (l & 1) ? zb : za;
        ok |= 1u << k;
      }
    }
    return ok;
  }
}

// MODE: bit 0 = DPM, bit 1 = NOISE.  COND: the masked update (x0, z, mask, obs_coef; NOISE: obs_noise too).  DPM: coef rows
// (A, E, C, hx, he) and the fp32 history, as dpmpp_step_kernel -- a row with C == 0 does not read hist (the branch is uniform
// over the launch), every row writes it, except at a vector of observed elements only.  NOISE: the gain (sigma, G) is the
// last column of the row, (cx, ce, sigma) or (A, E, C, hx, he, G); BLK as trial_noise takes it.  The mask is read at the
// first copy's in-window frame: the caller gives every copy of an element the same mask value (the Python layer's mask is
// the same in every frame).
template <typename TY, int V, bool COND, int MODE, bool BLK>
__global__ __launch_bounds__(256) void stitch_step_kernel(stitch_args<MODE> p) {
#pragma clang fp contract(off)
  constexpr bool DPM = MODE & 1, NOISE = MODE & 2;
  TY* __restrict__ x = (TY*)p.x;
  const TY* __restrict__ eps = (const TY*)p.eps;
  float* hist = nullptr;
  if constexpr (DPM) hist = p.hist;
  TY* zb = (TY*)p.z;
  constexpr int NC = (DPM ? 5 : 2) + (NOISE ? 1 : 0);
  int s = p.step_dev ? *p.step_dev : p.step;
  s = s < 0 ? 0 : (s >= p.num_steps ? (int)p.num_steps - 1 : s);
  const float cx = p.coef[NC * s], ce = p.coef[NC * s + 1];
  float ch = 0.f, hx = 0.f, he = 0.f, ox = 0.f, oz = 0.f, sg = 0.f, rr = 0.f, rq = 0.f;
  // where sg is loaded and `noisy` formed decides the scalar schedule of the prologue, so the order is deliberate: MODE 2
  // does both ahead of the other coefficients, MODE 3 loads sg after the DPM columns and forms `noisy` after `second`.
  // One order for both changes the instructions of the twelve kernels of either mode (tools/kernel_resources.py --digest
  // --kernels shows it).
  if constexpr (MODE == 2) sg = p.coef[NC * s + 2];
  bool noisy = MODE == 2 && sg != 0.f;                                 // uniform over the launch
  if constexpr (DPM) { ch = p.coef[NC * s + 2]; hx = p.coef[NC * s + 3]; he = p.coef[NC * s + 4]; }
  if constexpr (MODE == 3) sg = p.coef[NC * s + 5];
  if constexpr (COND) {
    ox = p.obs_coef[2 * (s + 1)]; oz = p.obs_coef[2 * (s + 1) + 1];
    if constexpr (NOISE) { rr = p.obs_noise[2 * s]; rq = p.obs_noise[2 * s + 1]; }
  }
  const bool second = DPM && ch != 0.f;                                // uniform over the launch
  if constexpr (MODE == 3) noisy = sg != 0.f;
  const bool mix8 = V == 8 || p.mix8;
  constexpr unsigned ALL = (1u << V) - 1;
  const int64_t ld = p.ld, cv = ld / V, nv = p.N * p.F * cv;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cv, n = r / p.F;
    const int c = (int)(i - r * cv) * V, f = (int)(r - n * p.F);
    const int w0 = p.cover[2 * f];
    int cnt = p.cover[2 * f + 1];
    cnt = cnt > KMAX ? KMAX : cnt;
    if (cnt < 1) continue;
    int64_t off[KMAX];                                                 // the element's copies, window order
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < cnt) off[k] = ((n * p.W + (w0 + k)) * p.T + (f - p.start[w0 + k])) * ld + c;
    unsigned bits = 0;
    if constexpr (COND) {
      const int64_t m0 = off[0] - (n * p.W + w0) * p.T * ld;           // the first copy's offset inside its window
      if constexpr (V == 1) {
        bits = p.mask[m0] != 0;
      } else {
        const uint64_t mv = *reinterpret_cast<const uint64_t*>(p.mask + m0);
#pragma unroll
        for (int k = 0; k < V; ++k) bits |= (((mv >> (8 * k)) & 0xff) != 0 ? 1u : 0u) << k;
      }
    }
    float o[V], hn[V], zn[V], b[V];
    bool put_z = false;
    const bool free_any = !COND || bits != ALL;
    if (free_any) {
      float y[V], e[KMAX][V], eb[V];
      ldv<TY, V>(x + off[0], y);
#pragma unroll
      for (int k = 0; k < KMAX; ++k)                                   // every load is issued before the first use
        if (k < cnt) ldv<TY, V>(eps + off[k], e[k]);
      if (cnt == 1) {
#pragma unroll
        for (int j = 0; j < V; ++j) eb[j] = e[0][j];
      } else {
        const float wa = p.wn[KMAX * f];
#pragma unroll
        for (int j = 0; j < V; ++j) eb[j] = wa * e[0][j];
#pragma unroll
        for (int k = 1; k < KMAX; ++k)
          if (k < cnt) {
            const float wk = p.wn[KMAX * f + k];
#pragma unroll
            for (int j = 0; j < V; ++j) eb[j] = __builtin_fmaf(wk, e[k][j], eb[j]);
          }
      }
#pragma unroll
      for (int j = 0; j < V; ++j)
        o[j] = mix8 ? ddim_mix<TY, 8>((c + j) & 7, cx, y[j], ce, eb[j]) : ddim_mix<TY, 1>(0, cx, y[j], ce, eb[j]);
      if constexpr (DPM) {
        if (second) {
          float h[V];
          ldv<float, V>(hist + off[0], h);
#pragma unroll
          for (int j = 0; j < V; ++j) o[j] = __builtin_fmaf(ch, h[j], o[j]);
        }
#pragma unroll
        for (int j = 0; j < V; ++j) hn[j] = __builtin_fmaf(hx, y[j], he * eb[j]);
      }
    }
    if constexpr (NOISE) {
      if (noisy) {                                                     // after the loads: the generator hides their latency
        const unsigned ok = trial_noise<V, BLK>(p.k0, p.k1, (uint32_t)s, (uint32_t)p.trial_id[n], f, c, p.D, zn);
        if (free_any) {
#pragma unroll
          for (int j = 0; j < V; ++j)
            if ((ok >> j) & 1u) o[j] = __builtin_fmaf(sg, zn[j], o[j]);
        }
      }
    }
    if constexpr (COND) {
      if (bits != 0) {
        float a[V];
        ldv<TY, V>((const TY*)p.x0 + off[0], a);
        ldv<TY, V>((const TY*)zb + off[0], b);
        if (noisy) {
#pragma unroll
          for (int j = 0; j < V; ++j)
            if ((bits >> j) & 1u) {
              b[j] = ib_to_f32(ib_from_f32<TY>(__builtin_fmaf(rr, b[j], rq * zn[j])));
              o[j] = __builtin_fmaf(ox, a[j], oz * b[j]);
            }
          put_z = true;                              // a free element of a mixed vector gets back the value it had
        } else {
#pragma unroll
          for (int j = 0; j < V; ++j)
            if ((bits >> j) & 1u) o[j] = V == 1 ? obs_pin1(ox, a[j], oz, b[j]) : obs_pin8(j, ox, a[j], oz, b[j]);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < cnt) {
        stv<TY, V>(x + off[k], o);
        if constexpr (DPM)
          if (free_any) stv<float, V>(hist + off[k], hn);
        if constexpr (COND && NOISE)
          if (put_z) stv<TY, V>(zb + off[k], b);
      }
  }
  if (p.t_out && blockIdx.x == 0) {
    const int64_t tn = (s + 1 < p.num_steps) ? p.timesteps[s + 1] : 0;
    for (int64_t b = threadIdx.x; b < p.N * p.W; b += blockDim.x) p.t_out[b] = tn;
  }
}

// the kernel form of one launch: launch(tag, width, cond, blk) with the element type as a value, V as an ib_width and COND
// and BLK as std::bool_constant.  BLK exists for the 8-wide kernels of a family that draws noise alone
template <bool NOISE, typename F>
int stitch_dispatch(int dtype, bool v8, bool cond, bool blk, F&& launch) {
  return ib_dispatch_dtype_width<8>(dtype, v8, [&](auto tag, auto width) {
    auto go = [&](auto c) {
      if constexpr (NOISE && decltype(width)::value == 8) {
        if (blk) return launch(tag, width, c, std::true_type{});
      }
      launch(tag, width, c, std::false_type{});
    };
    if (cond) go(std::true_type{}); else go(std::false_type{});
  });
}

// the checks and the launch of the four entry points.  hist is given when MODE & 1, nullptr otherwise; MODE & 2 brings
// obs_noise, trial_id and seed, and counts obs_noise among the masked operands
template <int MODE>
int stitch_launch(void* x, const void* eps, float* hist, const void* x0, void* z, const uint8_t* mask, const float* coef,
                  const float* obs_coef, const float* obs_noise, const int64_t* timesteps, int64_t num_steps, int32_t step,
                  const int32_t* step_dev, int64_t* t_out, const int32_t* start, const int32_t* cover, const float* wn,
                  const int64_t* trial_id, uint64_t seed, int64_t N, int64_t W, int64_t T, int64_t F, int64_t D, int64_t ld,
                  int dtype, ib_stream_t stream) {
  constexpr bool DPM = MODE & 1, NOISE = MODE & 2;
  if (!x || !eps || (DPM && !hist) || !coef || !start || !cover || !wn || (NOISE && !trial_id) || num_steps <= 0)
    return IB_E_ARG;
  const int all = NOISE ? 5 : 4;
  const int given = (x0 != nullptr) + (z != nullptr) + (mask != nullptr) + (obs_coef != nullptr) +
                    (NOISE && obs_noise != nullptr);
  if (given != 0 && given != all) return IB_E_ARG;                     // the masked operands come together or not at all
  if (N <= 0 || W <= 0 || T <= 0 || F < T || D <= 0 || ld < D) return IB_E_ARG;
  if (t_out && !timesteps) return IB_E_ARG;
  if (!ib_dtype_known(dtype)) return IB_E_DTYPE;
  if (T * ld >= (int64_t)1 << 31) return IB_E_UNSUPPORTED;             // offsets inside a window are 32-bit
  if (NOISE && F * D >= (int64_t)1 << 31) return IB_E_UNSUPPORTED;     // the block index is one 32-bit counter word
  const SamplerGeom g = ib_sampler_geom(N * W * T * ld, T * ld, x, eps, hist, x0, z, mask);
  const bool v8 = g.v8 && ld % 8 == 0;
  const bool blk = NOISE && D % 4 == 0;                                // with ld % 8 == 0: ib_step_noise_blk(D, ld)
  const uint32_t k0 = (uint32_t)(seed & 0xFFFFFFFFu), k1 = (uint32_t)(seed >> 32);
  const auto p = [&] {
    if constexpr (MODE == 3)
      return SdeArgs{x, eps, hist, x0, z, mask, coef, obs_coef, obs_noise, timesteps, num_steps, step, step_dev, t_out,
                     start, cover, wn, trial_id, k0, k1, N, W, T, F, ld, (int)D, (int)g.mix8};
    else if constexpr (MODE == 2)
      return StitchNoiseArgs{x, eps, x0, z, mask, coef, obs_coef, obs_noise, timesteps, num_steps, step, step_dev, t_out,
                             start, cover, wn, trial_id, k0, k1, N, W, T, F, ld, (int)D, (int)g.mix8};
    else
      return StitchArgs{x, eps, hist, x0, z, mask, coef, obs_coef, timesteps, num_steps, step, step_dev, t_out,
                        start, cover, wn, N, W, T, F, ld, (int)g.mix8};
  }();
  const int grid = ib_grid_1d(N * F * ld / (v8 ? 8 : 1), 256);
  return stitch_dispatch<NOISE>(dtype, v8, given == all, blk, [&](auto tag, auto width, auto c, auto b) {
    hipLaunchKernelGGL((stitch_step_kernel<decltype(tag), decltype(width)::value, decltype(c)::value, MODE,
                                           decltype(b)::value>), dim3(grid), dim3(256), 0, ib_s(stream), p);
  });
}

}  // namespace
