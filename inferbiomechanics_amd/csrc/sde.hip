// [BUILD-DEFINED] the SDE-DPM-Solver++(2M) update of the stitched loop (include/ib_hip_sde.h): stitch.hip's
// stitch_step_kernel with MODE 1 (the second-order multistep update and its fp32 history) and MODE 2 (the step noise per
// trial element and the stored noise of observed elements) together, over the same window-batch state x [N, W, T, ld] and
// under the same INVARIANT: all copies of a trial element are bitwise equal before and after every launch, in x, hist and
// z.  A file of its own: stitch.hip's instantiations are pinned by count, and diffusion.hip bit for bit.
//
// One thread owns V consecutive columns of one trial row (n, f), as there: no LDS, no atomics, the update in place.  Width
// and rounding are stitch.hip's rule, stated there once: V = 8 when ld % 8 == 0 and ib_sampler_geom allows it, else 1; the
// form of ddim_mix is chosen by column; the blend is fp32 in window order.  coef rows are (A, E, C, hx, he, G).  Per free
// element o = ddim_mix(A, x, E, eb), then fmaf(C, hist, o) in a row with C != 0, then fmaf(G, z', o) in a row with G != 0 on
// logical columns -- both branches uniform over the launch -- and hist = fmaf(hx, x, he * eb) goes to every copy.  z' is the
// draw of ib_stitch_ddim_step_noise: counter ((f D + d) >> 2, s, trial_id[n], kDomainStep), key = seed, f the TRIAL frame.
// An observed element of a G != 0 row updates its stored noise to b' = round_to_dtype(fmaf(r, b, q z')), written to every
// copy of z, and is pinned to fmaf(ox, x0, oz b'); in a G == 0 row it is obs_pin8 / obs_pin1 and z stays untouched.  So a
// table with G == 0 everywhere is ib_stitch_dpmpp_step and one with C == 0 everywhere ib_stitch_ddim_step_noise, bit for bit.
#include <type_traits>

#include "ib_common.h"
#include "launch.h"
#include "philox.h"
#include "sampler_elem.h"
#include "../../include/ib_hip_sde.h"

namespace {

constexpr int KMAX = IB_STITCH_KMAX;

struct SdeArgs {
  void* x; const void* eps; float* hist; const void* x0; void* z; const uint8_t* mask;
  const float* coef; const float* obs_coef; const float* obs_noise; const int64_t* timesteps; int64_t num_steps; int step;
  const int32_t* step_dev; int64_t* t_out;
  const int32_t* start; const int32_t* cover; const float* wn;
  const int64_t* trial_id; uint32_t k0, k1;
  int64_t N, W, T, F, ld; int D; int mix8;
};

// A COPY of trial_noise of stitch.hip (the convention sampler_elem.h documents: that file's kernels are pinned, so its
// helpers are copied, not moved).  The normals of the V elements from column c (a multiple of V) of trial row f; bit k of
// the result: element k is a logical column.  V = 8, BLK (D % 4 == 0; ld % 8 == 0 holds for every 8-wide launch): the vector
// is two whole Philox blocks, each made once or -- in the pad columns -- not at all.  Otherwise an element looks its block
// up, and neighbours that share a block share the call.  Whoever changes the draw here changes it there.
template <int V, bool BLK>
__device__ __forceinline__ unsigned trial_noise(uint32_t k0, uint32_t k1, uint32_t s, uint32_t tid, int f, int c, int D,
                                                float (&z)[V]) {
#pragma unroll
  for (int k = 0; k < V; ++k) z[k] = 0.f;
  if constexpr (V == 8 && BLK) {
    const unsigned ok = (c + 4 <= D ? 0x0fu : 0u) | (c + 8 <= D ? 0xf0u : 0u);
    const uint32_t q = ((uint32_t)f * (uint32_t)D + (uint32_t)c) >> 2;
    if (ok & 0x0fu) {
      const U4 w = philox4x32_10(U4{q, s, tid, kDomainStep}, k0, k1);
      box_muller(w.x, w.y, z[0], z[1]); box_muller(w.z, w.w, z[2], z[3]);
    }
    if (ok & 0xf0u) {
      const U4 w = philox4x32_10(U4{q + 1u, s, tid, kDomainStep}, k0, k1);
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
        if (q != cur) { w = philox4x32_10(U4{q, s, tid, kDomainStep}, k0, k1); cur = q; }
        float za, zb;
        if ((l & 2) == 0) box_muller(w.x, w.y, za, zb); else box_muller(w.z, w.w, za, zb);
        z[k] = (l & 1) ? zb : za;
        ok |= 1u << k;
      }
    }
    return ok;
  }
}

// COND: the masked update (x0, z, mask, obs_coef, obs_noise).  A row with C == 0 does not read hist, every row writes it,
// except at a vector of observed elements only.  BLK as trial_noise takes it.  The mask is read at the first copy's
// in-window frame: the caller gives every copy of an element the same mask value.
template <typename TY, int V, bool COND, bool BLK>
__global__ __launch_bounds__(256) void sde_step_kernel(SdeArgs p) {
#pragma clang fp contract(off)
  TY* __restrict__ x = (TY*)p.x;
  const TY* __restrict__ eps = (const TY*)p.eps;
  float* hist = p.hist;
  TY* zb = (TY*)p.z;
  int s = p.step_dev ? *p.step_dev : p.step;
  s = s < 0 ? 0 : (s >= p.num_steps ? (int)p.num_steps - 1 : s);
  const float cx = p.coef[6 * s], ce = p.coef[6 * s + 1], ch = p.coef[6 * s + 2];
  const float hx = p.coef[6 * s + 3], he = p.coef[6 * s + 4], sg = p.coef[6 * s + 5];
  float ox = 0.f, oz = 0.f, rr = 0.f, rq = 0.f;
  if constexpr (COND) {
    ox = p.obs_coef[2 * (s + 1)]; oz = p.obs_coef[2 * (s + 1) + 1];
    rr = p.obs_noise[2 * s]; rq = p.obs_noise[2 * s + 1];
  }
  const bool second = ch != 0.f;                                       // uniform over the launch
  const bool noisy = sg != 0.f;                                        // uniform over the launch
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
      if (second) {
        float h[V];
        ldv<float, V>(hist + off[0], h);
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = __builtin_fmaf(ch, h[j], o[j]);
      }
#pragma unroll
      for (int j = 0; j < V; ++j) hn[j] = __builtin_fmaf(hx, y[j], he * eb[j]);
    }
    if (noisy) {                                                       // after the loads: the generator hides their latency
      const unsigned ok = trial_noise<V, BLK>(p.k0, p.k1, (uint32_t)s, (uint32_t)p.trial_id[n], f, c, p.D, zn);
      if (free_any) {
#pragma unroll
        for (int j = 0; j < V; ++j)
          if ((ok >> j) & 1u) o[j] = __builtin_fmaf(sg, zn[j], o[j]);
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
        if (free_any) stv<float, V>(hist + off[k], hn);
        if constexpr (COND)
          if (put_z) stv<TY, V>(zb + off[k], b);
      }
  }
  if (p.t_out && blockIdx.x == 0) {
    const int64_t tn = (s + 1 < p.num_steps) ? p.timesteps[s + 1] : 0;
    for (int64_t b = threadIdx.x; b < p.N * p.W; b += blockDim.x) p.t_out[b] = tn;
  }
}

}  // namespace

extern "C" int ib_sde_dpmpp_step(void* x, const void* eps, float* hist, const void* x0, void* z, const uint8_t* mask,
                                 const float* coef, const float* obs_coef, const float* obs_noise_coef,
                                 const int64_t* timesteps, int64_t num_steps, int32_t step, const int32_t* step_dev,
                                 int64_t* t_out, const int32_t* start, const int32_t* cover, const float* wn,
                                 const int64_t* trial_id, uint64_t seed, int64_t N, int64_t W, int64_t T, int64_t F,
                                 int64_t D, int64_t ld, int dtype, ib_stream_t stream) {
  if (!x || !eps || !hist || !coef || !start || !cover || !wn || !trial_id || num_steps <= 0) return IB_E_ARG;
  const int given = (x0 != nullptr) + (z != nullptr) + (mask != nullptr) + (obs_coef != nullptr) +
                    (obs_noise_coef != nullptr);
  if (given != 0 && given != 5) return IB_E_ARG;                       // the masked operands come together or not at all
  if (N <= 0 || W <= 0 || T <= 0 || F < T || D <= 0 || ld < D) return IB_E_ARG;
  if (t_out && !timesteps) return IB_E_ARG;
  if (!ib_dtype_known(dtype)) return IB_E_DTYPE;
  if (T * ld >= (int64_t)1 << 31) return IB_E_UNSUPPORTED;             // offsets inside a window are 32-bit
  if (F * D >= (int64_t)1 << 31) return IB_E_UNSUPPORTED;              // the block index is one 32-bit counter word
  const bool cond = given == 5;
  const SamplerGeom g = ib_sampler_geom(N * W * T * ld, T * ld, x, eps, hist, x0, z, mask);
  const bool v8 = g.v8 && ld % 8 == 0;
  const bool blk = D % 4 == 0;                                         // with ld % 8 == 0: ib_step_noise_blk(D, ld)
  const SdeArgs p{x, eps, hist, x0, z, mask, coef, obs_coef, obs_noise_coef, timesteps, num_steps, step, step_dev, t_out,
                  start, cover, wn, trial_id, (uint32_t)(seed & 0xFFFFFFFFu), (uint32_t)(seed >> 32),
                  N, W, T, F, ld, (int)D, (int)g.mix8};
  const int grid = ib_grid_1d(N * F * ld / (v8 ? 8 : 1), 256);
  return ib_dispatch_dtype_width<8>(dtype, v8, [&](auto tag, auto width) {
    using TY = decltype(tag);
    constexpr int V = decltype(width)::value;
    auto go = [&](auto c, auto b) {
      hipLaunchKernelGGL((sde_step_kernel<TY, V, decltype(c)::value, decltype(b)::value>), dim3(grid), dim3(256), 0,
                         ib_s(stream), p);
    };
    if constexpr (V == 8) {                                            // BLK exists for the 8-wide kernels alone
      if (cond && blk) go(std::true_type{}, std::true_type{});
      else if (cond) go(std::true_type{}, std::false_type{});
      else if (blk) go(std::false_type{}, std::true_type{});
      else go(std::false_type{}, std::false_type{});
    } else {
      if (cond) go(std::true_type{}, std::false_type{});
      else go(std::false_type{}, std::false_type{});
    }
  });
}
