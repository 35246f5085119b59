// [BUILD-DEFINED] stitched sampler updates (include/ib_hip_stitch.h): the DDIM and DPM-Solver++(2M) updates of a trial of F
// frames that is denoised as W overlapping windows of T frames (MultiDiffusion / DiffCollage stitching).  The state stays
// the window batch the denoiser plan consumes, x [N, W, T, ld]; a trial element (n, f, c) has one copy x[n, w, f - start[w], c]
// in every window w that covers frame f.  INVARIANT: all copies of a trial element are bitwise equal before and after every
// launch.  The update blends the noise predictions of the covering windows, updates the element once and writes the one
// result to every copy.
//
// One thread owns V consecutive columns of one trial row (n, f): it alone reads and writes the copies of those elements, so
// the update is in place with no LDS and no atomics.  Per launch it reads count x the eps bytes of a row (count = windows
// that cover the frame, <= IB_STITCH_KMAX), x (and hist, x0, z where used) once from the first copy, and writes x (and hist)
// count times.
//
// WIDTH AND ROUNDING, stated once.  V = 8 (16-byte accesses) when ld % 8 == 0 and ib_sampler_geom (launch_geom.h, called
// unchanged with per = T * ld) allows 8-wide kernels on the window buffers: a vector then never crosses a frame row.
// Otherwise V = 1.  The form of ddim_mix is chosen by COLUMN: the 8-wide form ddim_mix<T, 8>(c & 7, ...) whenever
// ib_sampler_geom's mix8 holds for the window buffers, the lone-element form otherwise.  A copy's flat offset differs from
// window to window, its column does not, so all copies of an element round alike; for ld % 8 == 0 column and flat offset
// agree modulo 8, so it is also what the 8-wide kernels of diffusion.hip do.  The blend is fp32 in window order,
// eb = wn[0] e_0, eb = fmaf(wn[k], e_k, eb); a frame with one covering window takes that window's eps bits with no multiply.
// An observed element (mask != 0) is obs_coef[s + 1] (x0, z) of the first copy: obs_pin8 in a vector, obs_pin1 alone.
#include <type_traits>

#include "ib_common.h"
#include "launch.h"
#include "sampler_elem.h"
#include "../../include/ib_hip_stitch.h"

namespace {

constexpr int KMAX = IB_STITCH_KMAX;

struct StitchArgs {
  void* x; const void* eps; float* hist; const void* x0; const void* z; const uint8_t* mask;
  const float* coef; const float* obs_coef; const int64_t* timesteps; int64_t num_steps; int step;
  const int32_t* step_dev; int64_t* t_out;
  const int32_t* start; const int32_t* cover; const float* wn;
  int64_t N, W, T, F, ld; int mix8;
};

// COND: the masked update (x0, z, mask, obs_coef); DPM: coef rows (A, E, C, hx, he) and the fp32 history, as
// dpmpp_step_kernel -- a row with C == 0 does not read hist (the branch is uniform over the launch), every row writes it,
// except at a vector of observed elements only.  The mask is read at the first copy's in-window frame: the caller gives
// every copy of an element the same mask value (the Python layer's mask is the same in every frame).
template <typename TY, int V, bool COND, bool DPM>
__global__ __launch_bounds__(256) void stitch_step_kernel(StitchArgs p) {
#pragma clang fp contract(off)
  TY* __restrict__ x = (TY*)p.x;
  const TY* __restrict__ eps = (const TY*)p.eps;
  float* hist = p.hist;
  constexpr int NC = DPM ? 5 : 2;
  int s = p.step_dev ? *p.step_dev : p.step;
  s = s < 0 ? 0 : (s >= p.num_steps ? (int)p.num_steps - 1 : s);
  const float cx = p.coef[NC * s], ce = p.coef[NC * s + 1];
  float ch = 0.f, hx = 0.f, he = 0.f, ox = 0.f, oz = 0.f;
  if constexpr (DPM) { ch = p.coef[5 * s + 2]; hx = p.coef[5 * s + 3]; he = p.coef[5 * s + 4]; }
  if constexpr (COND) { ox = p.obs_coef[2 * (s + 1)]; oz = p.obs_coef[2 * (s + 1) + 1]; }
  const bool second = DPM && ch != 0.f;                                // uniform over the launch
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
    float o[V], hn[V];
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
    if constexpr (COND) {
      if (bits != 0) {
        float a[V], b[V];
        ldv<TY, V>((const TY*)p.x0 + off[0], a);
        ldv<TY, V>((const TY*)p.z + off[0], b);
#pragma unroll
        for (int j = 0; j < V; ++j)
          if ((bits >> j) & 1u) o[j] = V == 1 ? obs_pin1(ox, a[j], oz, b[j]) : obs_pin8(j, ox, a[j], oz, b[j]);
      }
    }
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < cnt) {
        stv<TY, V>(x + off[k], o);
        if constexpr (DPM)
          if (free_any) stv<float, V>(hist + off[k], hn);
      }
  }
  if (p.t_out && blockIdx.x == 0) {
    const int64_t tn = (s + 1 < p.num_steps) ? p.timesteps[s + 1] : 0;
    for (int64_t b = threadIdx.x; b < p.N * p.W; b += blockDim.x) p.t_out[b] = tn;
  }
}

// the checks and the launch of both entry points (dpm: ib_stitch_dpmpp_step)
int stitch_launch(bool dpm, void* x, const void* eps, float* hist, const void* x0, const void* z, const uint8_t* mask,
                  const float* coef, const float* obs_coef, const int64_t* timesteps, int64_t num_steps, int32_t step,
                  const int32_t* step_dev, int64_t* t_out, const int32_t* start, const int32_t* cover, const float* wn,
                  int64_t N, int64_t W, int64_t T, int64_t F, int64_t D, int64_t ld, int dtype, ib_stream_t stream) {
  if (!x || !eps || (dpm && !hist) || !coef || !start || !cover || !wn || num_steps <= 0) return IB_E_ARG;
  const int given = (x0 != nullptr) + (z != nullptr) + (mask != nullptr) + (obs_coef != nullptr);
  if (given != 0 && given != 4) return IB_E_ARG;                       // the masked operands come together or not at all
  if (N <= 0 || W <= 0 || T <= 0 || F < T || D <= 0 || ld < D) return IB_E_ARG;
  if (t_out && !timesteps) return IB_E_ARG;
  if (!ib_dtype_known(dtype)) return IB_E_DTYPE;
  if (T * ld >= (int64_t)1 << 31) return IB_E_UNSUPPORTED;             // offsets inside a window are 32-bit
  const bool cond = given == 4;
  const SamplerGeom g = ib_sampler_geom(N * W * T * ld, T * ld, x, eps, hist, x0, z, mask);
  const bool v8 = g.v8 && ld % 8 == 0;
  const StitchArgs p{x, eps, hist, x0, z, mask, coef, obs_coef, timesteps, num_steps, step, step_dev, t_out,
                     start, cover, wn, N, W, T, F, ld, (int)g.mix8};
  const int grid = ib_grid_1d(N * F * ld / (v8 ? 8 : 1), 256);
  return ib_dispatch_dtype_width<8>(dtype, v8, [&](auto tag, auto width) {
    using TY = decltype(tag);
    constexpr int V = decltype(width)::value;
    auto go = [&](auto c, auto d) {
      hipLaunchKernelGGL((stitch_step_kernel<TY, V, decltype(c)::value, decltype(d)::value>), dim3(grid), dim3(256), 0,
                         ib_s(stream), p);
    };
    if (cond && dpm) go(std::true_type{}, std::true_type{});
    else if (cond) go(std::true_type{}, std::false_type{});
    else if (dpm) go(std::false_type{}, std::true_type{});
    else go(std::false_type{}, std::false_type{});
  });
}

}  // namespace

extern "C" int ib_stitch_ddim_step(void* x, const void* eps, const void* x0, const void* z, const uint8_t* mask,
                                   const float* coef, const float* obs_coef, const int64_t* timesteps, int64_t num_steps,
                                   int32_t step, const int32_t* step_dev, int64_t* t_out, const int32_t* start,
                                   const int32_t* cover, const float* wn, int64_t N, int64_t W, int64_t T, int64_t F,
                                   int64_t D, int64_t ld, int dtype, ib_stream_t stream) {
  return stitch_launch(false, x, eps, nullptr, x0, z, mask, coef, obs_coef, timesteps, num_steps, step, step_dev, t_out,
                       start, cover, wn, N, W, T, F, D, ld, dtype, stream);
}

extern "C" int ib_stitch_dpmpp_step(void* x, const void* eps, float* hist, const void* x0, const void* z,
                                    const uint8_t* mask, const float* coef, const float* obs_coef, const int64_t* timesteps,
                                    int64_t num_steps, int32_t step, const int32_t* step_dev, int64_t* t_out,
                                    const int32_t* start, const int32_t* cover, const float* wn, int64_t N, int64_t W,
                                    int64_t T, int64_t F, int64_t D, int64_t ld, int dtype, ib_stream_t stream) {
  return stitch_launch(true, x, eps, hist, x0, z, mask, coef, obs_coef, timesteps, num_steps, step, step_dev, t_out,
                       start, cover, wn, N, W, T, F, D, ld, dtype, stream);
}
