// [BUILD-DEFINED] the jump of a resampled masked loop (include/ib_hip_resample.h; RePaint, Lugmayr et al. 2022, Algorithm 1):
// the state at position s is diffused back to position q = s - back, x <- sqrt(rho) x + sqrt(1 - rho) z' at the free elements
// with fresh noise, and the observed elements are pinned to the observation at level q.  The state, the layout tables and
// the copies INVARIANT are those of stitch.hip: x [N, W, T, ld], a trial element (n, f, c) has one copy in every window
// that covers frame f, all copies bitwise equal before and after the launch.
//
// A streaming kernel: one thread owns V consecutive columns of one trial row (n, f), reads x once from the first copy (and
// x0, z, the mask where a vector holds observed elements) and writes the one result to every copy, with plain vector
// stores.  No LDS, no atomics.  The WIDTH rule is stitch.hip's, stated there: V = 8 (16-byte accesses) when ld % 8 == 0 and
// ib_sampler_geom allows 8-wide kernels on the window buffers, V = 1 otherwise.  An observed element takes the form that
// stitch_step_kernel pins at the same width, obs_pin8 by column in a vector and obs_pin1 alone, over obs_coef[q]: so it is
// what the eta = 0 update that stepped to position q wrote, bit for bit.
//
// NOISE.  The normal z' of trial element (n, f, d) is Box-Muller over Philox4x32-10 (philox.h) at counter
// ((f * D + d) >> 2, visit, trial_id[n], kDomainJump), key = seed: stitch_step.h's trial_noise, the draw of the update
// kernels, in a domain of its own, with `visit`, the ordinal of the jump within the call, where they put the step.  f is the
// TRIAL frame, so every copy of an element gets the same normal by construction.  Pad columns (d >= D) get no noise: cx * 0
// stays 0.
//
// The position lives on the device, so a launch that finds s outside back .. num_steps cannot be refused by the host: it
// reads no table row and writes nothing.
#include "stitch_step.h"
#include "../../include/ib_hip_resample.h"

namespace {

constexpr uint32_t kDomainJump = 4u;         // philox.h lists the domains

struct ResampleArgs {
  void* x; const void* x0; const void* z; const uint8_t* mask;
  const float* coef; const float* obs_coef; const int64_t* timesteps; int64_t num_steps; int step;
  const int32_t* step_dev; int back; uint32_t visit; int64_t* t_out;
  const int32_t* start; const int32_t* cover;
  const int64_t* trial_id; uint32_t k0, k1;
  int64_t N, W, T, F, ld; int D;
};

// COND: x0, z, mask, obs_coef are given.  BLK as trial_noise takes it.  The loop's head -- the copies' offsets and the mask
// bits -- is stitch_step_kernel's, repeated here: shared as device functions it changes the instructions of every kernel
// of both.
template <typename TY, int V, bool COND, bool BLK>
__global__ __launch_bounds__(256) void resample_renoise_kernel(ResampleArgs p) {
#pragma clang fp contract(off)
  const int s = p.step + (p.step_dev ? *p.step_dev : 0);
  if (s < p.back || s > p.num_steps) return;                           // uniform over the launch: no row read, nothing written
  const int q = s - p.back;
  TY* __restrict__ x = (TY*)p.x;
  const float cx = p.coef[2 * s], cz = p.coef[2 * s + 1];
  float ox = 0.f, oz = 0.f;
  if constexpr (COND) { ox = p.obs_coef[2 * q]; oz = p.obs_coef[2 * q + 1]; }
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
    float o[V];
    if (!COND || bits != ALL) {
      float y[V], zn[V];
      ldv<TY, V>(x + off[0], y);
      const unsigned ok = trial_noise<V, BLK, kDomainJump>(p.k0, p.k1, p.visit, (uint32_t)p.trial_id[n], f, c, p.D, zn);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float m = cx * y[j];
        o[j] = ((ok >> j) & 1u) ? __builtin_fmaf(cz, zn[j], m) : m;
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
      if (k < cnt) stv<TY, V>(x + off[k], o);
  }
  if (blockIdx.x == 0) {
    const int64_t tq = p.timesteps[q];
    for (int64_t b = threadIdx.x; b < p.N * p.W; b += blockDim.x) p.t_out[b] = tq;
  }
}

}  // namespace

extern "C" int ib_resample_renoise(void* x, const void* x0, const void* z, const uint8_t* mask, const float* coef,
                                   const float* obs_coef, const int64_t* timesteps, int64_t num_steps, int32_t step,
                                   const int32_t* step_dev, int32_t back, uint32_t visit, int64_t* t_out,
                                   const int32_t* start, const int32_t* cover, const int64_t* trial_id, uint64_t seed,
                                   int64_t N, int64_t W, int64_t T, int64_t F, int64_t D, int64_t ld, int dtype,
                                   ib_stream_t stream) {
  if (!x || !coef || !timesteps || !t_out || !start || !cover || !trial_id || num_steps <= 0) return IB_E_ARG;
  const int given = (x0 != nullptr) + (z != nullptr) + (mask != nullptr) + (obs_coef != nullptr);
  if (given != 0 && given != 4) return IB_E_ARG;                       // the masked operands come together or not at all
  if (back < 1) return IB_E_ARG;
  if (N <= 0 || W <= 0 || T <= 0 || F < T || D <= 0 || ld < D) return IB_E_ARG;
  if (!ib_dtype_known(dtype)) return IB_E_DTYPE;
  if (T * ld >= (int64_t)1 << 31) return IB_E_UNSUPPORTED;             // offsets inside a window are 32-bit
  if (F * D >= (int64_t)1 << 31) return IB_E_UNSUPPORTED;              // the block index is one 32-bit counter word
  const bool cond = given == 4;
  const SamplerGeom g = ib_sampler_geom(N * W * T * ld, T * ld, x, nullptr, nullptr, x0, z, mask);
  const bool v8 = g.v8 && ld % 8 == 0;
  const bool blk = D % 4 == 0;
  const ResampleArgs p{x, x0, z, mask, coef, obs_coef, timesteps, num_steps, step, step_dev, back, visit, t_out, start, cover,
                       trial_id, (uint32_t)(seed & 0xFFFFFFFFu), (uint32_t)(seed >> 32), N, W, T, F, ld, (int)D};
  const int grid = ib_grid_1d(N * F * ld / (v8 ? 8 : 1), 256);
  return stitch_dispatch<true>(dtype, v8, cond, blk, [&](auto tag, auto width, auto c, auto b) {
    hipLaunchKernelGGL((resample_renoise_kernel<decltype(tag), decltype(width)::value, decltype(c)::value,
                                                decltype(b)::value>), dim3(grid), dim3(256), 0, ib_s(stream), p);
  });
}
