// [BUILD-DEFINED] diffusion wrapper kernels (no reference counterpart):
// DDPM q_sample, DDIM update (eta = 0, and eta > 0 with the noise term drawn inside the update), the DPM-Solver++(2M) update, table gathers.  The schedule / coefficient / timestep-embedding
// tables are computed in float64 on the host and cast ONCE to fp32 (bit-exactness target of §8c); these
// kernels only index them, so noise-schedule and timestep indexing stay bit-exact.
#include <type_traits>

#include "ib_common.h"
#include "head_jobs.h"
#include "launch.h"
#include "philox.h"
#include "sampler_elem.h"

namespace {

template <typename T>
__global__ void gather_rows_kernel(const float* __restrict__ table, const int64_t* __restrict__ idx, T* __restrict__ out,
                                   int64_t B, int64_t dim, int64_t table_rows) {
  const int64_t n = B * dim;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / dim, d = i % dim;
    int64_t r = idx[b];
    r = r < 0 ? 0 : (r >= table_rows ? table_rows - 1 : r);
    out[i] = ib_from_f32<T>(table[r * dim + d]);
  }
}

// q_mix (one element of q_sample with its roundings spelled out) and the kernel's body live in head_jobs.h: the merged head
// launch of the transformer step (chain.hip: ib_tr_head_prep) runs the same body as a block range of its grid.
template <typename T, int V>
__global__ void q_sample_kernel(const T* __restrict__ x0, const T* __restrict__ eps, const int64_t* __restrict__ t,
                                const float* __restrict__ sqrt_ab, const float* __restrict__ sqrt_1mab, T* __restrict__ xt,
                                int64_t ld_xt, int64_t rows, int64_t rows_per_window, int64_t cols, int64_t table_rows) {
  q_sample_body<T, V>(x0, eps, t, sqrt_ab, sqrt_1mab, xt, ld_xt, rows, rows_per_window, cols, table_rows,
                      (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

// q_sample for a denoiser conditioned on the first C columns of every row (0 < C < cols): those columns reach x_t as they
// are (a copy of x0's bits, no arithmetic), the free columns c >= C are q_sample_kernel's.  Same geometry as that kernel.
// A vector inside the conditioning range moves x0 only (eps is not read); the one vector that straddles C (D = 300,
// C = 270: columns 268 .. 271) loads both and chooses per element.
template <typename T, int V>
__global__ void q_sample_cond_kernel(const T* __restrict__ x0, const T* __restrict__ eps, const int64_t* __restrict__ t,
                                     const float* __restrict__ sqrt_ab, const float* __restrict__ sqrt_1mab,
                                     T* __restrict__ xt, int64_t ld_xt, int64_t rows, int64_t rows_per_window, int64_t cols,
                                     int64_t table_rows, int64_t C) {
  const int64_t cv = cols / V;
  const int64_t n = rows * cv;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cv, c = (i % cv) * V;
    if constexpr (V == 4) {
      using VT = typename std::conditional<sizeof(T) == 2, bf16x4_t, float4>::type;
      const VT tx = *reinterpret_cast<const VT*>(x0 + r * cols + c);
      if (c + 4 <= C) {                                // conditioning only
        *reinterpret_cast<VT*>(xt + r * ld_xt + c) = tx;
        continue;
      }
      int64_t k = t[r / rows_per_window];
      k = k < 0 ? 0 : (k >= table_rows ? table_rows - 1 : k);
      const float a = sqrt_ab[k], s = sqrt_1mab[k];
      const VT te = *reinterpret_cast<const VT*>(eps + r * cols + c);
      if constexpr (sizeof(T) == 2) {
        bf16x4_t o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (c + j < C) ? tx[j] : (bf16_t)q_mix<T, 4>(a, (float)tx[j], s, (float)te[j]);
        *reinterpret_cast<bf16x4_t*>(xt + r * ld_xt + c) = o;
      } else {
        const float x[4] = {tx.x, tx.y, tx.z, tx.w}, e[4] = {te.x, te.y, te.z, te.w};
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (c + j < C) ? x[j] : q_mix<T, 4>(a, x[j], s, e[j]);
        *reinterpret_cast<float4*>(xt + r * ld_xt + c) = make_float4(o[0], o[1], o[2], o[3]);
      }
    } else {
      const T x = x0[r * cols + c];
      if (c < C) { xt[r * ld_xt + c] = x; continue; }
      int64_t k = t[r / rows_per_window];
      k = k < 0 ? 0 : (k >= table_rows ? table_rows - 1 : k);
      xt[r * ld_xt + c] = ib_from_f32<T>(q_mix<T, 1>(sqrt_ab[k], ib_to_f32(x), sqrt_1mab[k], ib_to_f32(eps[r * cols + c])));
    }
  }
}

// ---- the sampler updates.  Every floating-point result below is spelled with its roundings (ddim_mix, obs_pin1 / obs_pin8
// of sampler_elem.h, __builtin_fmaf) under `fp contract(off)`, so no result depends on how the compiler would contract an
// expression in one instantiation or another, and the loops can be shared, moved and inlined freely.

// the step row of a launch: *step_dev (a device counter: a replayed graph serves every step) or `step`, clamped to the table
__device__ __forceinline__ int step_row(int step, const int32_t* step_dev, int64_t num_steps) {
  const int s = step_dev ? *step_dev : step;
  return s < 0 ? 0 : (s >= num_steps ? (int)num_steps - 1 : s);
}

// block 0 hands the next step's timestep to the B windows of the batch (0 after the last step)
__device__ __forceinline__ void put_next_timestep(int64_t* __restrict__ t_out, const int64_t* __restrict__ timesteps,
                                                  int64_t num_steps, int s, int64_t B) {
  if (t_out && blockIdx.x == 0) {
    const int64_t tn = (s + 1 < num_steps) ? timesteps[s + 1] : 0;
    for (int64_t b = threadIdx.x; b < B; b += blockDim.x) t_out[b] = tn;
  }
}

// bit k: element k of the V from offset m0 of the window's mask [T, ld] is observed.  V = 8 reads the 8 bytes at once
template <int V>
__device__ __forceinline__ unsigned mask_bits(const uint8_t* __restrict__ mask, int64_t m0) {
  if constexpr (V == 1) {
    return mask[m0] != 0;
  } else {
    const uint64_t mv = *reinterpret_cast<const uint64_t*>(mask + m0);
    unsigned bits = 0;
#pragma unroll
    for (int k = 0; k < V; ++k) bits |= (((mv >> (8 * k)) & 0xff) != 0 ? 1u : 0u) << k;
    return bits;
  }
}

// ddim_mix of element k of the V from flat offset e0.  mix8: ib_ddim_step would take its 8-wide kernel on these buffers, so
// an element-wise kernel (a window of T * ld % 8 != 0, an operand off 16-byte alignment) rounds as that one does at e0 & 7
template <typename T, int V>
__device__ __forceinline__ float mix_at(int k, int64_t e0, int mix8, float cx, float a, float ce, float e) {
  return (V == 1 && mix8) ? ddim_mix<T, 8>((int)(e0 & 7), cx, a, ce, e) : ddim_mix<T, V>(k, cx, a, ce, e);
}

template <typename T, int V>
__global__ void ddim_step_kernel(T* __restrict__ x, const T* __restrict__ eps, const float* __restrict__ coef,
                                 const int64_t* __restrict__ timesteps, int64_t num_steps, int step,
                                 const int32_t* __restrict__ step_dev, int64_t* __restrict__ t_out, int64_t B, int64_t n) {
#pragma clang fp contract(off)
  const int s = step_row(step, step_dev, num_steps);
  const float cx = coef[2 * s], ce = coef[2 * s + 1];
  const int64_t nv = n / V;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
    float a[V], e[V], o[V];
    ldv<T, V>(x + i * V, a);
    ldv<T, V>(eps + i * V, e);
#pragma unroll
    for (int k = 0; k < V; ++k) o[k] = ddim_mix<T, V>(k, cx, a[k], ce, e[k]);
    stv<T, V>(x + i * V, o);
  }
  put_next_timestep(t_out, timesteps, num_steps, s, B);
}

// ---- the masked (inpainting) updates over the sampler state x [B, T, ld] with one mask [T, ld] for the whole batch.  A free
// element (mask 0) takes the unmasked update (ddim_mix: the same fp32 roundings); an observed one the forward-noised
// observation at the next noise level, obs_coef[s + 1] = (sqrt ab_prev(s), sqrt(1 - ab_prev(s))) times (x0, z) -- (1, 0)
// after the last step, so the loop ends on x0 itself -- pinned by position in a vector of 8 (obs_pin8) or alone (obs_pin1).
// V = 8 loads only what the vector needs: x / eps when one of its elements is free, x0 / z when one is observed.
// The coefficients of one launch: the update's row (cx, ce; DPM: ch, hx, he) and the observation's (ox, oz).
struct MaskedCoef { float cx, ce, ch, hx, he, ox, oz; };

// THE masked loop of the deterministic updates: ddim_cond_step_kernel, the sigma == 0 rows of ddim_cond_step_noise_kernel and
// dpmpp_cond_step_kernel all run it.  INIT: the start state, observed elements <- obs_coef[0] (x0, z), free ones keep the
// drawn noise (eps is not read).  DPM: the vectors that have a free element add the history as dpmpp_step_kernel does;
// SECOND: the row has C != 0 and reads hist.  What hist holds at an observed element is unspecified (a vector of observed
// elements only is not touched; in a mixed vector it gets the expression of the free ones) and no step reads it there.
// i0, stride: the thread's first vector and the grid's step, formed in the kernel (as q_sample_body takes them): blockDim.x
// read inside a device function compiles to a vector load in the prologue, 0.3 us per launch of the start-state kernel.
template <typename T, int V, bool INIT, bool DPM, bool SECOND>
__device__ __forceinline__ void masked_update(T* __restrict__ x, const T* __restrict__ eps, float* hist,
                                              const T* __restrict__ x0, const T* __restrict__ z,
                                              const uint8_t* __restrict__ mask, const MaskedCoef c, int64_t per, int64_t n,
                                              int mix8, int64_t i0, int64_t stride) {
#pragma clang fp contract(off)
  constexpr unsigned ALL = (1u << V) - 1;
  const int64_t nv = n / V;
  for (int64_t i = i0; i < nv; i += stride) {
    const int64_t e0 = i * V;
    const unsigned bits = mask_bits<V>(mask, e0 % per);     // per % V == 0: a vector never straddles two windows
    if (INIT && bits == 0) continue;                        // all free: the drawn noise stays
    float o[V];
    if (bits != ALL) {
      float a[V];
      ldv<T, V>(x + e0, a);
      if constexpr (INIT) {
#pragma unroll
        for (int k = 0; k < V; ++k) o[k] = a[k];
      } else {
        float e[V];
        ldv<T, V>(eps + e0, e);
#pragma unroll
        for (int k = 0; k < V; ++k) o[k] = mix_at<T, V>(k, e0, mix8, c.cx, a[k], c.ce, e[k]);
        if constexpr (DPM) {
          float h[V];
          if constexpr (SECOND) {
            ldv<float, V>(hist + e0, h);
#pragma unroll
            for (int k = 0; k < V; ++k) o[k] = __builtin_fmaf(c.ch, h[k], o[k]);
          }
#pragma unroll
          for (int k = 0; k < V; ++k) h[k] = __builtin_fmaf(c.hx, a[k], c.he * e[k]);
          stv<float, V>(hist + e0, h);
        }
      }
    }
    if (bits != 0) {
      float a[V], b[V];
      ldv<T, V>(x0 + e0, a);
      ldv<T, V>(z + e0, b);
      __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);    // both loads are issued before the first conversion waits for
      __builtin_amdgcn_sched_group_barrier(0x002, 1, 0);    // one (obs_pin8's product of x0 alone at k == 1 drew it forward)
#pragma unroll
      for (int k = 0; k < V; ++k)
        if ((bits >> k) & 1u) o[k] = V == 1 ? obs_pin1(c.ox, a[k], c.oz, b[k]) : obs_pin8(k, c.ox, a[k], c.oz, b[k]);
    }
    stv<T, V>(x + e0, o);
  }
}

template <typename T, int V, bool INIT>
__global__ void ddim_cond_step_kernel(T* __restrict__ x, const T* __restrict__ eps, const T* __restrict__ x0,
                                      const T* __restrict__ z, const uint8_t* __restrict__ mask,
                                      const float* __restrict__ coef, const float* __restrict__ obs_coef,
                                      const int64_t* __restrict__ timesteps, int64_t num_steps, int step,
                                      const int32_t* __restrict__ step_dev, int64_t* __restrict__ t_out, int64_t B,
                                      int64_t per, int64_t n, int mix8) {
  if constexpr (INIT) {
    masked_update<T, V, true, false, false>(x, eps, nullptr, x0, z, mask, {0.f, 0.f, 0.f, 0.f, 0.f, obs_coef[0], obs_coef[1]},
                                            per, n, mix8, (int64_t)blockIdx.x * blockDim.x + threadIdx.x,
                                            (int64_t)gridDim.x * blockDim.x);
  } else {
    const int s = step_row(step, step_dev, num_steps);
    masked_update<T, V, false, false, false>(x, eps, nullptr, x0, z, mask, {coef[2 * s], coef[2 * s + 1], 0.f, 0.f, 0.f,
                                             obs_coef[2 * (s + 1)], obs_coef[2 * (s + 1) + 1]}, per, n, mix8,
                                             (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
    put_next_timestep(t_out, timesteps, num_steps, s, B);
  }
}

// ---- the stochastic update (eta > 0): x' = cx x + ce eps + sigma z', coef rows (cx, ce, sigma), with z' drawn INSIDE the
// update kernel -- no noise buffer in HBM and no launch beside the update.  The normal of element (window, frame f,
// column d) at sampling step s is Box-Muller over Philox4x32-10 (philox.h) at counter ((f * D + d) / 4, s, window id,
// domain 2), key = seed: a function of (seed, window id, s, f, d) alone -- not of the batch position, the batch size, the
// row pitch or the vector width.  Pad columns (d >= D) get no noise.  A step whose sigma is 0 (every row of an eta = 0
// table, the last row of any table) skips the generator and is ib_ddim_step / ib_ddim_cond_step bit for bit.
struct StepNoise {
  uint32_t k0, k1;                  // the seed
  const int64_t* win_id;            // [B] window ids (device: a replayed graph serves new batches)
  int32_t D, ld, per;               // logical columns, row pitch, T * ld
};

// the normals of the V elements from flat offset e0 (a multiple of V) of the state [B, T, ld]; bit k of the result: element
// k is a logical column (a pad column gets 0).  V = 8, BLK (D % 4 == 0 and rows that start on a multiple of 8, or no pitch):
// the vector is two whole Philox blocks, each made once or -- in the pad columns -- not at all.  Otherwise an element looks
// its block up, and neighbours that share a block share the call.  (trial_noise of stitch_step.h is the same draw given
// (row, column); the unpitched 8-wide launch here has a vector straddle two rows and no division to find them with.)
template <int V, bool BLK>
__device__ __forceinline__ unsigned step_noise(const StepNoise& nz, uint32_t s, int64_t e0, float (&z)[V]) {
  const int64_t b = e0 / nz.per;
  const int m0 = (int)(e0 - b * nz.per);
  const uint32_t wid = (uint32_t)nz.win_id[b];
#pragma unroll
  for (int k = 0; k < V; ++k) z[k] = 0.f;
  if constexpr (V == 8 && BLK) {
    int l = m0;
    unsigned ok = 0xffu;
    if (nz.ld != nz.D) {
      const int f = m0 / nz.ld, c = m0 - f * nz.ld;
      l = f * nz.D + c;
      ok = (c + 4 <= nz.D ? 0x0fu : 0u) | (c + 8 <= nz.D ? 0xf0u : 0u);
    }
    const uint32_t q = (uint32_t)l >> 2;
    if (ok & 0x0fu) {
      const U4 w = philox4x32_10(U4{q, s, wid, kDomainStep}, nz.k0, nz.k1);
      box_muller(w.x, w.y, z[0], z[1]); box_muller(w.z, w.w, z[2], z[3]);
    }
    if (ok & 0xf0u) {
      const U4 w = philox4x32_10(U4{q + 1u, s, wid, kDomainStep}, nz.k0, nz.k1);
      box_muller(w.x, w.y, z[4], z[5]); box_muller(w.z, w.w, z[6], z[7]);
    }
    return ok;
  } else {
    unsigned ok = 0;
    uint32_t cur = 0xffffffffu;                  // no block has this index: T * D / 4 < 2^29
    U4 w{};
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const int mm = m0 + k, f = mm / nz.ld, c = mm - f * nz.ld;
      if (c < nz.D) {
        const int l = f * nz.D + c;
        const uint32_t q = (uint32_t)l >> 2;
        if (q != cur) { w = philox4x32_10(U4{q, s, wid, kDomainStep}, nz.k0, nz.k1); cur = q; }
        float za, zb;
        if ((l & 2) == 0) box_muller(w.x, w.y, za, zb); else box_muller(w.z, w.w, za, zb);
        z[k] = (l & 1) ? zb : za;
        ok |= 1u << k;
      }
    }
    return ok;
  }
}

// The noise term is one more fused multiply-add on the ddim_mix value, in every kernel.
template <typename T, int V, bool BLK>
__global__ __launch_bounds__(256) void ddim_step_noise_kernel(T* __restrict__ x, const T* __restrict__ eps,
                                                              const float* __restrict__ coef,
                                                              const int64_t* __restrict__ timesteps, int64_t num_steps,
                                                              int step, const int32_t* __restrict__ step_dev,
                                                              int64_t* __restrict__ t_out, int64_t B, int64_t n, int mix8,
                                                              StepNoise nz) {
#pragma clang fp contract(off)
  const int s = step_row(step, step_dev, num_steps);
  const float cx = coef[3 * s], ce = coef[3 * s + 1], sg = coef[3 * s + 2];
  const bool noisy = sg != 0.f;                                        // uniform over the launch
  const int64_t nv = n / V;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e0 = i * V;
    float a[V], e[V], o[V];
    ldv<T, V>(x + e0, a);
    ldv<T, V>(eps + e0, e);
#pragma unroll
    for (int k = 0; k < V; ++k) o[k] = mix_at<T, V>(k, e0, mix8, cx, a[k], ce, e[k]);
    if (noisy) {
      float z[V];
      const unsigned ok = step_noise<V, BLK>(nz, (uint32_t)s, e0, z);
#pragma unroll
      for (int k = 0; k < V; ++k)
        if ((ok >> k) & 1u) o[k] = __builtin_fmaf(sg, z[k], o[k]);
    }
    stv<T, V>(x + e0, o);
  }
  put_next_timestep(t_out, timesteps, num_steps, s, B);
}

// masked stochastic update.  Free elements: ddim_mix + sigma z'.  Observed elements follow the DDIM posterior given the
// observation: their stored noise z (the buffer, in place) becomes e' = r e + q z' (obs_noise row (r, q), r^2 + q^2 = 1),
// rounded to the state's dtype, and the pinned value is obs_coef[s + 1] (x0, e') over that stored e', so state and buffer
// stay on x = sqrt(ab) x0 + sqrt(1 - ab) e.  Free elements leave z as it is.
template <typename T, int V, bool BLK>
__global__ __launch_bounds__(256) void ddim_cond_step_noise_kernel(T* __restrict__ x, const T* __restrict__ eps,
                                                                   const T* __restrict__ x0, T* z,
                                                                   const uint8_t* __restrict__ mask,
                                                                   const float* __restrict__ coef,
                                                                   const float* __restrict__ obs_coef,
                                                                   const float* __restrict__ obs_noise,
                                                                   const int64_t* __restrict__ timesteps, int64_t num_steps,
                                                                   int step, const int32_t* __restrict__ step_dev,
                                                                   int64_t* __restrict__ t_out, int64_t B, int64_t per,
                                                                   int64_t n, int mix8, StepNoise nz) {
#pragma clang fp contract(off)
  const int s = step_row(step, step_dev, num_steps);
  const float cx = coef[3 * s], ce = coef[3 * s + 1], sg = coef[3 * s + 2];
  const float ox = obs_coef[2 * (s + 1)], oz = obs_coef[2 * (s + 1) + 1];
  if (sg == 0.f) {                                                     // uniform over the launch: ib_ddim_cond_step's loop
    masked_update<T, V, false, false, false>(x, eps, nullptr, x0, z, mask, {cx, ce, 0.f, 0.f, 0.f, ox, oz}, per, n, mix8,
                                             (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
  } else {
    const float r = obs_noise[2 * s], q = obs_noise[2 * s + 1];
    constexpr unsigned ALL = (1u << V) - 1;
    const int64_t nv = n / V;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
      const int64_t e0 = i * V;
      const unsigned bits = mask_bits<V>(mask, e0 % per);
      float zn[V], o[V];
      const unsigned ok = step_noise<V, BLK>(nz, (uint32_t)s, e0, zn);
      if (bits != ALL) {
        float a[V], e[V];
        ldv<T, V>(x + e0, a);
        ldv<T, V>(eps + e0, e);
#pragma unroll
        for (int k = 0; k < V; ++k) {
          o[k] = mix_at<T, V>(k, e0, mix8, cx, a[k], ce, e[k]);
          if ((ok >> k) & 1u) o[k] = __builtin_fmaf(sg, zn[k], o[k]);
        }
      }
      if (bits != 0) {
        float a[V], b[V];
        ldv<T, V>(x0 + e0, a);
        ldv<T, V>(z + e0, b);
#pragma unroll
        for (int k = 0; k < V; ++k)
          if ((bits >> k) & 1u) {
            b[k] = ib_to_f32(ib_from_f32<T>(__builtin_fmaf(r, b[k], q * zn[k])));
            o[k] = __builtin_fmaf(ox, a[k], oz * b[k]);
          }
        stv<T, V>(z + e0, b);                       // a free element of a mixed vector gets back the value it had
      }
      stv<T, V>(x + e0, o);
    }
  }
  put_next_timestep(t_out, timesteps, num_steps, s, B);
}

// ---- DPM-Solver++(2M) update (schedule.dpmpp_coefficients): coef rows (A, E, C, hx, he), x' = A x + E eps + C h_prev, and
// the history the next step reads is h = hx x + he eps, the data prediction at this step's level.  hist is fp32 whatever
// the state's dtype: the update takes the difference of two consecutive data predictions, and rounding each to bf16 would
// be amplified by c = h_i / (2 h_{i-1}).  A x + E eps goes through ddim_mix and C h is one more fused multiply-add on its
// value (as the noise term of ddim_step_noise_kernel is).  A row with C == 0 (the first and the last of every table: no
// history yet, and the step to alpha_bar = 1) does not read hist -- the branch is uniform over the launch -- so its state is
// ib_ddim_step's given (A, E), bit for bit, and an uninitialised history never reaches the state.  Every row writes hist.
template <typename T, int V>
__global__ __launch_bounds__(256) void dpmpp_step_kernel(T* __restrict__ x, const T* __restrict__ eps, float* hist,
                                                         const float* __restrict__ coef,
                                                         const int64_t* __restrict__ timesteps, int64_t num_steps, int step,
                                                         const int32_t* __restrict__ step_dev, int64_t* __restrict__ t_out,
                                                         int64_t B, int64_t n, int mix8) {
#pragma clang fp contract(off)
  const int s = step_row(step, step_dev, num_steps);
  const float cx = coef[5 * s], ce = coef[5 * s + 1], ch = coef[5 * s + 2], hx = coef[5 * s + 3], he = coef[5 * s + 4];
  const bool second = ch != 0.f;                                       // uniform over the launch
  const int64_t nv = n / V;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e0 = i * V;
    float a[V], e[V], o[V], h[V];
    ldv<T, V>(x + e0, a);
    ldv<T, V>(eps + e0, e);
#pragma unroll
    for (int k = 0; k < V; ++k) o[k] = mix_at<T, V>(k, e0, mix8, cx, a[k], ce, e[k]);
    if (second) {
      ldv<float, V>(hist + e0, h);
#pragma unroll
      for (int k = 0; k < V; ++k) o[k] = __builtin_fmaf(ch, h[k], o[k]);
    }
#pragma unroll
    for (int k = 0; k < V; ++k) h[k] = __builtin_fmaf(hx, a[k], he * e[k]);
    stv<float, V>(hist + e0, h);
    stv<T, V>(x + e0, o);
  }
  put_next_timestep(t_out, timesteps, num_steps, s, B);
}

// masked DPM-Solver++(2M) update (masked_update): free elements as dpmpp_step_kernel, observed ones the pinned value of
// ddim_cond_step_kernel, obs_coef[s + 1] (x0, z)
template <typename T, int V>
__global__ __launch_bounds__(256) void dpmpp_cond_step_kernel(T* __restrict__ x, const T* __restrict__ eps, float* hist,
                                                              const T* __restrict__ x0, const T* __restrict__ z,
                                                              const uint8_t* __restrict__ mask,
                                                              const float* __restrict__ coef,
                                                              const float* __restrict__ obs_coef,
                                                              const int64_t* __restrict__ timesteps, int64_t num_steps,
                                                              int step, const int32_t* __restrict__ step_dev,
                                                              int64_t* __restrict__ t_out, int64_t B, int64_t per, int64_t n,
                                                              int mix8) {
  const int s = step_row(step, step_dev, num_steps);
  const MaskedCoef c{coef[5 * s], coef[5 * s + 1], coef[5 * s + 2], coef[5 * s + 3], coef[5 * s + 4],
                     obs_coef[2 * (s + 1)], obs_coef[2 * (s + 1) + 1]};
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  if (c.ch == 0.f)                                                     // uniform over the launch
    masked_update<T, V, false, true, false>(x, eps, hist, x0, z, mask, c, per, n, mix8, i0, stride);
  else
    masked_update<T, V, false, true, true>(x, eps, hist, x0, z, mask, c, per, n, mix8, i0, stride);
  put_next_timestep(t_out, timesteps, num_steps, s, B);
}

// mean and unbiased standard deviation over the K members of an ensemble x [B, K, n], fp32 out.  One lane per (b, j); the
// members are added in the order k = 0 .. K - 1, then the squared deviations from the rounded mean in the same order
// (two passes: the second reads what the first left in cache).  K = 1: std = 0.
template <typename T>
__global__ __launch_bounds__(256) void ensemble_stats_kernel(const T* __restrict__ x, float* __restrict__ mean,
                                                             float* __restrict__ sd, int64_t B, int64_t K, int64_t n) {
#pragma clang fp contract(off)
  const int64_t total = B * n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / n, j = i - b * n;
    const T* p = x + b * K * n + j;
    float sum = 0.f;
    for (int64_t k = 0; k < K; ++k) sum += ib_to_f32(p[k * n]);
    const float m = sum / (float)K;
    float ss = 0.f;
    for (int64_t k = 0; k < K; ++k) {
      const float d = ib_to_f32(p[k * n]) - m;
      ss = __builtin_fmaf(d, d, ss);
    }
    mean[i] = m;
    sd[i] = K > 1 ? __builtin_sqrtf(ss / (float)(K - 1)) : 0.f;
  }
}

__global__ void counter_add_kernel(int32_t* c, int32_t d) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *c += d;
}
__global__ void fill_i64_kernel(int64_t* dst, int64_t v, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] = v;
}

}  // namespace

extern "C" int ib_gather_rows(const float* table, const int64_t* idx, void* out, int64_t B, int64_t dim,
                              int64_t table_rows, int dtype_out, ib_stream_t stream) {
  if (!table || !idx || !out || B <= 0 || dim <= 0 || table_rows <= 0) return IB_E_ARG;
  const int grid = ib_grid_1d(B * dim, 256);
  return ib_dispatch_dtype(dtype_out, [&](auto tag) {
    using TY = decltype(tag);
    hipLaunchKernelGGL((gather_rows_kernel<TY>), dim3(grid), dim3(256), 0, ib_s(stream), table, idx, (TY*)out, B, dim, table_rows);
  });
}

// The launchers below share one shape: the entry point's own argument checks in its own order, the launch geometry from
// launch_geom.h (the width rule is stated there, once), then launch.h's dispatch of dtype (and width) onto the kernel.

extern "C" int ib_q_sample(const void* x0, const void* eps, const int64_t* t, const float* sqrt_ab, const float* sqrt_1mab,
                           void* x_t, int64_t ld_xt, int64_t B, int64_t T, int64_t D, int64_t table_rows, int dtype,
                           ib_stream_t stream) {
  if (!x0 || !eps || !t || !sqrt_ab || !sqrt_1mab || !x_t || B <= 0 || T <= 0 || D <= 0 || table_rows <= 0 || ld_xt < D)
    return IB_E_ARG;
  const bool v4 = ib_q_sample_v4(D, ld_xt, dtype == IB_BF16 ? 2 : 4, x0, eps, x_t);
  const int64_t rows = B * T;
  const int grid = ib_grid_1d(rows * D / (v4 ? 4 : 1), 256);
  return ib_dispatch_dtype_width<4>(dtype, v4, [&](auto tag, auto width) {
    using TY = decltype(tag);
    hipLaunchKernelGGL((q_sample_kernel<TY, decltype(width)::value>), dim3(grid), dim3(256), 0, ib_s(stream), (const TY*)x0, (const TY*)eps, t,
                       sqrt_ab, sqrt_1mab, (TY*)x_t, ld_xt, rows, T, D, table_rows);
  });
}

extern "C" int ib_q_sample_cond(const void* x0, const void* eps, const int64_t* t, const float* sqrt_ab,
                                const float* sqrt_1mab, void* x_t, int64_t ld_xt, int64_t B, int64_t T, int64_t D,
                                int64_t table_rows, int64_t cond_cols, int dtype, ib_stream_t stream) {
  if (cond_cols < 0 || cond_cols >= D) return IB_E_ARG;
  if (cond_cols == 0)                                  // no conditioning columns: ib_q_sample's own launch
    return ib_q_sample(x0, eps, t, sqrt_ab, sqrt_1mab, x_t, ld_xt, B, T, D, table_rows, dtype, stream);
  if (!x0 || !eps || !t || !sqrt_ab || !sqrt_1mab || !x_t || B <= 0 || T <= 0 || D <= 0 || table_rows <= 0 || ld_xt < D)
    return IB_E_ARG;
  const bool v4 = ib_q_sample_v4(D, ld_xt, dtype == IB_BF16 ? 2 : 4, x0, eps, x_t);
  const int64_t rows = B * T;
  const int grid = ib_grid_1d(rows * D / (v4 ? 4 : 1), 256);
  return ib_dispatch_dtype_width<4>(dtype, v4, [&](auto tag, auto width) {
    using TY = decltype(tag);
    hipLaunchKernelGGL((q_sample_cond_kernel<TY, decltype(width)::value>), dim3(grid), dim3(256), 0, ib_s(stream), (const TY*)x0, (const TY*)eps,
                       t, sqrt_ab, sqrt_1mab, (TY*)x_t, ld_xt, rows, T, D, table_rows, cond_cols);
  });
}

extern "C" int ib_ddim_step(void* x, const void* eps, const float* coef, const int64_t* timesteps, int64_t num_steps,
                            int32_t step, const int32_t* step_dev, int64_t* t_out, int64_t B, int64_t n, int dtype,
                            ib_stream_t stream) {
  if (!x || !eps || !coef || num_steps <= 0 || n <= 0) return IB_E_ARG;
  if (t_out && (!timesteps || B <= 0)) return IB_E_ARG;
  const SamplerGeom g = ib_sampler_geom(n, 0, x, eps, nullptr, nullptr, nullptr, nullptr);
  const int grid = ib_grid_1d(n / (g.v8 ? 8 : 1), 256);
  return ib_dispatch_dtype_width<8>(dtype, g.v8, [&](auto tag, auto width) {
    using TY = decltype(tag);
    hipLaunchKernelGGL((ddim_step_kernel<TY, decltype(width)::value>), dim3(grid), dim3(256), 0, ib_s(stream), (TY*)x, (const TY*)eps, coef,
                       timesteps, num_steps, step, step_dev, t_out, B, n);
  });
}

extern "C" int ib_ddim_cond_step(void* x, const void* eps, const void* x0, const void* z, const uint8_t* mask,
                                 const float* coef, const float* obs_coef, const int64_t* timesteps, int64_t num_steps,
                                 int32_t step, const int32_t* step_dev, int64_t* t_out, int64_t B, int64_t T, int64_t D,
                                 int64_t ld, int dtype, ib_stream_t stream) {
  if (!x || !eps || !x0 || !z || !mask || !coef || !obs_coef || num_steps <= 0) return IB_E_ARG;
  if (B <= 0 || T <= 0 || D <= 0 || ld < D) return IB_E_ARG;
  if (t_out && !timesteps) return IB_E_ARG;
  const SamplerGeom g = ib_sampler_geom(B * T * ld, T * ld, x, eps, nullptr, x0, z, mask);
  const int grid = ib_grid_1d(g.n / (g.v8 ? 8 : 1), 256);
  return ib_dispatch_dtype_width<8>(dtype, g.v8, [&](auto tag, auto width) {
    using TY = decltype(tag);
    hipLaunchKernelGGL((ddim_cond_step_kernel<TY, decltype(width)::value, false>), dim3(grid), dim3(256), 0, ib_s(stream), (TY*)x,
                       (const TY*)eps, (const TY*)x0, (const TY*)z, mask, coef, obs_coef, timesteps, num_steps, step, step_dev,
                       t_out, B, g.per, g.n, (int)g.mix8);
  });
}

extern "C" int ib_ddim_cond_init(void* x, const void* x0, const void* z, const uint8_t* mask, const float* obs_coef,
                                 int64_t B, int64_t T, int64_t D, int64_t ld, int dtype, ib_stream_t stream) {
  if (!x || !x0 || !z || !mask || !obs_coef || B <= 0 || T <= 0 || D <= 0 || ld < D) return IB_E_ARG;
  const SamplerGeom g = ib_sampler_geom(B * T * ld, T * ld, x, nullptr, nullptr, x0, z, mask);
  const int grid = ib_grid_1d(g.n / (g.v8 ? 8 : 1), 256);
  return ib_dispatch_dtype_width<8>(dtype, g.v8, [&](auto tag, auto width) {      // no eps, no update: mix8 = 0
    using TY = decltype(tag);
    hipLaunchKernelGGL((ddim_cond_step_kernel<TY, decltype(width)::value, true>), dim3(grid), dim3(256), 0, ib_s(stream), (TY*)x,
                       (const TY*)nullptr, (const TY*)x0, (const TY*)z, mask, (const float*)nullptr, obs_coef,
                       (const int64_t*)nullptr, (int64_t)1, 0, (const int32_t*)nullptr, (int64_t*)nullptr, B, g.per, g.n, 0);
  });
}

// the per-window arguments of the two stochastic updates, checked, and the generator's parameters made of them
namespace {
int step_noise_of(StepNoise& nz, const int64_t* win_id, uint64_t seed, int64_t B, int64_t T, int64_t D, int64_t ld) {
  if (!win_id || B <= 0 || T <= 0 || D <= 0 || ld < D) return IB_E_ARG;
  if (T * ld >= (int64_t)1 << 31) return IB_E_UNSUPPORTED;             // offsets inside a window are 32-bit
  nz = StepNoise{(uint32_t)(seed & 0xFFFFFFFFu), (uint32_t)(seed >> 32), win_id, (int32_t)D, (int32_t)ld, (int32_t)(T * ld)};
  return IB_OK;
}
}  // namespace

extern "C" int ib_ddim_step_noise(void* x, const void* eps, const float* coef, const int64_t* timesteps, int64_t num_steps,
                                  int32_t step, const int32_t* step_dev, int64_t* t_out, const int64_t* win_id,
                                  uint64_t seed, int64_t B, int64_t T, int64_t D, int64_t ld, int dtype, ib_stream_t stream) {
  if (!x || !eps || !coef || num_steps <= 0) return IB_E_ARG;
  if (t_out && !timesteps) return IB_E_ARG;
  if (!ib_dtype_known(dtype)) return IB_E_DTYPE;                       // refused before the window arguments
  StepNoise nz;
  if (const int rc = step_noise_of(nz, win_id, seed, B, T, D, ld)) return rc;
  const SamplerGeom g = ib_sampler_geom(B * T * ld, T * ld, x, eps, nullptr, nullptr, nullptr, nullptr);
  const bool blk = ib_step_noise_blk(D, ld);
  const int grid = ib_grid_1d(g.n / (g.v8 ? 8 : 1), 256);
  return ib_dispatch_dtype(dtype, [&](auto tag) {
    using TY = decltype(tag);
    auto go = [&](auto width, auto whole_blocks) {
      hipLaunchKernelGGL((ddim_step_noise_kernel<TY, decltype(width)::value, decltype(whole_blocks)::value>), dim3(grid),
                         dim3(256), 0, ib_s(stream), (TY*)x, (const TY*)eps, coef, timesteps, num_steps, step, step_dev, t_out, B, g.n,
                         (int)g.mix8, nz);
    };
    if (!g.v8) go(ib_width<1>{}, std::false_type{});
    else if (blk) go(ib_width<8>{}, std::true_type{});
    else go(ib_width<8>{}, std::false_type{});
  });
}

extern "C" int ib_ddim_cond_step_noise(void* x, const void* eps, const void* x0, void* z, const uint8_t* mask,
                                       const float* coef, const float* obs_coef, const float* obs_noise_coef,
                                       const int64_t* timesteps, int64_t num_steps, int32_t step, const int32_t* step_dev,
                                       int64_t* t_out, const int64_t* win_id, uint64_t seed, int64_t B, int64_t T, int64_t D,
                                       int64_t ld, int dtype, ib_stream_t stream) {
  if (!x || !eps || !x0 || !z || !mask || !coef || !obs_coef || !obs_noise_coef || num_steps <= 0) return IB_E_ARG;
  if (t_out && !timesteps) return IB_E_ARG;
  if (!ib_dtype_known(dtype)) return IB_E_DTYPE;                       // refused before the window arguments
  StepNoise nz;
  if (const int rc = step_noise_of(nz, win_id, seed, B, T, D, ld)) return rc;
  const SamplerGeom g = ib_sampler_geom(B * T * ld, T * ld, x, eps, nullptr, x0, z, mask);
  const bool blk = ib_step_noise_blk(D, ld);
  const int grid = ib_grid_1d(g.n / (g.v8 ? 8 : 1), 256);
  return ib_dispatch_dtype(dtype, [&](auto tag) {
    using TY = decltype(tag);
    auto go = [&](auto width, auto whole_blocks) {
      hipLaunchKernelGGL((ddim_cond_step_noise_kernel<TY, decltype(width)::value, decltype(whole_blocks)::value>), dim3(grid),
                         dim3(256), 0, ib_s(stream), (TY*)x, (const TY*)eps, (const TY*)x0, (TY*)z, mask, coef, obs_coef, obs_noise_coef,
                         timesteps, num_steps, step, step_dev, t_out, B, g.per, g.n, (int)g.mix8, nz);
    };
    if (!g.v8) go(ib_width<1>{}, std::false_type{});
    else if (blk) go(ib_width<8>{}, std::true_type{});
    else go(ib_width<8>{}, std::false_type{});
  });
}

extern "C" int ib_dpmpp_step(void* x, const void* eps, float* hist, const float* coef, const int64_t* timesteps,
                             int64_t num_steps, int32_t step, const int32_t* step_dev, int64_t* t_out, int64_t B, int64_t n,
                             int dtype, ib_stream_t stream) {
  if (!x || !eps || !hist || !coef || num_steps <= 0 || n <= 0) return IB_E_ARG;
  if (t_out && (!timesteps || B <= 0)) return IB_E_ARG;
  const SamplerGeom g = ib_sampler_geom(n, 0, x, eps, hist, nullptr, nullptr, nullptr);
  const int grid = ib_grid_1d(n / (g.v8 ? 8 : 1), 256);
  return ib_dispatch_dtype_width<8>(dtype, g.v8, [&](auto tag, auto width) {
    using TY = decltype(tag);
    hipLaunchKernelGGL((dpmpp_step_kernel<TY, decltype(width)::value>), dim3(grid), dim3(256), 0, ib_s(stream), (TY*)x, (const TY*)eps, hist,
                       coef, timesteps, num_steps, step, step_dev, t_out, B, n, (int)g.mix8);
  });
}

extern "C" int ib_dpmpp_cond_step(void* x, const void* eps, float* hist, const void* x0, const void* z, const uint8_t* mask,
                                  const float* coef, const float* obs_coef, const int64_t* timesteps, int64_t num_steps,
                                  int32_t step, const int32_t* step_dev, int64_t* t_out, int64_t B, int64_t T, int64_t D,
                                  int64_t ld, int dtype, ib_stream_t stream) {
  if (!x || !eps || !hist || !x0 || !z || !mask || !coef || !obs_coef || num_steps <= 0) return IB_E_ARG;
  if (B <= 0 || T <= 0 || D <= 0 || ld < D) return IB_E_ARG;
  if (t_out && !timesteps) return IB_E_ARG;
  const SamplerGeom g = ib_sampler_geom(B * T * ld, T * ld, x, eps, hist, x0, z, mask);
  const int grid = ib_grid_1d(g.n / (g.v8 ? 8 : 1), 256);
  return ib_dispatch_dtype_width<8>(dtype, g.v8, [&](auto tag, auto width) {
    using TY = decltype(tag);
    hipLaunchKernelGGL((dpmpp_cond_step_kernel<TY, decltype(width)::value>), dim3(grid), dim3(256), 0, ib_s(stream), (TY*)x, (const TY*)eps,
                       hist, (const TY*)x0, (const TY*)z, mask, coef, obs_coef, timesteps, num_steps, step, step_dev, t_out, B,
                       g.per, g.n, (int)g.mix8);
  });
}

extern "C" int ib_ensemble_stats(const void* x, float* mean, float* std_out, int64_t B, int64_t K, int64_t n, int dtype,
                                 ib_stream_t stream) {
  if (!x || !mean || !std_out || B <= 0 || K <= 0 || n <= 0) return IB_E_ARG;
  const int grid = ib_grid_1d(B * n, 256);
  return ib_dispatch_dtype(dtype, [&](auto tag) {
    using TY = decltype(tag);
    hipLaunchKernelGGL((ensemble_stats_kernel<TY>), dim3(grid), dim3(256), 0, ib_s(stream), (const TY*)x, mean, std_out, B, K, n);
  });
}

extern "C" int ib_counter_add(int32_t* counter, int32_t delta, ib_stream_t stream) {
  if (!counter) return IB_E_ARG;
  hipLaunchKernelGGL(counter_add_kernel, dim3(1), dim3(64), 0, ib_s(stream), counter, delta);
  IB_CHECK_LAUNCH();
  return IB_OK;
}

extern "C" int ib_fill_i64(int64_t* dst, int64_t value, int64_t n, ib_stream_t stream) {
  if (!dst || n <= 0) return IB_E_ARG;
  hipLaunchKernelGGL(fill_i64_kernel, dim3(ib_grid_1d(n, 256)), dim3(256), 0, ib_s(stream), dst, value, n);
  IB_CHECK_LAUNCH();
  return IB_OK;
}

// ---- gradient of a row gather (nn.Embedding backward, TransformerBaseline.py:41-48): dtable[r, :] = sum over the
// positions i with idx[i] == r of dout[i, :], added in position order (deterministic; tables of a few dozen rows)
namespace {
__global__ __launch_bounds__(256) void gather_rows_bwd_kernel(const float* __restrict__ dout, const int64_t* __restrict__ idx,
                                                              float* __restrict__ dtable, int64_t n, int64_t dim,
                                                              int64_t table_rows) {
  const int64_t total = table_rows * dim;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e / dim, d = e % dim;
    float s = 0.f;
    for (int64_t i = 0; i < n; ++i) {
      int64_t k = idx[i];
      k = k < 0 ? 0 : (k >= table_rows ? table_rows - 1 : k);
      if (k == r) s += dout[i * dim + d];
    }
    dtable[e] = s;
  }
}
}  // namespace

extern "C" int ib_gather_rows_bwd(const float* dout, const int64_t* idx, float* dtable, int64_t n, int64_t dim,
                                  int64_t table_rows, ib_stream_t stream) {
  if (!dout || !idx || !dtable || n <= 0 || dim <= 0 || table_rows <= 0) return IB_E_ARG;
  if (n * table_rows * dim > ((int64_t)1 << 32)) return IB_E_UNSUPPORTED;      // meant for per-frame tables
  hipLaunchKernelGGL(gather_rows_bwd_kernel, dim3(ib_grid_1d(table_rows * dim, 256)), dim3(256), 0, ib_s(stream), dout, idx,
                     dtable, n, dim, table_rows);
  IB_CHECK_LAUNCH();
  return IB_OK;
}

// ---- on-device window cache (replaces AddBiomechanicsDataset.__getitem__ `:161-285` + the
// DataLoader collate + the model's torch.concat `FeedForwardRegressionBaseline.py:97-108` for cached windows):
// one packed fp32 row per window = [model input, frame-major F x 147 | labels, key-major: cop F' x 6, force F' x 6,
// torque F' x 6, wrench F' x 12], every block zero-padded to 4 values so each starts on a 16-byte boundary of the row
// ('last_frame' labels: 6 | 6 | 6 | 12 values in 8 | 8 | 8 | 12 slots).  One launch gathers a batch of rows into the model's input tensor (compute dtype) and the
// four contiguous label tensors the loss kernel takes.
namespace {
struct GatherWin {
  const float* table; int64_t row_elems, rows; const int64_t* idx; int64_t B;
  void* x_out; int64_t x_elems, x_pad; int x_bf16;
  float* lab[4]; int64_t lab_elems[4], lab_pad[4];
};
__global__ __launch_bounds__(256) void gather_windows_kernel(GatherWin p) {
  const int64_t per = p.row_elems / 4;                     // float4 pieces per window row (row_elems % 4 == 0)
  const int64_t n = p.B * per;
  const int64_t xq = p.x_pad / 4;
  const bool xvec = (p.x_elems & 3) == 0;               // 1470 inputs per window at the reference defaults: not a multiple of 4
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / per, q = i % per;
    int64_t r = p.idx[b];
    r = r < 0 ? 0 : (r >= p.rows ? p.rows - 1 : r);
    const float4 v = *reinterpret_cast<const float4*>(p.table + r * p.row_elems + 4 * q);
    if (q < xq) {
      if (!xvec) {                       // rows of the model input are then only element-aligned: scalar stores
        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int64_t c = 4 * q + k;
          if (c < p.x_elems) {
            if (p.x_bf16) reinterpret_cast<bf16_t*>(p.x_out)[b * p.x_elems + c] = (bf16_t)e[k];
            else reinterpret_cast<float*>(p.x_out)[b * p.x_elems + c] = e[k];
          }
        }
      } else if (p.x_bf16) {
        bf16x4_t o; o[0] = (bf16_t)v.x; o[1] = (bf16_t)v.y; o[2] = (bf16_t)v.z; o[3] = (bf16_t)v.w;
        *reinterpret_cast<bf16x4_t*>(reinterpret_cast<bf16_t*>(p.x_out) + b * p.x_elems + 4 * q) = o;
      } else {
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.x_out) + b * p.x_elems + 4 * q) = v;
      }
    } else {
      int64_t d = 4 * (q - xq);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (d < p.lab_pad[k]) {
          float* dst = p.lab[k] + b * p.lab_elems[k] + d;
          if (p.lab_elems[k] == p.lab_pad[k]) {
            *reinterpret_cast<float4*>(dst) = v;
          } else {                       // a label block that is not a whole number of 16-byte pieces: element stores
            const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int c = 0; c < 4; ++c)
              if (d + c < p.lab_elems[k]) dst[c] = e[c];
          }
          break;
        }
        d -= p.lab_pad[k];
      }
    }
  }
}
}  // namespace

extern "C" int ib_gather_windows(const float* table, int64_t row_elems, int64_t rows, const int64_t* idx, int64_t B,
                                 void* x_out, int64_t x_elems, int dtype_x, float* const* lab_out,
                                 const int64_t* lab_elems, ib_stream_t stream) {
  if (!table || !idx || !x_out || !lab_out || !lab_elems || rows <= 0 || B <= 0 || x_elems <= 0) return IB_E_ARG;
  if (dtype_x != IB_F32 && dtype_x != IB_BF16) return IB_E_DTYPE;
  const int64_t x_pad = (x_elems + 3) / 4 * 4;             // the input segment of a packed row is padded to 16 bytes
  int64_t total = x_pad;
  GatherWin p{};
  for (int k = 0; k < 4; ++k) {
    if (!lab_out[k] || lab_elems[k] <= 0 || (reinterpret_cast<uintptr_t>(lab_out[k]) % 16)) return IB_E_ARG;
    p.lab[k] = lab_out[k]; p.lab_elems[k] = lab_elems[k]; p.lab_pad[k] = (lab_elems[k] + 3) / 4 * 4;
    total += p.lab_pad[k];
  }
  if (total != row_elems || (reinterpret_cast<uintptr_t>(table) % 16) ||
      (reinterpret_cast<uintptr_t>(x_out) % (dtype_x == IB_BF16 ? 8 : 16)))
    return IB_E_ARG;
  p.table = table; p.row_elems = row_elems; p.rows = rows; p.idx = idx; p.B = B;
  p.x_out = x_out; p.x_elems = x_elems; p.x_pad = x_pad; p.x_bf16 = dtype_x == IB_BF16;
  hipLaunchKernelGGL(gather_windows_kernel, dim3(ib_grid_1d(B * (row_elems / 4), 256)), dim3(256), 0, ib_s(stream), p);
  IB_CHECK_LAUNCH();
  return IB_OK;
}
