// [BUILD-DEFINED] classifier-free guidance (include/ib_hip_cfg.h): condition dropout for training and the two launches of
// the guided sampling step's seam.  The null condition is all-zero conditioning columns.  A file of its own: diffusion.hip's
// kernels are pinned bit for bit, so ib_q_sample_cond_drop restates q_sample_cond_kernel's loop here (its free columns go
// through the same q_mix of head_jobs.h under the same width rule, so they agree bit for bit) instead of growing that kernel.
//
// All three are streaming kernels with one thread per vector, no LDS, no atomics; every store is a plain C++ store.
#include <type_traits>

#include "ib_common.h"
#include "head_jobs.h"
#include "launch.h"
#include "philox.h"
#include "sampler_elem.h"
#include "../../include/ib_hip_cfg.h"

namespace {

struct DropArgs {
  uint32_t k0, k1, stream_id; int32_t step; const int32_t* step_dev;
  uint64_t thr;                                          // 0: nothing drops and the generator is not run
  uint8_t* dropped_out;
};

// window b's decision: a function of (seed, step, stream id, b) alone
__device__ __forceinline__ bool cond_dropped(const DropArgs& d, uint32_t step, int64_t b) {
  if (d.thr == 0) return false;
  const U4 w = philox4x32_10(U4{(uint32_t)b, step, d.stream_id, kDomainDrop}, d.k0, d.k1);
  return (uint64_t)w.x < d.thr;
}

// q_sample_cond_kernel (diffusion.hip) with the conditioning columns of a dropped window +0.  Same geometry: V = 4
// consecutive columns per thread or 1; a vector of free columns only never runs the generator; the one vector that
// straddles C chooses per element.  The thread that owns a window's first vector reports the decision.
template <typename T, int V>
__global__ __launch_bounds__(256) void q_sample_cond_drop_kernel(
    const T* __restrict__ x0, const T* __restrict__ eps, const int64_t* __restrict__ t, const float* __restrict__ sqrt_ab,
    const float* __restrict__ sqrt_1mab, T* __restrict__ xt, int64_t ld_xt, int64_t rows, int64_t rows_per_window,
    int64_t cols, int64_t table_rows, int64_t C, DropArgs d) {
  const uint32_t step = (uint32_t)(d.step + (d.step_dev ? *d.step_dev : 0));
  const int64_t cv = cols / V;
  const int64_t n = rows * cv;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cv, c = (i % cv) * V;
    const int64_t b = r / rows_per_window;
    const bool first = c == 0 && r == b * rows_per_window;
    const bool tell = first && d.dropped_out != nullptr;
    bool drop = false;
    if (c < C || tell) drop = cond_dropped(d, step, b);
    if (tell) d.dropped_out[b] = drop ? 1 : 0;
    if constexpr (V == 4) {
      using VT = typename std::conditional<sizeof(T) == 2, bf16x4_t, float4>::type;
      if (c + 4 <= C) {                                // conditioning only
        VT o;
        if (drop) {
          if constexpr (sizeof(T) == 2) {
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = (bf16_t)0.f;
          } else {
            o = make_float4(0.f, 0.f, 0.f, 0.f);
          }
        } else {
          o = *reinterpret_cast<const VT*>(x0 + r * cols + c);
        }
        *reinterpret_cast<VT*>(xt + r * ld_xt + c) = o;
        continue;
      }
      const VT tx = *reinterpret_cast<const VT*>(x0 + r * cols + c);
      int64_t k = t[b];
      k = k < 0 ? 0 : (k >= table_rows ? table_rows - 1 : k);
      const float a = sqrt_ab[k], s = sqrt_1mab[k];
      const VT te = *reinterpret_cast<const VT*>(eps + r * cols + c);
      if constexpr (sizeof(T) == 2) {
        bf16x4_t o;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          o[j] = (c + j < C) ? (drop ? (bf16_t)0.f : tx[j]) : (bf16_t)q_mix<T, 4>(a, (float)tx[j], s, (float)te[j]);
        *reinterpret_cast<bf16x4_t*>(xt + r * ld_xt + c) = o;
      } else {
        const float x[4] = {tx.x, tx.y, tx.z, tx.w}, e[4] = {te.x, te.y, te.z, te.w};
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (c + j < C) ? (drop ? 0.f : x[j]) : q_mix<T, 4>(a, x[j], s, e[j]);
        *reinterpret_cast<float4*>(xt + r * ld_xt + c) = make_float4(o[0], o[1], o[2], o[3]);
      }
    } else {
      if (c < C) { xt[r * ld_xt + c] = drop ? ib_from_f32<T>(0.f) : x0[r * cols + c]; continue; }
      int64_t k = t[b];
      k = k < 0 ? 0 : (k >= table_rows ? table_rows - 1 : k);
      xt[r * ld_xt + c] = ib_from_f32<T>(q_mix<T, 1>(sqrt_ab[k], ib_to_f32(x0[r * cols + c]), sqrt_1mab[k],
                                                     ib_to_f32(eps[r * cols + c])));
    }
  }
}

// g = ec + s (ec - eu) with its three fp32 roundings as written
__device__ __forceinline__ float cfg_mix(float ec, float eu, float s) {
#pragma clang fp contract(off)
  const float d = ec - eu;
  const float q = s * d;
  return ec + q;
}

// eps [2, half]: the first half in place from both; V elements per thread
template <typename T, int V>
__global__ __launch_bounds__(256) void cfg_combine_kernel(T* __restrict__ eps, float s, int64_t half) {
  const int64_t nv = half / V;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
    float ec[V], eu[V], g[V];
    ldv<T, V>(eps + i * V, ec);
    ldv<T, V>(eps + half + i * V, eu);
#pragma unroll
    for (int k = 0; k < V; ++k) g[k] = cfg_mix(ec[k], eu[k], s);
    stv<T, V>(eps + i * V, g);
  }
}

// x [2B, T, ld]: columns C .. D-1 of window b -> window B + b, bits only.  A vector inside [C, D) moves whole; one that
// holds a conditioning or a pad column moves its free elements one by one, so those columns of the second half are never
// written.  Block 0 also copies the timesteps.
template <typename T, int V>
__global__ __launch_bounds__(256) void cfg_mirror_kernel(T* __restrict__ x, int64_t* __restrict__ t, int64_t B, int64_t rows,
                                                         int64_t D, int64_t ld, int64_t C) {
  const int64_t cv = ld / V;
  const int64_t n = rows * cv, half = rows * ld;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cv, c = (i - r * cv) * V;
    if (c + V <= C || c >= D) continue;
    const T* src = x + r * ld + c;
    T* dst = x + half + r * ld + c;
    if constexpr (V == 8) {
      if (c >= C && c + 8 <= D) {
        if constexpr (sizeof(T) == 2) {
          *reinterpret_cast<bf16x8_t*>(dst) = *reinterpret_cast<const bf16x8_t*>(src);
        } else {
          const float4 a = *reinterpret_cast<const float4*>(src), b = *reinterpret_cast<const float4*>(src + 4);
          *reinterpret_cast<float4*>(dst) = a;
          *reinterpret_cast<float4*>(dst + 4) = b;
        }
        continue;
      }
    }
#pragma unroll
    for (int k = 0; k < V; ++k)
      if (c + k >= C && c + k < D) dst[k] = src[k];
  }
  if (blockIdx.x == 0)
    for (int64_t b = threadIdx.x; b < B; b += blockDim.x) t[B + b] = t[b];
}

}  // namespace

extern "C" int ib_q_sample_cond_drop(const void* x0, const void* eps, const int64_t* t, const float* sqrt_ab,
                                     const float* sqrt_1mab, void* x_t, int64_t ld_xt, int64_t B, int64_t T, int64_t D,
                                     int64_t table_rows, int64_t cond_cols, uint64_t seed, int32_t step,
                                     const int32_t* step_dev, uint32_t stream_id, uint64_t drop_threshold,
                                     uint8_t* dropped_out, int dtype, ib_stream_t stream) {
  if (!x0 || !eps || !t || !sqrt_ab || !sqrt_1mab || !x_t || B <= 0 || T <= 0 || D <= 0 || table_rows <= 0 || ld_xt < D)
    return IB_E_ARG;
  if (cond_cols < 0 || cond_cols >= D || drop_threshold > (uint64_t)1 << 32) return IB_E_ARG;
  if (B >= (int64_t)1 << 32) return IB_E_ARG;                          // the window is one 32-bit counter word
  if (!ib_dtype_known(dtype)) return IB_E_DTYPE;
  const bool v4 = ib_q_sample_v4(D, ld_xt, dtype == IB_BF16 ? 2 : 4, x0, eps, x_t);
  const int64_t rows = B * T;
  const int grid = ib_grid_1d(rows * D / (v4 ? 4 : 1), 256);
  const DropArgs d{(uint32_t)(seed & 0xFFFFFFFFu), (uint32_t)(seed >> 32), stream_id, step, step_dev, drop_threshold,
                   dropped_out};
  return ib_dispatch_dtype_width<4>(dtype, v4, [&](auto tag, auto width) {
    using TY = decltype(tag);
    hipLaunchKernelGGL((q_sample_cond_drop_kernel<TY, decltype(width)::value>), dim3(grid), dim3(256), 0, ib_s(stream),
                       (const TY*)x0, (const TY*)eps, t, sqrt_ab, sqrt_1mab, (TY*)x_t, ld_xt, rows, T, D, table_rows,
                       cond_cols, d);
  });
}

extern "C" int ib_cfg_combine(void* eps, float s, int64_t B, int64_t n, int dtype, ib_stream_t stream) {
  if (!eps || B <= 0 || n <= 0) return IB_E_ARG;
  if (!ib_dtype_known(dtype)) return IB_E_DTYPE;
  const int64_t half = B * n;
  const bool v8 = half % 8 == 0 && ib_aligned(eps, 16);                // then the second half starts 16-byte aligned too
  const int grid = ib_grid_1d(half / (v8 ? 8 : 1), 256);
  return ib_dispatch_dtype_width<8>(dtype, v8, [&](auto tag, auto width) {
    using TY = decltype(tag);
    hipLaunchKernelGGL((cfg_combine_kernel<TY, decltype(width)::value>), dim3(grid), dim3(256), 0, ib_s(stream), (TY*)eps, s,
                       half);
  });
}

extern "C" int ib_cfg_mirror(void* x, int64_t* t, int64_t B, int64_t T, int64_t D, int64_t ld, int64_t cond_cols, int dtype,
                             ib_stream_t stream) {
  if (!x || !t || B <= 0 || T <= 0 || D <= 0 || ld < D || cond_cols < 0 || cond_cols >= D) return IB_E_ARG;
  if (!ib_dtype_known(dtype)) return IB_E_DTYPE;
  const int64_t rows = B * T;
  const bool v8 = ld % 8 == 0 && ib_aligned(x, 16);                    // every row of either half starts 16-byte aligned
  const int grid = ib_grid_1d(rows * ld / (v8 ? 8 : 1), 256);
  return ib_dispatch_dtype_width<8>(dtype, v8, [&](auto tag, auto width) {
    using TY = decltype(tag);
    hipLaunchKernelGGL((cfg_mirror_kernel<TY, decltype(width)::value>), dim3(grid), dim3(256), 0, ib_s(stream), (TY*)x, t, B,
                       rows, D, ld, cond_cols);
  });
}
