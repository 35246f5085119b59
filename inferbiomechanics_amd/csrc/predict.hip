// What the denoiser predicts -- eps, x0 or v (include/ib_hip_predict.h holds the arithmetic): the loss launch of a training
// step under x0 / v, with the target formed in registers, and the conversion of network outputs into noise predictions that a
// sampling step runs between the forward and the update.  A file of its own: csrc/loss.hip and csrc/loss_weight.hip are
// pinned as they are, and an eps model launches neither kernel.  One form of the arithmetic at every vector width and dtype
// (`fp contract(off)`, every fma spelled), as in csrc/clip.hip.
#include "ib_common.h"
#include "launch.h"
#include "sampler_elem.h"
#include "../../include/ib_hip_lossweight.h"
#include "../../include/ib_hip_predict.h"

namespace {

constexpr int NB = IB_LOSS_LEVEL_BUCKETS;
constexpr int NS = 2 + NB;                  // sums per workgroup, as csrc/loss_weight.hip lays them out: sw, su, sb[0 .. NB)

// csrc/loss_weight.hip's 64-lane sum, operation for operation (that file is pinned, so it cannot lend it): the same adds in the
// same order are what makes kind 0 bitwise the weighted entry
template <int CTRL>
__device__ __forceinline__ float pr_dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float pr_wave_sum(float v) {
#pragma clang fp contract(off)
  v += pr_dpp<0xB1>(v);     // quad_perm [1,0,3,2]
  v += pr_dpp<0x4E>(v);     // quad_perm [2,3,0,1]
  v += pr_dpp<0x141>(v);    // row_half_mirror
  v += pr_dpp<0x140>(v);    // row_mirror
  const int i = __builtin_bit_cast(int, v);
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 0));
  const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 32));
  const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 48));
  return ((r0 + r1) + r2) + r3;
}

// the weighted entry's geometry, through the same host query
int pr_parts(int64_t n) { return (int)(ib_mse_loss_workspace(n) / sizeof(float)); }

__device__ __forceinline__ int pr_level(const int64_t* __restrict__ t, int64_t window, int n_levels) {
  const int64_t v = t[window];
  return v < 0 ? 0 : (v >= n_levels ? n_levels - 1 : (int)v);      // a bad level never becomes an out-of-bounds index
}
__device__ __forceinline__ int pr_band(int level, int n_levels) {
  if (n_levels <= (1 << 28)) return (int)(((uint32_t)level * (uint32_t)NB) / (uint32_t)n_levels);
  return (int)(((int64_t)level * NB) / n_levels);
}
__device__ __forceinline__ int64_t pr_window(int64_t r, int64_t rows, int64_t rows_per_window) {
  if (rows <= 0x7fffffff) return (int64_t)((uint32_t)r / (uint32_t)rows_per_window);
  return r / rows_per_window;
}

// the target of one element: what the network's output is held against
template <int KIND>
__device__ __forceinline__ float pr_target(float a, float s, float x0, float eps) {
#pragma clang fp contract(off)
  if constexpr (KIND == IB_PRED_EPS) return eps;
  else if constexpr (KIND == IB_PRED_X0) return x0;
  else {
    const float p = s * x0;
    return __builtin_fmaf(a, eps, -p);
  }
}

// the noise prediction of one element from the output o and the state x
template <int KIND>
__device__ __forceinline__ float pr_eps(float a, float s, float is, float x, float o) {
#pragma clang fp contract(off)
  if constexpr (KIND == IB_PRED_V) {
    const float p = s * x;
    return __builtin_fmaf(a, o, p);
  } else {
    const float r = __builtin_fmaf(-a, o, x);
    return r * is;
  }
}

template <typename T, int V>
__device__ __forceinline__ void pr_ld(const T* p, float (&v)[V]) {
  if constexpr (V == 1) { v[0] = ib_to_f32(p[0]); }
  else if constexpr (sizeof(T) == 2) {
    const bf16x4_t t = *reinterpret_cast<const bf16x4_t*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (float)t[e];
  } else {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  }
}

// mse_weighted_partial_kernel's body (csrc/loss_weight.hip) with the target made per element and u on the reported sums.  A
// tensor the kind does not read is not loaded: eps streams three tensors, x0 three, v four.
template <typename T, int V, int KIND>
__global__ __launch_bounds__(256) void mse_pred_partial_kernel(const T* __restrict__ pred, int64_t ld_pred,
                                                               const T* __restrict__ x0, const T* __restrict__ eps,
                                                               T* __restrict__ dpred, int64_t ld_dpred,
                                                               const int64_t* __restrict__ t, const float* __restrict__ wtab,
                                                               const float* __restrict__ utab, const float* __restrict__ sqrt_ab,
                                                               const float* __restrict__ sqrt_1mab, int n_levels,
                                                               int64_t rows_per_window, float* __restrict__ partial,
                                                               int64_t rows, int64_t cols, int64_t C, float gscale) {
#pragma clang fp contract(off)
  __shared__ float red[4][NS];
  float sw = 0.f, su = 0.f;
  float sb[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) sb[j] = 0.f;
  const int64_t cv = cols / V;
  const int64_t n = rows * cv;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = n <= 0x7fffffff ? (int64_t)((uint32_t)i / (uint32_t)cv) : i / cv;       // uniform branch
    const int64_t c = (i - r * cv) * V;
    float d[V];
#pragma unroll
    for (int e = 0; e < V; ++e) d[e] = 0.f;
    if (c + V > C) {                                   // at least one free column
      const int level = pr_level(t, pr_window(r, rows, rows_per_window), n_levels);
      const float w = wtab[level], u = utab[level];
      const float a = KIND == IB_PRED_V ? sqrt_ab[level] : 0.f, s = KIND == IB_PRED_V ? sqrt_1mab[level] : 0.f;
      const int k = pr_band(level, n_levels);
      float p[V], z[V], ep[V];
#pragma unroll
      for (int e = 0; e < V; ++e) { z[e] = 0.f; ep[e] = 0.f; }
      pr_ld<T, V>(pred + r * ld_pred + c, p);
      if constexpr (KIND != IB_PRED_EPS) pr_ld<T, V>(x0 + r * cols + c, z);
      if constexpr (KIND != IB_PRED_X0) pr_ld<T, V>(eps + r * cols + c, ep);
      float band = 0.f;
#pragma unroll
      for (int j = 0; j < NB; ++j) band = (k == j) ? sb[j] : band;
#pragma unroll
      for (int e = 0; e < V; ++e)
        if (c + e >= C) {
          const float q = p[e] - pr_target<KIND>(a, s, z[e], ep[e]);
          const float qu = q * u;
          sw = __builtin_fmaf(q * w, q, sw);
          su = __builtin_fmaf(qu, q, su);
          band = __builtin_fmaf(qu, q, band);
          d[e] = (q * gscale) * w;
        }
#pragma unroll
      for (int j = 0; j < NB; ++j) sb[j] = (k == j) ? band : sb[j];
    }
    if (dpred) {
      if constexpr (V == 4) {
        if constexpr (sizeof(T) == 2) {
          bf16x4_t o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = (bf16_t)d[e];
          *reinterpret_cast<bf16x4_t*>(dpred + r * ld_dpred + c) = o;
        } else {
          *reinterpret_cast<float4*>(dpred + r * ld_dpred + c) = make_float4(d[0], d[1], d[2], d[3]);
        }
      } else {
        dpred[r * ld_dpred + c] = ib_from_f32<T>(d[0]);
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  sw = pr_wave_sum(sw);
  su = pr_wave_sum(su);
  if (lane == 0) { red[wave][0] = sw; red[wave][1] = su; }
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const float s = pr_wave_sum(sb[j]);
    if (lane == 0) red[wave][2 + j] = s;
  }
  __syncthreads();
  if (threadIdx.x < NS) {
    const int j = threadIdx.x;
    partial[(int64_t)blockIdx.x * NS + j] = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
  }
}

// one thread per vector of V of the [rows, ld] buffers; rows = B * Tw, row r belongs to window r / Tw
template <typename T, int V, int KIND>
__global__ __launch_bounds__(256) void pred_to_eps_kernel(const T* __restrict__ x, T* __restrict__ out,
                                                          const int64_t* __restrict__ t, const float* __restrict__ sqrt_ab,
                                                          const float* __restrict__ sqrt_1mab,
                                                          const float* __restrict__ inv_sqrt_1mab, int n_levels, int64_t rows,
                                                          int64_t Tw, int64_t D, int64_t ld) {
  const int64_t cv = ld / V, n = rows * cv;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cv, c = (i - r * cv) * V;
    if (c >= D) continue;                                              // a vector of pad columns
    const int level = pr_level(t, r / Tw, n_levels);
    const float a = sqrt_ab[level], s = sqrt_1mab[level], is = inv_sqrt_1mab[level];
    const int64_t off = r * ld + c;
    if constexpr (V == 8) {
      if (c + 8 <= D) {
        float xv[8], o[8];
        ldv<T, 8>(x + off, xv);
        ldv<T, 8>(out + off, o);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = pr_eps<KIND>(a, s, is, xv[j], o[j]);
        stv<T, 8>(out + off, o);
        continue;
      }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if (c + j >= D) break;
      out[off + j] = ib_from_f32<T>(pr_eps<KIND>(a, s, is, ib_to_f32(x[off + j]), ib_to_f32(out[off + j])));
    }
  }
}

}  // namespace

extern "C" int ib_mse_loss_pred_partial(const void* pred, int64_t ld_pred, const void* x0, const void* eps, void* dpred,
                                        int64_t ld_dpred, const int64_t* t, const float* wtab, const float* utab,
                                        const float* sqrt_ab, const float* sqrt_1mab, int n_levels, int64_t rows_per_window,
                                        void* workspace, size_t workspace_bytes, int64_t rows, int64_t cols, int64_t cond_cols,
                                        int kind, int dtype, ib_stream_t stream) {
  if (!pred || !x0 || !eps || !t || !wtab || !utab || !sqrt_ab || !sqrt_1mab) return IB_E_ARG;
  if (rows <= 0 || cols <= 0 || ld_pred < cols || (dpred && ld_dpred < cols)) return IB_E_ARG;
  if (rows_per_window <= 0 || rows % rows_per_window != 0 || n_levels < 1 || cond_cols < 0 || cond_cols >= cols) return IB_E_ARG;
  if (kind != IB_PRED_EPS && kind != IB_PRED_X0 && kind != IB_PRED_V) return IB_E_ARG;
  if (!ib_dtype_known(dtype)) return IB_E_DTYPE;
  const int parts = pr_parts(rows * cols);             // the launch covers every column: the conditioning ones get dpred = 0
  if (!workspace || workspace_bytes < (size_t)parts * NS * sizeof(float)) return IB_E_WORKSPACE;
  float* partial = reinterpret_cast<float*>(workspace);
  const float gscale = 2.f / (float)(rows * (cols - cond_cols));
  const unsigned vb = 4u * (dtype == IB_BF16 ? 2u : 4u);
  const bool v4 = (cols % 4 == 0) && (ld_pred % 4 == 0) && (!dpred || ld_dpred % 4 == 0) && ib_aligned(pred, vb) &&
                  ib_aligned(x0, vb) && ib_aligned(eps, vb) && ib_aligned(dpred, vb);
  auto launch = [&](auto tag, auto width, auto kd) {
    using TY = decltype(tag);
    hipLaunchKernelGGL((mse_pred_partial_kernel<TY, decltype(width)::value, decltype(kd)::value>), dim3(parts), dim3(256), 0,
                       ib_s(stream), (const TY*)pred, ld_pred, (const TY*)x0, (const TY*)eps, (TY*)dpred, ld_dpred, t, wtab, utab,
                       sqrt_ab, sqrt_1mab, n_levels, rows_per_window, partial, rows, cols, cond_cols, gscale);
  };
  return ib_dispatch_dtype_width<4>(dtype, v4, [&](auto tag, auto width) {
    if (kind == IB_PRED_EPS) launch(tag, width, ib_width<IB_PRED_EPS>{});
    else if (kind == IB_PRED_X0) launch(tag, width, ib_width<IB_PRED_X0>{});
    else launch(tag, width, ib_width<IB_PRED_V>{});
  });
}

extern "C" int ib_pred_to_eps(const void* x, void* out, const int64_t* t, const float* sqrt_ab, const float* sqrt_1mab,
                              const float* inv_sqrt_1mab, int n_levels, int kind, int64_t B, int64_t T, int64_t D, int64_t ld,
                              int dtype, ib_stream_t stream) {
  if (!x || !out || !t || !sqrt_ab || !sqrt_1mab || !inv_sqrt_1mab) return IB_E_ARG;
  if (kind != IB_PRED_X0 && kind != IB_PRED_V) return IB_E_ARG;      // eps: the caller launches nothing
  if (n_levels < 1 || B <= 0 || T <= 0 || D <= 0 || ld < D) return IB_E_ARG;
  if (B > (((int64_t)1 << 62) / T) / ld) return IB_E_ARG;
  if (!ib_dtype_known(dtype)) return IB_E_DTYPE;
  const int64_t rows = B * T;
  const bool v8 = ld % 8 == 0 && ib_al16({x, out});                    // every row of either buffer starts 16-byte aligned
  const int grid = ib_grid_1d(rows * ld / (v8 ? 8 : 1), 256);
  return ib_dispatch_dtype_width<8>(dtype, v8, [&](auto tag, auto width) {
    using TY = decltype(tag);
    constexpr int V = decltype(width)::value;
    if (kind == IB_PRED_V)
      hipLaunchKernelGGL((pred_to_eps_kernel<TY, V, IB_PRED_V>), dim3(grid), dim3(256), 0, ib_s(stream), (const TY*)x, (TY*)out,
                         t, sqrt_ab, sqrt_1mab, inv_sqrt_1mab, n_levels, rows, T, D, ld);
    else
      hipLaunchKernelGGL((pred_to_eps_kernel<TY, V, IB_PRED_X0>), dim3(grid), dim3(256), 0, ib_s(stream), (const TY*)x, (TY*)out,
                         t, sqrt_ab, sqrt_1mab, inv_sqrt_1mab, n_levels, rows, T, D, ld);
  });
}
