// The diffusion loss weighted by noise level, with the unweighted error overall and per band of noise level from the same pass
// (include/ib_hip_lossweight.h holds the arithmetic and the order of the sums).  csrc/loss.hip is untouched: a step without a
// weight launches its kernels as ever.
#include "ib_common.h"
#include "../../include/ib_hip_lossweight.h"

namespace {
// 64-lane sum without the LDS crossbar, as csrc/loss.hip's regression kernel takes it: four DPP adds give every lane its
// 16-lane row total, the four row totals are read out as scalars and added in a fixed order.  Ten butterflies of ds_bpermute
// shuffles at the end of every workgroup were 1.3 of this kernel's 8.8 us at M = 12800, D = 300 (docs/EXPERIMENTS.md).
template <int CTRL>
__device__ __forceinline__ float lw_dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float lw_wave_sum(float v) {
  v += lw_dpp<0xB1>(v);     // quad_perm [1,0,3,2]
  v += lw_dpp<0x4E>(v);     // quad_perm [2,3,0,1]
  v += lw_dpp<0x141>(v);    // row_half_mirror
  v += lw_dpp<0x140>(v);    // row_mirror
  const int i = __builtin_bit_cast(int, v);
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 0));
  const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 32));
  const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 48));
  return ((r0 + r1) + r2) + r3;
}

constexpr int NB = IB_LOSS_LEVEL_BUCKETS;
constexpr int NS = 2 + NB;                  // sums per workgroup: sw, su, sb[0 .. NB)

// the launch geometry of csrc/loss.hip's mse kernels, through its own host query: ib_mse_loss_workspace(n) is one float per
// workgroup of ib_mse_loss_partial (tests/test_loss_weight_plumbing_cpu.py pins the two together)
int lw_parts(int64_t n) { return (int)(ib_mse_loss_workspace(n) / sizeof(float)); }

__device__ __forceinline__ int lw_level(const int64_t* __restrict__ t, int64_t window, int n_levels) {
  const int64_t v = t[window];
  return v < 0 ? 0 : (v >= n_levels ? n_levels - 1 : (int)v);      // a bad level never becomes an out-of-bounds index
}
// level < n_levels: the product fits 32 bits below 2^28 levels, and a 32-bit division is a third of a 64-bit one
__device__ __forceinline__ int lw_band(int level, int n_levels) {
  if (n_levels <= (1 << 28)) return (int)(((uint32_t)level * (uint32_t)NB) / (uint32_t)n_levels);
  return (int)(((int64_t)level * NB) / n_levels);
}
// the window of row r; rows below 2^31 (a branch on a kernel argument) take the 32-bit division
__device__ __forceinline__ int64_t lw_window(int64_t r, int64_t rows, int64_t rows_per_window) {
  if (rows <= 0x7fffffff) return (int64_t)((uint32_t)r / (uint32_t)rows_per_window);
  return r / rows_per_window;
}

// mse_partial_cond_kernel's geometry and vector rule; C = 0 runs the same body.  All V elements of a thread's vector lie in
// one row, hence one window: one level, one weight, one band per trip.  The band accumulators are registers: the band's one is
// selected under compares (constant indices after unrolling), advanced element by element, and put back the same way.
template <typename T, int V>
__global__ __launch_bounds__(256) void mse_weighted_partial_kernel(const T* __restrict__ pred, int64_t ld_pred,
                                                                   const T* __restrict__ target, T* __restrict__ dpred,
                                                                   int64_t ld_dpred, const int64_t* __restrict__ t,
                                                                   const float* __restrict__ wtab, int n_levels,
                                                                   int64_t rows_per_window, float* __restrict__ partial,
                                                                   int64_t rows, int64_t cols, int64_t C, float gscale) {
  __shared__ float red[4][NS];
  float sw = 0.f, su = 0.f;
  float sb[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) sb[j] = 0.f;
  const int64_t cv = cols / V;
  const int64_t n = rows * cv;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = n <= 0x7fffffff ? (int64_t)((uint32_t)i / (uint32_t)cv) : i / cv;       // uniform branch, as above
    const int64_t c = (i - r * cv) * V;
    float d[V];
#pragma unroll
    for (int e = 0; e < V; ++e) d[e] = 0.f;
    if (c + V > C) {                                   // at least one free column
      const int level = lw_level(t, lw_window(r, rows, rows_per_window), n_levels);
      const float w = wtab[level];
      const int k = lw_band(level, n_levels);
      float a[V], b[V];
      if constexpr (V == 4) {
        if constexpr (sizeof(T) == 2) {
          const bf16x4_t ta = *reinterpret_cast<const bf16x4_t*>(pred + r * ld_pred + c), tb = *reinterpret_cast<const bf16x4_t*>(target + r * cols + c);
#pragma unroll
          for (int e = 0; e < 4; ++e) { a[e] = (float)ta[e]; b[e] = (float)tb[e]; }
        } else {
          const float4 ta = *reinterpret_cast<const float4*>(pred + r * ld_pred + c), tb = *reinterpret_cast<const float4*>(target + r * cols + c);
          a[0] = ta.x; a[1] = ta.y; a[2] = ta.z; a[3] = ta.w; b[0] = tb.x; b[1] = tb.y; b[2] = tb.z; b[3] = tb.w;
        }
      } else {
        a[0] = ib_to_f32(pred[r * ld_pred + c]); b[0] = ib_to_f32(target[r * cols + c]);
      }
      float band = 0.f;
#pragma unroll
      for (int j = 0; j < NB; ++j) band = (k == j) ? sb[j] : band;
#pragma unroll
      for (int e = 0; e < V; ++e)
        if (c + e >= C) {
          const float q = a[e] - b[e];
          sw = __builtin_fmaf(q * w, q, sw);
          su = __builtin_fmaf(q, q, su);
          band = __builtin_fmaf(q, q, band);
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
  sw = lw_wave_sum(sw);
  su = lw_wave_sum(su);
  if (lane == 0) { red[wave][0] = sw; red[wave][1] = su; }
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const float s = lw_wave_sum(sb[j]);
    if (lane == 0) red[wave][2 + j] = s;
  }
  __syncthreads();
  if (threadIdx.x < NS) {
    const int j = threadIdx.x;
    partial[(int64_t)blockIdx.x * NS + j] = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
  }
}

// one workgroup of 256: every column of the partials as mse_final_kernel adds its one (thread-strided, then the tree), the
// windows per band counted in integers the same way; thread 0 writes result and advances accum in index order
__global__ __launch_bounds__(256) void mse_weighted_final_kernel(const float* __restrict__ partial, int nparts,
                                                                 const int64_t* __restrict__ t, int64_t n_windows, int n_levels,
                                                                 float* __restrict__ result, double* __restrict__ accum,
                                                                 float inv_n) {
  __shared__ float red[NS][256];
  __shared__ int cnt[NB][256];
  float s[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) s[j] = 0.f;
  for (int i = threadIdx.x; i < nparts; i += blockDim.x) {
#pragma unroll
    for (int j = 0; j < NS; ++j) s[j] += partial[(int64_t)i * NS + j];
  }
  int nb[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) nb[j] = 0;
  for (int64_t wdw = threadIdx.x; wdw < n_windows; wdw += blockDim.x) {
    const int k = lw_band(lw_level(t, wdw, n_levels), n_levels);
#pragma unroll
    for (int j = 0; j < NB; ++j) nb[j] += (k == j) ? 1 : 0;
  }
#pragma unroll
  for (int j = 0; j < NS; ++j) red[j][threadIdx.x] = s[j];
#pragma unroll
  for (int j = 0; j < NB; ++j) cnt[j][threadIdx.x] = nb[j];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
#pragma unroll
      for (int j = 0; j < NS; ++j) red[j][threadIdx.x] += red[j][threadIdx.x + o];
#pragma unroll
      for (int j = 0; j < NB; ++j) cnt[j][threadIdx.x] += cnt[j][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    float out[2 + 2 * NB];
    out[0] = red[0][0] * inv_n;
    out[1] = red[1][0] * inv_n;
#pragma unroll
    for (int j = 0; j < NB; ++j) { out[2 + j] = red[2 + j][0]; out[2 + NB + j] = (float)cnt[j][0]; }
#pragma unroll
    for (int j = 0; j < 2 + 2 * NB; ++j) {
      result[j] = out[j];
      if (accum) accum[j] += (double)out[j];
    }
  }
}

}  // namespace

extern "C" int ib_loss_level_buckets(void) { return NB; }

extern "C" size_t ib_mse_loss_weighted_workspace(int64_t n) {
  return n <= 0 ? 0 : (size_t)lw_parts(n) * NS * sizeof(float);
}

extern "C" int ib_mse_loss_weighted_partial(const void* pred, int64_t ld_pred, const void* target, void* dpred,
                                            int64_t ld_dpred, const int64_t* t, const float* wtab, int n_levels,
                                            int64_t rows_per_window, void* workspace, size_t workspace_bytes, int64_t rows,
                                            int64_t cols, int64_t cond_cols, int dtype, ib_stream_t stream) {
  if (!pred || !target || !t || !wtab || rows <= 0 || cols <= 0 || ld_pred < cols || (dpred && ld_dpred < cols)) return IB_E_ARG;
  if (rows_per_window <= 0 || rows % rows_per_window != 0 || n_levels < 1 || cond_cols < 0 || cond_cols >= cols) return IB_E_ARG;
  if (dtype != IB_F32 && dtype != IB_BF16) return IB_E_DTYPE;
  const int parts = lw_parts(rows * cols);             // the launch covers every column: the conditioning ones get dpred = 0
  if (!workspace || workspace_bytes < (size_t)parts * NS * sizeof(float)) return IB_E_WORKSPACE;
  float* partial = reinterpret_cast<float*>(workspace);
  hipStream_t s = ib_s(stream);
  const float gscale = 2.f / (float)(rows * (cols - cond_cols));
  const int es = dtype == IB_BF16 ? 2 : 4;
  const bool v4 = (cols % 4 == 0) && (ld_pred % 4 == 0) && (!dpred || ld_dpred % 4 == 0) && ib_aligned(pred, 4 * es) &&
                  ib_aligned(target, 4 * es) && ib_aligned(dpred, 4 * es);
#define IB_MSE_WEIGHTED(TY, V)                                                                                                \
  hipLaunchKernelGGL((mse_weighted_partial_kernel<TY, V>), dim3(parts), dim3(256), 0, s, (const TY*)pred, ld_pred,            \
                     (const TY*)target, (TY*)dpred, ld_dpred, t, wtab, n_levels, rows_per_window, partial, rows, cols,        \
                     cond_cols, gscale)
  if (dtype == IB_F32) {
    if (v4) IB_MSE_WEIGHTED(float, 4); else IB_MSE_WEIGHTED(float, 1);
  } else {
    if (v4) IB_MSE_WEIGHTED(bf16_t, 4); else IB_MSE_WEIGHTED(bf16_t, 1);
  }
#undef IB_MSE_WEIGHTED
  IB_CHECK_LAUNCH();
  return IB_OK;
}

extern "C" int ib_mse_loss_weighted_finalize(const void* workspace, size_t workspace_bytes, const int64_t* t,
                                             int64_t n_windows, int n_levels, float* result, double* accum, int64_t n_launch,
                                             int64_t n_mean, ib_stream_t stream) {
  if (!workspace || !t || !result || n_windows < 1 || n_levels < 1 || n_launch <= 0 || n_mean <= 0 || n_mean > n_launch)
    return IB_E_ARG;
  const int parts = lw_parts(n_launch);
  if (workspace_bytes < (size_t)parts * NS * sizeof(float)) return IB_E_WORKSPACE;
  hipLaunchKernelGGL(mse_weighted_final_kernel, dim3(1), dim3(256), 0, ib_s(stream), reinterpret_cast<const float*>(workspace),
                     parts, t, n_windows, n_levels, result, accum, 1.f / (float)n_mean);
  IB_CHECK_LAUNCH();
  return IB_OK;
}
