// The velocity term of the diffusion loss: the squared error of the network's output and the squared error of the frame
// difference of the implied x0, from one pass (include/ib_hip_velocity.h holds the arithmetic, the geometry and the order of
// the sums).  The first loss that couples rows, so not a grid-stride element loop: a thread walks a chunk of a window's frames
// for its columns with every q in registers.  A file of its own: csrc/loss.hip, csrc/loss_weight.hip and csrc/predict.hip are
// pinned as they are, and a trainer without the term launches none of this.  One form of the arithmetic at every vector width
// and dtype (`fp contract(off)`, every fma spelled), as in csrc/predict.hip.
#include <type_traits>

#include "ib_common.h"
#include "launch.h"
#include "../../include/ib_hip_velocity.h"

namespace {

constexpr int NB = IB_LOSS_LEVEL_BUCKETS;
constexpr int NS = 2 + NB;                  // sums per half: {sw, su, sb[0 .. NB)} and {sv, sx, sxb[0 .. NB)}
constexpr int NW = 2 * NS;                  // floats per workgroup
constexpr int FC = IB_VEL_FRAME_CHUNK;
constexpr int NR = IB_VEL_RESULT_LEN;
constexpr int MAX_PARTS = 2048;

// csrc/loss_weight.hip's 64-lane sum (that file is pinned, so it cannot lend it)
template <int CTRL>
__device__ __forceinline__ float vl_dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float vl_wave_sum(float v) {
#pragma clang fp contract(off)
  v += vl_dpp<0xB1>(v);     // quad_perm [1,0,3,2]
  v += vl_dpp<0x4E>(v);     // quad_perm [2,3,0,1]
  v += vl_dpp<0x141>(v);    // row_half_mirror
  v += vl_dpp<0x140>(v);    // row_mirror
  const int i = __builtin_bit_cast(int, v);
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 0));
  const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 32));
  const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 48));
  return ((r0 + r1) + r2) + r3;
}

__device__ __forceinline__ int vl_level(const int64_t* __restrict__ t, int64_t window, int n_levels) {
  const int64_t v = t[window];
  return v < 0 ? 0 : (v >= n_levels ? n_levels - 1 : (int)v);      // a bad level never becomes an out-of-bounds index
}
__device__ __forceinline__ int vl_band(int level, int n_levels) {
  if (n_levels <= (1 << 28)) return (int)(((uint32_t)level * (uint32_t)NB) / (uint32_t)n_levels);
  return (int)(((int64_t)level * NB) / n_levels);
}

// the shape checks both entry points and the workspace query share
bool vl_shape_ok(int64_t rows, int64_t cols, int64_t T) {
  return rows > 0 && cols > 0 && T >= 2 && rows % T == 0 && rows <= ((int64_t)1 << 62) / cols;
}
// workgroups of a launch: one thread per 4-column unit up to MAX_PARTS workgroups, whatever width the launch takes
int vl_parts(int64_t rows, int64_t cols, int64_t T) {
  const int64_t nch = (T + FC - 1) / FC, units = (rows / T) * nch * ((cols + 3) / 4);
  const int64_t g = (units + 255) / 256;
  return (int)(g < 1 ? 1 : (g > MAX_PARTS ? MAX_PARTS : g));
}

// a vector of V elements as it lies in memory: the loads of a chunk are issued in this form and converted at their use
template <typename T, int V> struct VlRaw { using type = T; };
template <> struct VlRaw<float, 4> { using type = float4; };
template <> struct VlRaw<bf16_t, 4> { using type = bf16x4_t; };

template <typename T, int V>
__device__ __forceinline__ float vl_elem(const typename VlRaw<T, V>::type& r, int e) {
  if constexpr (V == 1) return ib_to_f32(r);
  else if constexpr (sizeof(T) == 2) return (float)r[e];
  else return e == 0 ? r.x : (e == 1 ? r.y : (e == 2 ? r.z : r.w));
}

// the target of one element (csrc/predict.hip's pr_target, operation for operation)
template <int KIND>
__device__ __forceinline__ float vl_target(float a, float s, float x0, float eps) {
#pragma clang fp contract(off)
  if constexpr (KIND == IB_PRED_EPS) return eps;
  else if constexpr (KIND == IB_PRED_X0) return x0;
  else {
    const float p = s * x0;
    return __builtin_fmaf(a, eps, -p);
  }
}

template <typename T, int V>
__device__ __forceinline__ void vl_store(T* p, const float (&d)[V]) {
  if constexpr (V == 4) {
    if constexpr (sizeof(T) == 2) {
      bf16x4_t o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (bf16_t)d[e];
      *reinterpret_cast<bf16x4_t*>(p) = o;
    } else {
      *reinterpret_cast<float4*>(p) = make_float4(d[0], d[1], d[2], d[3]);
    }
  } else {
    p[0] = ib_from_f32<T>(d[0]);
  }
}

template <typename T, int V, int KIND>
__global__ __launch_bounds__(256) void vel_partial_kernel(const T* __restrict__ pred, int64_t ld_pred, const T* __restrict__ x0,
                                                          const T* __restrict__ eps, T* __restrict__ dpred, int64_t ld_dpred,
                                                          const int64_t* __restrict__ t, const float* __restrict__ wtab,
                                                          const float* __restrict__ utab, const float* __restrict__ vtab,
                                                          const float* __restrict__ xtab, const float* __restrict__ sqrt_ab,
                                                          const float* __restrict__ sqrt_1mab, int n_levels, int Tw, int nch,
                                                          float* __restrict__ partial, int64_t n_units, int64_t cols, int64_t C,
                                                          float gscale, float vscale) {
#pragma clang fp contract(off)
  using Raw = typename VlRaw<T, V>::type;
  __shared__ float red[4][NW];
  float sw = 0.f, su = 0.f, sv = 0.f, sx = 0.f;
  float sb[NB], sxb[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) { sb[j] = 0.f; sxb[j] = 0.f; }
  const int64_t cv = cols / V;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_units; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t wc, b;
    int ch;
    if (n_units <= 0x7fffffff) {                         // uniform branch: the 32-bit divisions
      const uint32_t q1 = (uint32_t)i / (uint32_t)cv;
      wc = q1;
      b = q1 / (uint32_t)nch;
      ch = (int)(q1 - (uint32_t)b * (uint32_t)nch);
    } else {
      wc = i / cv;
      b = wc / nch;
      ch = (int)(wc - b * nch);
    }
    const int64_t c = (i - wc * cv) * V;
    const int f0 = ch * FC;
    const int nf = Tw - f0 < FC ? Tw - f0 : FC;          // frames this unit owns: f0 .. f0 + nf - 1
    const int64_t row0 = b * Tw;
    if (c + V <= C) {                                    // conditioning columns only: nothing is read
      if (dpred) {
        float z[V];
#pragma unroll
        for (int e = 0; e < V; ++e) z[e] = 0.f;
#pragma unroll
        for (int j = 0; j < FC; ++j)
          if (j < nf) vl_store<T, V>(dpred + (row0 + f0 + j) * ld_dpred + c, z);
      }
      continue;
    }
    const int level = vl_level(t, b, n_levels);
    const float w = wtab[level], u = utab[level], v = vtab[level], x = xtab[level];
    const float a = KIND == IB_PRED_V ? sqrt_ab[level] : 0.f, s = KIND == IB_PRED_V ? sqrt_1mab[level] : 0.f;
    const int k = vl_band(level, n_levels);
    // FC frames and a halo on each side, every load issued before the first use; a frame the window does not have is aimed
    // at the nearest one it has (an address inside the window) and its q is not used below
    Raw rp[FC + 2], rz[FC + 2], re[FC + 2];
#pragma unroll
    for (int j = 0; j < FC + 2; ++j) {
      int fr = f0 - 1 + j;
      fr = fr < 0 ? 0 : (fr > Tw - 1 ? Tw - 1 : fr);
      const int64_t r = row0 + fr;
      rp[j] = *reinterpret_cast<const Raw*>(pred + r * ld_pred + c);
      if constexpr (KIND != IB_PRED_EPS) rz[j] = *reinterpret_cast<const Raw*>(x0 + r * cols + c);
      if constexpr (KIND != IB_PRED_X0) re[j] = *reinterpret_cast<const Raw*>(eps + r * cols + c);
    }
    float q[FC + 2][V];
#pragma unroll
    for (int j = 0; j < FC + 2; ++j)
#pragma unroll
      for (int e = 0; e < V; ++e) {
        float zz = 0.f, ee = 0.f;
        if constexpr (KIND != IB_PRED_EPS) zz = vl_elem<T, V>(rz[j], e);
        if constexpr (KIND != IB_PRED_X0) ee = vl_elem<T, V>(re[j], e);
        q[j][e] =vl_elem<T, V>(rp[j], e) - vl_target<KIND>(a, s, zz, ee);
      }
    float band = 0.f, xband = 0.f;
#pragma unroll
    for (int j = 0; j < NB; ++j) { band = (k == j) ? sb[j] : band; xband = (k == j) ? sxb[j] : xband; }
#pragma unroll
    for (int j = 1; j <= FC; ++j) {
      if (j <= nf) {
        const int f = f0 + j - 1;
        const bool first = f == 0, last = f == Tw - 1;
        float d[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
          d[e] = 0.f;
          if (c + e >= C) {
            const float qf = q[j][e];
            const float dn = last ? 0.f : q[j + 1][e] - qf;
            const float dp = first ? 0.f : qf - q[j - 1][e];
            const float qu = qf * u;
            sw = __builtin_fmaf(qf * w, qf, sw);
            su = __builtin_fmaf(qu, qf, su);
            band = __builtin_fmaf(qu, qf, band);
            if (!last) {
              const float dx = dn * x;
              sv = __builtin_fmaf(dn * v, dn, sv);
              sx = __builtin_fmaf(dx, dn, sx);
              xband = __builtin_fmaf(dx, dn, xband);
            }
            const float dm = (qf * gscale) * w;
            const float dv = ((dp - dn) * vscale) * v;
            d[e] = dm + dv;
          }
        }
        if (dpred) vl_store<T, V>(dpred + (row0 + f) * ld_dpred + c, d);
      }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) { sb[j] = (k == j) ? band : sb[j]; sxb[j] = (k == j) ? xband : sxb[j]; }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  sw = vl_wave_sum(sw);
  su = vl_wave_sum(su);
  sv = vl_wave_sum(sv);
  sx = vl_wave_sum(sx);
  if (lane == 0) { red[wave][0] = sw; red[wave][1] = su; red[wave][NS] = sv; red[wave][NS + 1] = sx; }
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const float s1 = vl_wave_sum(sb[j]), s2 = vl_wave_sum(sxb[j]);
    if (lane == 0) { red[wave][2 + j] = s1; red[wave][NS + 2 + j] = s2; }
  }
  __syncthreads();
  if (threadIdx.x < NW) {
    const int j = threadIdx.x;
    partial[(int64_t)blockIdx.x * NW + j] = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
  }
}

// one workgroup of 256: every column of the partials thread-strided, then the tree (csrc/loss_weight.hip's finalize over
// 4 + 2 NB columns), the windows per band counted in integers; thread 0 writes result and advances accum in index order
__global__ __launch_bounds__(256) void vel_final_kernel(const float* __restrict__ partial, int nparts,
                                                        const int64_t* __restrict__ t, int64_t n_windows, int n_levels,
                                                        float* __restrict__ result, double* __restrict__ accum, float inv_n,
                                                        float inv_nv) {
#pragma clang fp contract(off)
  __shared__ float red[NW][256];
  __shared__ int cnt[NB][256];
  float s[NW];
#pragma unroll
  for (int j = 0; j < NW; ++j) s[j] = 0.f;
  for (int i = threadIdx.x; i < nparts; i += blockDim.x) {
#pragma unroll
    for (int j = 0; j < NW; ++j) s[j] += partial[(int64_t)i * NW + j];
  }
  int nb[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) nb[j] = 0;
  for (int64_t wdw = threadIdx.x; wdw < n_windows; wdw += blockDim.x) {
    const int k = vl_band(vl_level(t, wdw, n_levels), n_levels);
#pragma unroll
    for (int j = 0; j < NB; ++j) nb[j] += (k == j) ? 1 : 0;
  }
#pragma unroll
  for (int j = 0; j < NW; ++j) red[j][threadIdx.x] = s[j];
#pragma unroll
  for (int j = 0; j < NB; ++j) cnt[j][threadIdx.x] = nb[j];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
#pragma unroll
      for (int j = 0; j < NW; ++j) red[j][threadIdx.x] += red[j][threadIdx.x + o];
#pragma unroll
      for (int j = 0; j < NB; ++j) cnt[j][threadIdx.x] += cnt[j][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    float out[NR];
    const float mse = red[0][0] * inv_n, vel = red[NS][0] * inv_nv;
    out[IB_VEL_R_TOTAL] = mse + vel;
    out[IB_VEL_R_EPS] = red[1][0] * inv_n;
    out[IB_VEL_R_MSE] = mse;
    out[IB_VEL_R_VEL] = vel;
    out[IB_VEL_R_X0] = red[NS + 1][0] * inv_nv;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      out[IB_VEL_R_BANDS + j] = red[2 + j][0];
      out[IB_VEL_R_COUNTS + j] = (float)cnt[j][0];
      out[IB_VEL_R_X0_BANDS + j] = red[NS + 2 + j][0];
    }
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      result[j] = out[j];
      if (accum) accum[j] += (double)out[j];
    }
  }
}

}  // namespace

extern "C" int ib_vel_loss_frame_chunk(void) { return FC; }

extern "C" size_t ib_vel_loss_workspace(int64_t rows, int64_t cols, int64_t rows_per_window) {
  return vl_shape_ok(rows, cols, rows_per_window) ? (size_t)vl_parts(rows, cols, rows_per_window) * NW * sizeof(float) : 0;
}

extern "C" int ib_vel_loss_partial(const void* pred, int64_t ld_pred, const void* x0, const void* eps, void* dpred,
                                   int64_t ld_dpred, const int64_t* t, const float* wtab, const float* utab, const float* vtab,
                                   const float* xtab, const float* sqrt_ab, const float* sqrt_1mab, int n_levels,
                                   int64_t rows_per_window, void* workspace, size_t workspace_bytes, int64_t rows, int64_t cols,
                                   int64_t cond_cols, int kind, int dtype, ib_stream_t stream) {
  if (!pred || !x0 || !eps || !t || !wtab || !utab || !vtab || !xtab || !sqrt_ab || !sqrt_1mab) return IB_E_ARG;
  if (rows <= 0 || cols <= 0 || ld_pred < cols || (dpred && ld_dpred < cols)) return IB_E_ARG;
  if (rows_per_window < 2 || rows_per_window > 0x3fffffff || !vl_shape_ok(rows, cols, rows_per_window)) return IB_E_ARG;
  if (n_levels < 1 || cond_cols < 0 || cond_cols >= cols) return IB_E_ARG;
  if (kind != IB_PRED_EPS && kind != IB_PRED_X0 && kind != IB_PRED_V) return IB_E_ARG;
  if (!ib_dtype_known(dtype)) return IB_E_DTYPE;
  const int parts = vl_parts(rows, cols, rows_per_window);
  if (!workspace || workspace_bytes < (size_t)parts * NW * sizeof(float)) return IB_E_WORKSPACE;
  float* partial = reinterpret_cast<float*>(workspace);
  const int Tw = (int)rows_per_window, nch = (Tw + FC - 1) / FC;
  const int64_t B = rows / rows_per_window, scored = cols - cond_cols;
  const float gscale = 2.f / (float)(rows * scored);
  const float vscale = 2.f / (float)((rows - B) * scored);
  const unsigned vb = 4u * (dtype == IB_BF16 ? 2u : 4u);
  const bool v4 = (cols % 4 == 0) && (ld_pred % 4 == 0) && (!dpred || ld_dpred % 4 == 0) && ib_aligned(pred, vb) &&
                  ib_aligned(x0, vb) && ib_aligned(eps, vb) && ib_aligned(dpred, vb);
  const int64_t n_units = B * nch * (cols / (v4 ? 4 : 1));
  auto launch = [&](auto tag, auto width, auto kd) {
    using TY = decltype(tag);
    hipLaunchKernelGGL((vel_partial_kernel<TY, decltype(width)::value, decltype(kd)::value>), dim3(parts), dim3(256), 0,
                       ib_s(stream), (const TY*)pred, ld_pred, (const TY*)x0, (const TY*)eps, (TY*)dpred, ld_dpred, t, wtab, utab,
                       vtab, xtab, sqrt_ab, sqrt_1mab, n_levels, Tw, nch, partial, n_units, cols, cond_cols, gscale, vscale);
  };
  return ib_dispatch_dtype_width<4>(dtype, v4, [&](auto tag, auto width) {
    if (kind == IB_PRED_EPS) launch(tag, width, ib_width<IB_PRED_EPS>{});
    else if (kind == IB_PRED_X0) launch(tag, width, ib_width<IB_PRED_X0>{});
    else launch(tag, width, ib_width<IB_PRED_V>{});
  });
}

extern "C" int ib_vel_loss_finalize(const void* workspace, size_t workspace_bytes, const int64_t* t, int n_levels, float* result,
                                    double* accum, int64_t rows, int64_t cols, int64_t cond_cols, int64_t rows_per_window,
                                    ib_stream_t stream) {
  if (!workspace || !t || !result || n_levels < 1) return IB_E_ARG;
  if (rows_per_window < 2 || !vl_shape_ok(rows, cols, rows_per_window) || cond_cols < 0 || cond_cols >= cols) return IB_E_ARG;
  const int parts = vl_parts(rows, cols, rows_per_window);
  if (workspace_bytes < (size_t)parts * NW * sizeof(float)) return IB_E_WORKSPACE;
  const int64_t B = rows / rows_per_window, scored = cols - cond_cols;
  hipLaunchKernelGGL(vel_final_kernel, dim3(1), dim3(256), 0, ib_s(stream), reinterpret_cast<const float*>(workspace), parts, t,
                     B, n_levels, result, accum, 1.f / (float)(rows * scored), 1.f / (float)((rows - B) * scored));
  IB_CHECK_LAUNCH();
  return IB_OK;
}
