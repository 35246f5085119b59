// [BUILD-DEFINED] the predicted x0 of a sampling step kept inside per-column bounds, and the per-column range of a window
// table (include/ib_hip_clip.h).  The two clip launches stand between the denoiser's forward and the update launch and
// rewrite eps alone, so no update kernel changes.  A file of its own: diffusion.hip's kernels are pinned bit for bit.
//
// New kernels, one form of the arithmetic at every vector width and dtype (clip_x0 / clip_eps below, `fp contract(off)`,
// every fma spelled): tests/clip_restatement.py states the same operations in the same order.  An element whose clipped
// prediction equals its prediction is not stored.  Every store is a plain C++ or vector store; the only atomics are integer
// adds into an LDS histogram, which commute, so the selected order statistic does not depend on arrival order.
#include <type_traits>

#include "ib_common.h"
#include "launch.h"
#include "sampler_elem.h"
#include "../../include/ib_hip_clip.h"

namespace {

struct StepCoef { float ia, sa, a, is; };

// the step row: *step_dev (a device counter: a replayed graph serves every step) or `step`, clamped to the table
__device__ __forceinline__ StepCoef step_coef(const float* __restrict__ coef, int64_t table_rows, int step,
                                              const int32_t* __restrict__ step_dev) {
  int s = step_dev ? *step_dev : step;
  s = s < 0 ? 0 : (s >= table_rows ? (int)table_rows - 1 : s);
  return StepCoef{coef[4 * s], coef[4 * s + 1], coef[4 * s + 2], coef[4 * s + 3]};
}

__device__ __forceinline__ bool finite_f(float v) { return __builtin_fabsf(v) < __builtin_inff(); }
__device__ __forceinline__ bool bounded(float lo, float hi) { return finite_f(lo) && finite_f(hi) && hi > lo; }

// x0 = fma(-sa, e, ia * x): the product rounded, the rest fused
__device__ __forceinline__ float clip_x0(const StepCoef& k, float x, float e) {
#pragma clang fp contract(off)
  const float p = k.ia * x;
  return __builtin_fmaf(-k.sa, e, p);
}

// the noise prediction that reconstructs x0c at this level: (x - a x0c) * is
__device__ __forceinline__ float clip_eps(const StepCoef& k, float x, float x0c) {
#pragma clang fp contract(off)
  const float r = __builtin_fmaf(-k.a, x0c, x);
  return r * k.is;
}

__device__ __forceinline__ float clamp_f(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- 'range': one thread per vector of V; rows = B * T
template <typename T, int V>
__global__ __launch_bounds__(256) void x0_clip_range_kernel(const T* __restrict__ x, T* __restrict__ eps,
                                                            const uint8_t* __restrict__ mask, const float* __restrict__ lo,
                                                            const float* __restrict__ hi, const float* __restrict__ coef,
                                                            int64_t table_rows, int step, const int32_t* __restrict__ step_dev,
                                                            int64_t rows, int64_t Tw, int64_t D, int64_t ld) {
  const StepCoef k = step_coef(coef, table_rows, step, step_dev);
  const int64_t cv = ld / V, n = rows * cv;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cv, c = (i - r * cv) * V;
    if (c >= D) continue;                                              // a vector of pad columns
    const int64_t off = r * ld + c, moff = (r % Tw) * ld + c;
    if constexpr (V == 8) {
      bool whole = c + 8 <= D;                                         // every element free and bounded
      float l[8], h[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool in = c + j < D;
        l[j] = in ? lo[c + j] : 0.f;
        h[j] = in ? hi[c + j] : 0.f;
        whole = whole && bounded(l[j], h[j]) && !(mask && mask[moff + j] != 0);
      }
      if (whole) {
        float a[8], e[8];
        ldv<T, 8>(x + off, a);
        ldv<T, 8>(eps + off, e);
        bool any = false;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float x0 = clip_x0(k, a[j], e[j]);
          const float x0c = clamp_f(x0, l[j], h[j]);
          if (x0c != x0) {
            // the value the dtype keeps, so the vector store below leaves an unchanged element's bits as they are
            e[j] = ib_to_f32(ib_from_f32<T>(clip_eps(k, a[j], x0c)));
            any = true;
          }
        }
        if (any) stv<T, 8>(eps + off, e);                              // e[j] of an unchanged element is its own widened bits
        continue;
      }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if (c + j >= D) break;
      if (mask && mask[moff + j] != 0) continue;
      const float l = lo[c + j], h = hi[c + j];
      if (!bounded(l, h)) continue;
      const float xv = ib_to_f32(x[off + j]);
      const float x0 = clip_x0(k, xv, ib_to_f32(eps[off + j]));
      const float x0c = clamp_f(x0, l, h);
      if (x0c != x0) eps[off + j] = ib_from_f32<T>(clip_eps(k, xv, x0c));
    }
  }
}

// ---- 'dynamic': one workgroup of 256 per window
// rank k (1-based) among the 256 bins of hist: every wave computes the same answer from the same LDS words, so nothing is
// broadcast.  Lane l sums bins 4l .. 4l+3, an inclusive scan over the 64 lanes finds the first lane whose running count
// reaches k, that lane's four bins finish the search.  -> the bin; k becomes the rank inside it.  The bin only ever indexes
// registers and shifts into the prefix, never memory.
__device__ __forceinline__ unsigned select_bin(const unsigned* hist, unsigned& k) {
  const int lane = threadIdx.x & 63;
  const uint4 b = *reinterpret_cast<const uint4*>(hist + 4 * lane);
  const unsigned s = b.x + b.y + b.z + b.w;
  unsigned incl = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  const unsigned total = (unsigned)__shfl((int)incl, 63, 64);
  if (k > total) k = total;                                            // a rank beyond the count is the largest element's
  const unsigned long long reach = __ballot(incl >= k);
  const int src = reach ? __builtin_ctzll(reach) : 63;
  unsigned before = incl - s;                                          // the count in the lanes below
  int sub = 3;
  if (before + b.x >= k) sub = 0;
  else if (before + b.x + b.y >= k) { sub = 1; before += b.x; }
  else if (before + b.x + b.y + b.z >= k) { sub = 2; before += b.x + b.y; }
  else before += b.x + b.y + b.z;
  const unsigned bin = (unsigned)__shfl(4 * lane + sub, src, 64);
  k -= (unsigned)__shfl((int)before, src, 64);
  return bin;
}

struct DynArgs {
  const void* x; void* eps; const uint8_t* mask; const float* lo; const float* hi; const float* coef;
  int64_t table_rows; int step; const int32_t* step_dev;
  const float* m; const float* h; const float* ih;
  unsigned k; int64_t B; int T, D; int64_t ld;
};

template <typename T>
__global__ __launch_bounds__(256) void x0_clip_dynamic_kernel(DynArgs p) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) unsigned hist[256];
  const T* __restrict__ x = (const T*)p.x;
  T* __restrict__ eps = (T*)p.eps;
  const StepCoef sc = step_coef(p.coef, p.table_rows, p.step, p.step_dev);
  const int per = p.T * p.D, tid = threadIdx.x;
  for (int64_t b = blockIdx.x; b < p.B; b += gridDim.x) {
    const int64_t base = b * p.T * p.ld;
    unsigned prefix = 0, decided = 0, k = p.k;
    for (int shift = 24; shift >= 0; shift -= 8) {
      hist[tid] = 0;
      __syncthreads();
      for (int i = tid; i < per; i += 256) {
        const int t = i / p.D, c = i - t * p.D;
        if (p.mask && p.mask[(int64_t)t * p.ld + c] != 0) continue;
        if (!bounded(p.lo[c], p.hi[c])) continue;
        const int64_t off = base + (int64_t)t * p.ld + c;
        const float x0 = clip_x0(sc, ib_to_f32(x[off]), ib_to_f32(eps[off]));
        const float d = x0 - p.m[c];
        const float u = d * p.ih[c];
        const unsigned key = __float_as_uint(__builtin_fabsf(u));    // monotone in |u|; -0 and +0 both key as 0
        if ((key & decided) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
      }
      __syncthreads();
      const unsigned bin = select_bin(hist, k);
      prefix |= bin << shift;
      decided |= 255u << shift;
      __syncthreads();                                                 // every wave has read hist before it is cleared
    }
    const float q = __uint_as_float(prefix);
    const float sw = q > 1.0f ? q : 1.0f;
    for (int i = tid; i < per; i += 256) {
      const int t = i / p.D, c = i - t * p.D;
      if (p.mask && p.mask[(int64_t)t * p.ld + c] != 0) continue;
      if (!bounded(p.lo[c], p.hi[c])) continue;
      const int64_t off = base + (int64_t)t * p.ld + c;
      const float xv = ib_to_f32(x[off]);
      const float x0 = clip_x0(sc, xv, ib_to_f32(eps[off]));
      const float m = p.m[c];
      const float d = x0 - m;
      const float u = d * p.ih[c];
      const float uc = clamp_f(u, -sw, sw) / sw;
      const float x0c = (uc == u) ? x0 : __builtin_fmaf(p.h[c], uc, m);
      if (x0c != x0) eps[off] = ib_from_f32<T>(clip_eps(sc, xv, x0c));
    }
  }
}

// ---- per-column range of a window table.  Stage 1: workgroup g owns logical rows [g * chunk, (g + 1) * chunk) of the
// N * T; the 256 threads are RL row lanes of CW consecutive columns (CW a power of two), so a wave reads consecutive values
template <typename T>
__global__ __launch_bounds__(256) void column_range_partial_kernel(const T* __restrict__ table, int64_t rows, int64_t Tw,
                                                                   int64_t D, int64_t pitch, int64_t chunk, int cw,
                                                                   float* __restrict__ partial) {
  __shared__ float smin[256], smax[256];
  const int tid = threadIdx.x, cl = tid & (cw - 1), rl = tid / cw, RL = 256 / cw;
  const int64_t r0 = (int64_t)blockIdx.x * chunk, r1 = r0 + chunk < rows ? r0 + chunk : rows;
  for (int64_t c0 = 0; c0 < D; c0 += cw) {
    const int64_t c = c0 + cl;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    if (c < D) {
      for (int64_t r = r0 + rl; r < r1; r += RL) {
        const int64_t n = r / Tw, t = r - n * Tw;
        const float v = ib_to_f32(table[n * pitch + t * D + c]);
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
      }
    }
    smin[tid] = mn;
    smax[tid] = mx;
    __syncthreads();
    if (rl == 0 && c < D) {
      for (int j = 1; j < RL; ++j) {
        const float a = smin[j * cw + cl], z = smax[j * cw + cl];
        mn = a < mn ? a : mn;
        mx = z > mx ? z : mx;
      }
      float* o = partial + ((int64_t)blockIdx.x * D + c) * 2;
      o[0] = mn;
      o[1] = mx;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void column_range_final_kernel(const float* __restrict__ partial, int64_t G, int64_t D,
                                                                 float* __restrict__ out) {
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < D; c += (int64_t)gridDim.x * blockDim.x) {
    float mn = __builtin_inff(), mx = -__builtin_inff();
    for (int64_t g = 0; g < G; ++g) {
      const float a = partial[(g * D + c) * 2], z = partial[(g * D + c) * 2 + 1];
      mn = a < mn ? a : mn;
      mx = z > mx ? z : mx;
    }
    out[2 * c] = mn;
    out[2 * c + 1] = mx;
  }
}

static inline bool clip_args_ok(const void* x, const void* eps, const float* lo, const float* hi, const float* coef,
                                int64_t table_rows, int64_t B, int64_t T, int64_t D, int64_t ld) {
  return x && eps && lo && hi && coef && table_rows > 0 && table_rows < ((int64_t)1 << 31) && B > 0 && T > 0 && D > 0 &&
         ld >= D;
}

}  // namespace

extern "C" int ib_x0_clip_range(const void* x, void* eps, const uint8_t* mask, const float* lo, const float* hi,
                                const float* coef, int64_t table_rows, int32_t step, const int32_t* step_dev, int64_t B,
                                int64_t T, int64_t D, int64_t ld, int dtype, ib_stream_t stream) {
  if (!clip_args_ok(x, eps, lo, hi, coef, table_rows, B, T, D, ld)) return IB_E_ARG;
  if (!ib_dtype_known(dtype)) return IB_E_DTYPE;
  const int64_t rows = B * T;
  const bool v8 = ld % 8 == 0 && ib_al16({x, eps});                    // every row of either buffer starts 16-byte aligned
  const int grid = ib_grid_1d(rows * ld / (v8 ? 8 : 1), 256);
  return ib_dispatch_dtype_width<8>(dtype, v8, [&](auto tag, auto width) {
    using TY = decltype(tag);
    hipLaunchKernelGGL((x0_clip_range_kernel<TY, decltype(width)::value>), dim3(grid), dim3(256), 0, ib_s(stream),
                       (const TY*)x, (TY*)eps, mask, lo, hi, coef, table_rows, step, step_dev, rows, T, D, ld);
  });
}

extern "C" int ib_x0_clip_dynamic(const void* x, void* eps, const uint8_t* mask, const float* lo, const float* hi,
                                  const float* coef, int64_t table_rows, int32_t step, const int32_t* step_dev,
                                  const float* m, const float* h, const float* ih, int64_t k, int64_t B, int64_t T, int64_t D,
                                  int64_t ld, int dtype, ib_stream_t stream) {
  if (!clip_args_ok(x, eps, lo, hi, coef, table_rows, B, T, D, ld) || !m || !h || !ih) return IB_E_ARG;
  if (T > ((int64_t)1 << 30) / D) return IB_E_ARG;                     // a window's elements are indexed in 32 bits
  if (k < 1 || k > T * D) return IB_E_ARG;
  if (!ib_dtype_known(dtype)) return IB_E_DTYPE;
  const DynArgs p{x, eps, mask, lo, hi, coef, table_rows, step, step_dev, m, h, ih, (unsigned)k, B, (int)T, (int)D, ld};
  const int grid = (int)(B < 512 ? B : 512);                           // two workgroups per CU, the rest by grid stride
  return ib_dispatch_dtype(dtype, [&](auto tag) {
    using TY = decltype(tag);
    hipLaunchKernelGGL((x0_clip_dynamic_kernel<TY>), dim3(grid), dim3(256), 0, ib_s(stream), p);
  });
}

extern "C" int ib_column_range(const void* table, int64_t N, int64_t T, int64_t D, int64_t pitch, float* partial, int64_t G,
                               float* out, int dtype, ib_stream_t stream) {
  if (!table || !partial || !out || N <= 0 || T <= 0 || D <= 0 || G <= 0 || G >= ((int64_t)1 << 31)) return IB_E_ARG;
  if (T > (((int64_t)1 << 62) / D) || pitch < T * D) return IB_E_ARG;
  if (!ib_dtype_known(dtype)) return IB_E_DTYPE;
  const int64_t rows = N * T, chunk = (rows + G - 1) / G;
  int cw = 1;
  while (cw < 256 && cw < D) cw <<= 1;
  const int rc = ib_dispatch_dtype(dtype, [&](auto tag) {
    using TY = decltype(tag);
    hipLaunchKernelGGL((column_range_partial_kernel<TY>), dim3((unsigned)G), dim3(256), 0, ib_s(stream), (const TY*)table,
                       rows, T, D, pitch, chunk, cw, partial);
  });
  if (rc != IB_OK) return rc;
  hipLaunchKernelGGL(column_range_final_kernel, dim3(ib_grid_1d(D, 256)), dim3(256), 0, ib_s(stream), partial, G, D, out);
  IB_CHECK_LAUNCH();
  return IB_OK;
}
