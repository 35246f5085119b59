// [BUILD-DEFINED] per-column standardisation of the diffusion windows (include/ib_hip_standardize.h): the one-pass fp64
// moments of a window table about a per-column shift, their finalisation into (mean, scale, inv), and the affine map
// between raw and standardised units.  A file of its own: nothing another header pins is touched.
//
// No float atomics: a workgroup's sums go through LDS into its own slot in a fixed order, the slots are summed in order, so
// a result is bit-reproducible run to run.  The affine has one form of the arithmetic at every vector width and dtype pair
// (affine_elem below, `fp contract(off)`, the fma spelled): tests/standardize_restatement.py states the same operations in
// the same order.  Every store is a plain C++ or vector store.
#include <type_traits>

#include "ib_common.h"
#include "launch.h"
#include "sampler_elem.h"
#include "../../include/ib_hip_standardize.h"

namespace {

// ---- moments.  A window is a flat run of L = T * D values from i * pitch; a lane reads VE consecutive values (16 bytes)
// of it at a time.  The column of value e is e % D, so the columns a lane sees repeat when it strides by a PERIOD of
// P = D / gcd(D, VE) vectors: lane slot s of row lane rl takes vector q * P + s of window i for every item (i, q) it
// owns and keeps VE column sums in registers.  P > 256 is covered in passes of SL <= 256 slots.  Items are dealt
// rl-first over the G workgroups by grid stride, four loads in flight per lane (eight measured the same).
template <typename T> struct MomVec;
template <> struct MomVec<bf16_t> { using type = bf16x8_t; static constexpr int VE = 8; };
template <> struct MomVec<float> { using type = f32x4_t; static constexpr int VE = 4; };

struct MomArgs {
  const void* src; const float* shift; double* acc;
  int64_t n, L, D, pitch, nv, Q, items;   // nv vectors per window (the last may be partial), Q periods per window
  int P, SL, RL, M;                        // slots per period, per pass, row lanes, VE / gcd(D, VE)
  int vec, narrow;                         // 16-byte loads allowed; items fit 32 bits
};

template <typename T>
__global__ __launch_bounds__(256) void column_moments_kernel(MomArgs p) {
  using V = typename MomVec<T>::type;
  constexpr int VE = MomVec<T>::VE, U = 4;
  __shared__ double part[256 * VE * 2];
  const T* __restrict__ src = (const T*)p.src;
  const int tid = threadIdx.x, sl = tid % p.SL, rl = tid / p.SL;
  const bool lane_on = rl < p.RL;
  const int64_t stride = (int64_t)gridDim.x * p.RL;
  for (int sb = 0; sb < p.P; sb += p.SL) {
    const int s = sb + sl;
    const bool on = lane_on && s < p.P;
    double sh[VE], s1[VE], s2[VE];
#pragma unroll
    for (int j = 0; j < VE; ++j) {
      sh[j] = on ? (double)p.shift[((int64_t)s * VE + j) % p.D] : 0.0;
      s1[j] = 0.0;
      s2[j] = 0.0;
    }
    if (on) {
      for (int64_t k0 = (int64_t)blockIdx.x * p.RL + rl; k0 < p.items; k0 += U * stride) {
        V raw[U];
        int cnt[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int64_t k = k0 + u * stride;
          cnt[u] = 0;
          if (k >= p.items) continue;
          int64_t i, q;
          if (p.n == 1) {                                               // a dense table: one run, no division
            i = 0;
            q = k;
          } else if (p.narrow) {
            const unsigned ku = (unsigned)k, Qu = (unsigned)p.Q, iu = ku / Qu;
            i = iu;
            q = ku - iu * Qu;
          } else {
            i = k / p.Q;
            q = k - i * p.Q;
          }
          const int64_t v = q * p.P + s;
          if (v >= p.nv) continue;
          const int64_t e0 = v * VE;
          const int64_t left = p.L - e0;                                // >= 1: v < nv
          cnt[u] = left < VE ? (int)left : VE;
          const T* q0 = src + i * p.pitch + e0;
          if (p.vec && cnt[u] == VE) {
            raw[u] = *reinterpret_cast<const V*>(q0);
          } else {
#pragma unroll
            for (int j = 0; j < VE; ++j) raw[u][j] = j < cnt[u] ? q0[j] : T(0.0f);   // nothing behind L is read
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
          for (int j = 0; j < VE; ++j) {
            if (j < cnt[u]) {
              const double d = (double)ib_to_f32(raw[u][j]) - sh[j];
              s1[j] += d;
              s2[j] = __builtin_fma(d, d, s2[j]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < VE; ++j) {
      part[(tid * VE + j) * 2] = s1[j];
      part[(tid * VE + j) * 2 + 1] = s2[j];
    }
    __syncthreads();
    // column c sits at values c + m * D, m < M, of a period: slot e / VE, element e % VE; row lanes in order
    const int sl_n = p.P - sb < p.SL ? p.P - sb : p.SL;
    for (int64_t c = tid; c < p.D; c += 256) {
      double a1 = 0.0, a2 = 0.0;
      for (int m = 0; m < p.M; ++m) {
        const int64_t e = c + (int64_t)m * p.D;
        const int64_t so = e / VE - sb;
        const int j = (int)(e % VE);
        if (so < 0 || so >= sl_n) continue;
        for (int r = 0; r < p.RL; ++r) {
          const int t = r * p.SL + (int)so;
          a1 += part[(t * VE + j) * 2];
          a2 += part[(t * VE + j) * 2 + 1];
        }
      }
      double* o = p.acc + ((int64_t)blockIdx.x * p.D + c) * 2;         // (g, c) belongs to this thread alone, in every pass
      o[0] += a1;
      o[1] += a2;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void column_moments_finalize_kernel(const double* __restrict__ acc, int64_t G, int64_t D,
                                                                      double count, const float* __restrict__ shift,
                                                                      float min_std, float* __restrict__ mean,
                                                                      float* __restrict__ scale, float* __restrict__ inv) {
#pragma clang fp contract(off)
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < D; c += (int64_t)gridDim.x * blockDim.x) {
    double S1 = 0.0, S2 = 0.0;
    for (int64_t g = 0; g < G; ++g) {
      S1 += acc[(g * D + c) * 2];
      S2 += acc[(g * D + c) * 2 + 1];
    }
    const double md = S1 / count;
    double var = S2 / count - md * md;
    var = var > 0.0 ? var : 0.0;                                       // a NaN sum stays out of sqrt as 0: scale 1
    mean[c] = (float)((double)shift[c] + md);
    const float s = (float)__builtin_sqrt(var);
    const float sc = s > min_std ? s : 1.0f;
    scale[c] = sc;
    inv[c] = (float)(1.0 / (double)sc);
  }
}

// ---- affine.  mode 0: (x - a) * b, two roundings; mode 1: fma(x, b, a), or x * b without a
__device__ __forceinline__ float affine_elem(int mode, bool has_a, float x, float a, float b) {
#pragma clang fp contract(off)
  if (mode == 0) {
    const float d = x - a;
    return d * b;
  }
  return has_a ? __builtin_fmaf(x, b, a) : x * b;
}

struct AffArgs {
  const void* src; void* dst; const float* a; const float* b;
  int64_t src_win, src_row, dst_win, dst_row, T, c0, per, total;      // per vectors in a row's window, total in all
  int mode, narrow;
};

template <typename TS, typename TD, int V>
__global__ __launch_bounds__(256) void column_affine_kernel(AffArgs p) {
  const TS* src = (const TS*)p.src;                                    // no __restrict__: src may be dst
  TD* dst = (TD*)p.dst;
  const bool has_a = p.a != nullptr;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.total; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t r, cv, n, t;
    if (p.narrow) {
      const unsigned iu = (unsigned)i, pu = (unsigned)p.per, ru = iu / pu, nu = ru / (unsigned)p.T;
      r = ru; cv = iu - ru * pu; n = nu; t = ru - nu * (unsigned)p.T;
    } else {
      r = i / p.per; cv = i - r * p.per; n = r / p.T; t = r - n * p.T;
    }
    const int64_t c = p.c0 + cv * V;
    float x[V], y[V];
    ldv<TS, V>(src + n * p.src_win + t * p.src_row + c, x);
#pragma unroll
    for (int j = 0; j < V; ++j) y[j] = affine_elem(p.mode, has_a, x[j], has_a ? p.a[c + j] : 0.f, p.b[c + j]);
    stv<TD, V>(dst + n * p.dst_win + t * p.dst_row + c, y);
  }
}

// Whole rows (c0 = 0, w = row on both sides) make a window one flat run of L = T * w values, and dense windows make the
// table one run of N * L: a lane takes 8 consecutive values of a run whatever w is, the column of value e being e % w.  The
// coefficients sit in LDS, extended by 8 columns so that a vector which wraps into the next row reads on.  The last chunk
// of a run (L % 8 values) goes element by element.  The same affine_elem: the same bits as the row kernel.
constexpr int RUN_WMAX = 2048;

struct RunArgs {
  const void* src; void* dst; const float* a; const float* b;
  int64_t src_win, dst_win, L, nv, total;                              // nv chunks per run, total in all
  int w, runs1, mode;
};

template <typename TS, typename TD>
__global__ __launch_bounds__(256) void column_affine_run_kernel(RunArgs p) {
  __shared__ float sa[RUN_WMAX + 8], sb[RUN_WMAX + 8];
  const TS* src = (const TS*)p.src;                                    // no __restrict__: src may be dst
  TD* dst = (TD*)p.dst;
  const bool has_a = p.a != nullptr;
  for (int c = threadIdx.x; c < p.w + 8; c += 256) {
    sa[c] = has_a ? p.a[c % p.w] : 0.f;
    sb[c] = p.b[c % p.w];
  }
  __syncthreads();
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int col = (int)((first * 8) % p.w);                                  // one run: the column advances by a fixed stride
  const int dcol = (int)((step * 8) % p.w);
  for (int64_t i = first; i < p.total; i += step) {
    int64_t run = 0, v = i;
    if (!p.runs1) {                                                    // total and L fit 32 bits (the launcher's test)
      const unsigned iu = (unsigned)i, nu = (unsigned)p.nv, ru = iu / nu, vu = iu - ru * nu;
      run = ru;
      v = vu;
      col = (int)((vu * 8u) % (unsigned)p.w);
    }
    const int64_t e0 = v * 8, left = p.L - e0;
    const TS* s = src + run * p.src_win + e0;
    TD* d = dst + run * p.dst_win + e0;
    if (left >= 8) {
      float x[8], y[8];
      ldv<TS, 8>(s, x);
#pragma unroll
      for (int j = 0; j < 8; ++j) y[j] = affine_elem(p.mode, has_a, x[j], sa[col + j], sb[col + j]);
      stv<TD, 8>(d, y);
    } else {
      for (int j = 0; j < (int)left; ++j)
        d[j] = ib_from_f32<TD>(affine_elem(p.mode, has_a, ib_to_f32(s[j]), sa[col + j], sb[col + j]));
    }
    col += dcol;
    col = col >= p.w ? col - p.w : col;
  }
}

template <typename TS, typename TD>
static inline void launch_affine_run(int grid, hipStream_t s, const RunArgs& p) {
  hipLaunchKernelGGL((column_affine_run_kernel<TS, TD>), dim3(grid), dim3(256), 0, s, p);
}

template <typename TS, typename TD>
static inline void launch_affine(bool v8, int grid, hipStream_t s, const AffArgs& p) {
  if (v8) hipLaunchKernelGGL((column_affine_kernel<TS, TD, 8>), dim3(grid), dim3(256), 0, s, p);
  else hipLaunchKernelGGL((column_affine_kernel<TS, TD, 1>), dim3(grid), dim3(256), 0, s, p);
}

static inline int64_t gcd64(int64_t a, int64_t b) {
  while (b) { const int64_t t = a % b; a = b; b = t; }
  return a;
}

static inline bool mul_fits(int64_t a, int64_t b) { return a <= (((int64_t)1 << 62) / b); }   // a, b > 0

}  // namespace

extern "C" int ib_column_moments_accum(const void* src, int64_t n, int64_t T, int64_t D, int64_t pitch, const float* shift,
                                       double* acc, int64_t G, int dtype, ib_stream_t stream) {
  if (!src || !shift || !acc || n <= 0 || T <= 0 || D <= 0 || G <= 0 || G > 65535) return IB_E_ARG;
  if (!mul_fits(T, D) || pitch < T * D || !mul_fits(n, pitch)) return IB_E_ARG;
  if (!ib_dtype_known(dtype)) return IB_E_DTYPE;
  const int VE = dtype == IB_BF16 ? 8 : 4;
  MomArgs p;
  p.src = src; p.shift = shift; p.acc = acc;
  p.n = n; p.L = T * D; p.D = D; p.pitch = pitch;
  if (pitch == p.L) {                                                  // a dense table is one run: no partial vector per window
    if (!mul_fits(n, p.L)) return IB_E_ARG;
    p.L = n * p.L;
    p.n = 1;
  }
  const int64_t g = gcd64(D, VE), P = D / g;
  if (P >= ((int64_t)1 << 30)) return IB_E_ARG;
  const int64_t passes = (P + 255) / 256;
  p.P = (int)P;
  p.SL = (int)((P + passes - 1) / passes);
  p.RL = 256 / p.SL;
  p.M = (int)(VE / g);
  p.nv = (p.L + VE - 1) / VE;
  p.Q = (p.nv + P - 1) / P;
  if (!mul_fits(p.n, p.Q)) return IB_E_ARG;
  p.items = p.n * p.Q;
  p.narrow = p.items < ((int64_t)1 << 32) && p.Q < ((int64_t)1 << 32);
  p.vec = ib_aligned(src, 16) && (p.n == 1 || pitch % VE == 0);
  return ib_dispatch_dtype(dtype, [&](auto tag) {
    using TY = decltype(tag);
    hipLaunchKernelGGL((column_moments_kernel<TY>), dim3((unsigned)G), dim3(256), 0, ib_s(stream), p);
  });
}

extern "C" int ib_column_moments_finalize(const double* acc, int64_t G, int64_t D, int64_t count, const float* shift,
                                          float min_std, float* mean, float* scale, float* inv, ib_stream_t stream) {
  if (!acc || !shift || !mean || !scale || !inv || G <= 0 || G > 65535 || D <= 0 || count <= 0) return IB_E_ARG;
  if (!(min_std >= 0.0f)) return IB_E_ARG;
  hipLaunchKernelGGL(column_moments_finalize_kernel, dim3(ib_grid_1d(D, 256)), dim3(256), 0, ib_s(stream), acc, G, D,
                     (double)count, shift, min_std, mean, scale, inv);
  IB_CHECK_LAUNCH();
  return IB_OK;
}

extern "C" int ib_column_affine(const void* src, int src_dtype, int64_t src_win, int64_t src_row, void* dst, int dst_dtype,
                                int64_t dst_win, int64_t dst_row, const float* a, const float* b, int64_t N, int64_t T,
                                int64_t c0, int64_t w, int mode, ib_stream_t stream) {
  if (!src || !dst || !b || N <= 0 || T <= 0 || c0 < 0 || w <= 0 || (mode != 0 && mode != 1)) return IB_E_ARG;
  if (mode == 0 && !a) return IB_E_ARG;
  if (c0 > ((int64_t)1 << 40) || w > ((int64_t)1 << 40)) return IB_E_ARG;
  const int64_t end = c0 + w;
  for (const int64_t* g : {&src_row, &dst_row})
    if (*g < end || !mul_fits(T, *g)) return IB_E_ARG;
  if (src_win < (T - 1) * src_row + end || dst_win < (T - 1) * dst_row + end) return IB_E_ARG;
  if (!mul_fits(N, src_win) || !mul_fits(N, dst_win) || !mul_fits(N, T) || !mul_fits(N * T, w)) return IB_E_ARG;
  if (!ib_dtype_known(src_dtype) || !ib_dtype_known(dst_dtype)) return IB_E_DTYPE;
  if (src == dst && (src_dtype != dst_dtype || src_win != dst_win || src_row != dst_row)) return IB_E_ARG;
  const unsigned sb = src_dtype == IB_BF16 ? 16u : 32u, db = dst_dtype == IB_BF16 ? 16u : 32u;
  const bool v8 = c0 % 8 == 0 && w % 8 == 0 && src_win % 8 == 0 && src_row % 8 == 0 && dst_win % 8 == 0 && dst_row % 8 == 0 &&
                  ib_aligned(src, sb) && ib_aligned(dst, db);
  hipStream_t s = ib_s(stream);
  // whole dense rows: flat runs (column_affine_run_kernel)
  if (c0 == 0 && src_row == w && dst_row == w && w <= RUN_WMAX && ib_aligned(src, sb) && ib_aligned(dst, db)) {
    const bool one = src_win == T * w && dst_win == T * w;             // dense windows too: one run
    RunArgs r;
    r.src = src; r.dst = dst; r.a = a; r.b = b;
    r.src_win = src_win; r.dst_win = dst_win;
    r.L = one ? N * T * w : T * w;
    r.nv = (r.L + 7) / 8;
    r.total = one ? r.nv : N * r.nv;
    r.w = (int)w; r.runs1 = one; r.mode = mode;
    const bool fits = r.total < ((int64_t)1 << 32) && r.L < ((int64_t)1 << 32);
    if (one || (src_win % 8 == 0 && dst_win % 8 == 0 && fits)) {
      const int grid = ib_grid_1d(r.total, 256, 256 * 8);
      if (src_dtype == IB_F32 && dst_dtype == IB_F32) launch_affine_run<float, float>(grid, s, r);
      else if (src_dtype == IB_F32) launch_affine_run<float, bf16_t>(grid, s, r);
      else if (dst_dtype == IB_F32) launch_affine_run<bf16_t, float>(grid, s, r);
      else launch_affine_run<bf16_t, bf16_t>(grid, s, r);
      IB_CHECK_LAUNCH();
      return IB_OK;
    }
  }
  AffArgs p;
  p.src = src; p.dst = dst; p.a = a; p.b = b;
  p.src_win = src_win; p.src_row = src_row; p.dst_win = dst_win; p.dst_row = dst_row;
  p.T = T; p.c0 = c0; p.per = w / (v8 ? 8 : 1); p.total = N * T * p.per;
  p.mode = mode;
  p.narrow = p.total < ((int64_t)1 << 32) && T < ((int64_t)1 << 32);
  const int grid = ib_grid_1d(p.total, 256, 256 * 16);
  if (src_dtype == IB_F32 && dst_dtype == IB_F32) launch_affine<float, float>(v8, grid, s, p);
  else if (src_dtype == IB_F32) launch_affine<float, bf16_t>(v8, grid, s, p);
  else if (dst_dtype == IB_F32) launch_affine<bf16_t, float>(v8, grid, s, p);
  else launch_affine<bf16_t, bf16_t>(v8, grid, s, p);
  IB_CHECK_LAUNCH();
  return IB_OK;
}
