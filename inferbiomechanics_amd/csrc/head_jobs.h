// Bodies of the small launches at the head of a training step, as __device__ functions: each stand-alone kernel
// (q_sample_kernel, cast2d_kernel, tiny_matmul_kernel<false>, transpose_multi_kernel) and the merged launches that run
// several of them as block ranges of ONE grid (chain.hip: ib_tr_head_prep; ffn_chain.hip: ib_ffn_chain_pack_ex) call the
// SAME code, so no arithmetic is written twice and the merged launches are bit-identical by construction.
// The element-wise bodies are grid-stride loops over a virtual thread index: `first` = this thread's index among the
// job's threads, `stride` = the job's thread count (a stand-alone kernel passes its whole grid, a merged launch the block
// range the job owns).  Every element is computed by exactly one thread from its own operands alone, so the result does
// not depend on the geometry.
#pragma once
#include "ib_common.h"

// One element of q_sample, a * x + s * e, with its fp32 roundings spelled out.  q_sample_kernel and the free columns of
// q_sample_cond_kernel both go through it, so the two agree bit for bit however the compiler would contract the bare
// expression in either kernel.  The forms are those that expression compiled to in q_sample_kernel<T, V> for gfx950 (its
// ISA is unchanged by the helper): the lone fp32 element sums two rounded products; every other form fuses a * x into the
// rounded s * e.
template <typename T, int V>
__device__ __forceinline__ float q_mix(float a, float x, float s, float e) {
#pragma clang fp contract(off)
  if constexpr (V == 1 && sizeof(T) == 4) return a * x + s * e;
  else return __builtin_fmaf(a, x, s * e);
}

// rows = B*T tokens, cols = D features; V = 4: 4 consecutive columns per thread (8 B bf16 / 16 B fp32).  x_t may have a
// padded leading dimension (the trainer keeps D = 300 activations at ld = 304 so every row starts 16-byte aligned).
template <typename T, int V>
__device__ __forceinline__ void q_sample_body(const T* __restrict__ x0, const T* __restrict__ eps,
                                              const int64_t* __restrict__ t, const float* __restrict__ sqrt_ab,
                                              const float* __restrict__ sqrt_1mab, T* __restrict__ xt, int64_t ld_xt,
                                              int64_t rows, int64_t rows_per_window, int64_t cols, int64_t table_rows,
                                              int64_t first, int64_t stride) {
  const int64_t cv = cols / V;
  const int64_t n = rows * cv;
  for (int64_t i = first; i < n; i += stride) {
    const int64_t r = i / cv, c = (i % cv) * V;
    int64_t k = t[r / rows_per_window];
    k = k < 0 ? 0 : (k >= table_rows ? table_rows - 1 : k);
    const float a = sqrt_ab[k], s = sqrt_1mab[k];
    if constexpr (V == 4) {
      float x[4], e[4];
      if constexpr (sizeof(T) == 2) {
        bf16x4_t tx = *reinterpret_cast<const bf16x4_t*>(x0 + r * cols + c), te = *reinterpret_cast<const bf16x4_t*>(eps + r * cols + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) { x[j] = (float)tx[j]; e[j] = (float)te[j]; }
        bf16x4_t o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (bf16_t)q_mix<T, 4>(a, x[j], s, e[j]);
        *reinterpret_cast<bf16x4_t*>(xt + r * ld_xt + c) = o;
      } else {
        const float4 tx = *reinterpret_cast<const float4*>(x0 + r * cols + c), te = *reinterpret_cast<const float4*>(eps + r * cols + c);
        *reinterpret_cast<float4*>(xt + r * ld_xt + c) =
            make_float4(q_mix<T, 4>(a, tx.x, s, te.x), q_mix<T, 4>(a, tx.y, s, te.y), q_mix<T, 4>(a, tx.z, s, te.z),
                        q_mix<T, 4>(a, tx.w, s, te.w));
      }
    } else {
      xt[r * ld_xt + c] = ib_from_f32<T>(q_mix<T, 1>(a, ib_to_f32(x0[r * cols + c]), s, ib_to_f32(eps[r * cols + c])));
    }
  }
}

// dst[r][c] = (D)src[r][c] over rows x cols, each side with its own pitch
template <typename S, typename D>
__device__ __forceinline__ void cast2d_body(const S* __restrict__ src, int64_t lds, D* __restrict__ dst, int64_t ldd,
                                            int64_t rows, int64_t cols, int64_t first, int64_t stride) {
  const int64_t n = rows * cols;
  for (int64_t i = first; i < n; i += stride) {
    const int64_t r = i / cols, c = i % cols;
    dst[r * ldd + c] = ib_from_f32<D>(ib_to_f32(src[r * lds + c]));
  }
}

// a cast2d job of a merged launch: dtypes are IB_F32 / IB_BF16 codes (checked on the host)
struct CastJob { const void* src; void* dst; int64_t lds, ldd, rows, cols; int sd, dd; };
__device__ __forceinline__ void cast2d_job(const CastJob& j, int64_t first, int64_t stride) {
  if (j.sd == IB_BF16 && j.dd == IB_BF16)
    cast2d_body((const bf16_t*)j.src, j.lds, (bf16_t*)j.dst, j.ldd, j.rows, j.cols, first, stride);
  else if (j.sd == IB_F32 && j.dd == IB_F32)
    cast2d_body((const float*)j.src, j.lds, (float*)j.dst, j.ldd, j.rows, j.cols, first, stride);
  else if (j.sd == IB_F32)
    cast2d_body((const float*)j.src, j.lds, (bf16_t*)j.dst, j.ldd, j.rows, j.cols, first, stride);
  else
    cast2d_body((const bf16_t*)j.src, j.lds, (float*)j.dst, j.ldd, j.rows, j.cols, first, stride);
}

// ---- tiny matrix products, short reductions (K < 64): one thread per output element
__device__ __forceinline__ float tiny_ld(const void* p, int dtype, int64_t i) {
  return dtype == IB_F32 ? static_cast<const float*>(p)[i] : static_cast<float>(static_cast<const bf16_t*>(p)[i]);
}
__device__ __forceinline__ void tiny_st(void* p, int dtype, int64_t i, float v, int accumulate) {
  if (dtype == IB_F32) {
    float* q = static_cast<float*>(p) + i;
    *q = accumulate ? *q + v : v;
  } else {
    bf16_t* q = static_cast<bf16_t*>(p) + i;
    *q = static_cast<bf16_t>(accumulate ? static_cast<float>(*q) + v : v);
  }
}
__device__ __forceinline__ void tiny_matmul_thread_body(const void* __restrict__ A, int ad, int64_t sam, int64_t sak,
                                                        const void* __restrict__ B, int bd, int64_t sbk, int64_t sbn,
                                                        void* __restrict__ C, int cd, int64_t ldc, int accumulate, int M,
                                                        int N, int K, int first, int stride) {
  const int total = M * N;
  for (int o = first; o < total; o += stride) {
    const int m = o / N, n = o - m * N;
    // a rolled loop is one memory round trip per k in sequence (K = 30: 31 us for the [50, 30] x [30, 512] frame-embedding
    // projection at the head of every step): batches of 8 operand pairs are requested together, the sum keeps its order
    float acc = 0.f;
    for (int k0 = 0; k0 < K; k0 += 8) {
      float a[8], b[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int k = min(k0 + e, K - 1);
        a[e] = tiny_ld(A, ad, m * sam + k * sak);
        b[e] = tiny_ld(B, bd, k * sbk + n * sbn);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (k0 + e < K) acc += a[e] * b[e];
    }
    tiny_st(C, cd, (int64_t)m * ldc + n, acc, accumulate);
  }
}

// ---- dst_i[c][r] = src_i[r][c] for several bf16 matrices: 64 x 64 tiles through LDS, one tile per block of 256 threads.
// `blk` = the block's index among the transpose blocks, `tile` = [64][TR_TILE_LD] bf16 of shared memory.
constexpr int TR_TILE_LD = 72;                                        // 144-byte rows: 16-byte row writes stay aligned
template <int MAXN>
struct TrMultiT { const bf16_t* src[MAXN]; bf16_t* dst[MAXN]; int rows[MAXN], cols[MAXN], lds[MAXN], ldd[MAXN], blk0[MAXN + 1]; int n; unsigned vec; };
template <int MAXN>
__device__ __forceinline__ void transpose_multi_body(const TrMultiT<MAXN>& m, int blk, bf16_t (*tile)[TR_TILE_LD]) {
  int e = 0;
  for (int j = 1; j < m.n; ++j)
    if (blk >= m.blk0[j]) e = j;
  const int b = blk - m.blk0[e];
  const int R = m.rows[e], Cc = m.cols[e];
  const int tc = (Cc + 63) / 64;
  const int r0 = (b / tc) * 64, c0 = (b % tc) * 64;
  const bf16_t* src = m.src[e];
  bf16_t* dst = m.dst[e];
  if ((m.vec >> e) & 1u) {
    // whole 64 x 64 tiles of 16-byte aligned matrices (every layer weight): 16-byte global accesses on both sides -- two
    // loads and two stores per thread instead of sixteen 2-byte ones each way (the launch was 21.7 us for 52 MB)
    const int pr = threadIdx.x >> 3, pc = threadIdx.x & 7;          // row 0..31 (+32), 16-byte piece 0..7
    uint4 v[2];
#pragma unroll
    for (int h = 0; h < 2; ++h)
      v[h] = *reinterpret_cast<const uint4*>(src + (int64_t)(r0 + pr + 32 * h) * m.lds[e] + c0 + 8 * pc);
#pragma unroll
    for (int h = 0; h < 2; ++h) *reinterpret_cast<uint4*>(&tile[pr + 32 * h][8 * pc]) = v[h];
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = pr + 32 * h;                                    // destination row = source column
      bf16x8_t o;
#pragma unroll
      for (int k = 0; k < 8; ++k) o[k] = tile[8 * pc + k][c];
      *reinterpret_cast<bf16x8_t*>(dst + (int64_t)(c0 + c) * m.ldd[e] + r0 + 8 * pc) = o;
    }
    return;
  }
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int r = ty; r < 64; r += 4)
    tile[r][tx] = (r0 + r < R && c0 + tx < Cc) ? src[(int64_t)(r0 + r) * m.lds[e] + c0 + tx] : (bf16_t)0.f;
  __syncthreads();
  for (int c = ty; c < 64; c += 4)
    if (c0 + c < Cc && r0 + tx < R) dst[(int64_t)(c0 + c) * m.ldd[e] + r0 + tx] = tile[tx][c];
}

// host side: fill one entry of a transpose descriptor; false = bad argument
template <int MAXN>
static inline bool tr_multi_add(TrMultiT<MAXN>& m, int i, const void* src, int64_t lds, void* dst, int64_t ldd, int64_t rows,
                                int64_t cols, int& blk) {
  if (!src || !dst || rows <= 0 || cols <= 0 || lds < cols || ldd < rows) return false;
  m.src[i] = (const bf16_t*)src; m.dst[i] = (bf16_t*)dst;
  m.rows[i] = (int)rows; m.cols[i] = (int)cols; m.lds[i] = (int)lds; m.ldd[i] = (int)ldd;
  m.blk0[i] = blk;
  if (rows % 64 == 0 && cols % 64 == 0 && lds % 8 == 0 && ldd % 8 == 0 && ib_al16({src, dst})) m.vec |= 1u << i;
  blk += (int)(((rows + 63) / 64) * ((cols + 63) / 64));
  return true;
}
