// bf16 Linear GEMMs for batches of a few rows, where the 128 x 128 tiles of gemm.hip leave most of the chip idle: smallm
// (forward and dgrad in 64 x 16 tiles whose waves split the reduction), skinny (dgrad of at most 256 rows, bias gradient in
// the same launch) and wsmall (weight gradient of a short reduction in one pass), behind the ib_*_try functions of
// gemm_families.h.
#include "wave_prims.h"
#include "launch.h"
#include "gemm_families.h"

namespace {

constexpr int BM = 128, BN = 128;   // the tiles of gemm.hip: the predicates count how few of them a problem would get
// IB_NO_SMALLM (measurement builds): smallm and wsmall decline everything
inline bool smallm_off() { static const int off = ib_ab_int("IB_NO_SMALLM", 0); return off; }

// ---- small-M forward -------------------------------------------------------------------------------------------------
// y[M,N] = act(x[M,K] w[N,K]^T + bias) when the 128 x 128 tiling yields only a handful of workgroups (a batch of a few
// hundred rows: the reference's regression models, batch-1 analysis): 64 x 16 output tiles, and the four waves of a
// workgroup split the REDUCTION (k-blocks w, w+4, ...), so every wave walks a quarter of K.  Both operands are
// k-contiguous: fragments come straight from global memory (no LDS staging), the four partial accumulators are combined
// through LDS in a fixed order.  [256, 512, 1470]: 8 workgroups x 46 serial K steps -> 128 workgroups x 12.
namespace smallm {
constexpr int TM = 64, TN = 16, PD = 3;

__device__ __forceinline__ bf16x8_t ldfrag(const bf16_t* __restrict__ rowp, int ks, int K) {
  bf16x8_t v;
  const int nv = K - ks;
  if (nv >= 8) {
    __builtin_memcpy(&v, __builtin_assume_aligned(rowp + ks, 4), 16);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = e < nv ? rowp[ks + e] : (bf16_t)0.f;
  }
  return v;
}

// NT = output-tile width / 16.  Only NT = 1 is instantiated: 64 x 64 tiles (NT = 4) were measured for the sampling loop's
// mid-sized problems (M = 3200, where 128 x 128 tiles leave most CUs idle) and lost to the ring kernel -- [3200, 1536,
// 512] 35.6 vs 17.6 us, [3200, 2048, 512] 48 vs 20 -- fragment loads straight from global memory are 16 rows x 64 bytes
// each and do not reach the rate of whole-row LDS-DMA staging once the tile count is in the hundreds.
template <int ACT, int NT>
__global__ __launch_bounds__(256) void fwd_smallm_kernel(const bf16_t* __restrict__ x, int64_t ldx, const bf16_t* __restrict__ w,
                                                         int64_t ldw, const float* __restrict__ bias,
                                                         const bf16_t* __restrict__ add_div, int64_t ld_ad,
                                                         const bf16_t* __restrict__ add_mod, int64_t ld_am, int seg,
                                                         bf16_t* __restrict__ y, int64_t ldy, int M, int N, int K) {
  constexpr int TNV = 16 * NT;
  __shared__ __attribute__((aligned(16))) float red[4][TM * TNV];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, kq = lane >> 4;
  const int i0 = blockIdx.y * TM, j0 = blockIdx.x * TNV;
  const bf16_t* arow[4];
  const bf16_t* brow[NT];
#pragma unroll
  for (int t = 0; t < 4; ++t) arow[t] = x + (int64_t)min(i0 + 16 * t + r, M - 1) * ldx;
#pragma unroll
  for (int u = 0; u < NT; ++u) brow[u] = w + (int64_t)min(j0 + 16 * u + r, N - 1) * ldw;
  const int nkb = (K + 31) / 32;
  const int nmine = wave < nkb ? (nkb - wave + 3) / 4 : 0;
  f32x4_t acc[4][NT];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int u = 0; u < NT; ++u) acc[t][u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  bf16x8_t fa[PD][4], fb[PD][NT];
  auto load = [&](int s, int it) {
    const int ks = (wave + 4 * it) * 32 + 8 * kq;
#pragma unroll
    for (int t = 0; t < 4; ++t) fa[s][t] = ldfrag(arow[t], ks, K);
#pragma unroll
    for (int u = 0; u < NT; ++u) fb[s][u] = ldfrag(brow[u], ks, K);
  };
#pragma unroll
  for (int s = 0; s < PD; ++s)
    if (s < nmine) load(s, s);
  for (int it0 = 0; it0 < nmine; it0 += PD) {
#pragma unroll
    for (int s = 0; s < PD; ++s) {
      const int it = it0 + s;
      if (it < nmine) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int u = 0; u < NT; ++u)
            acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[s][u], fa[s][t], acc[t][u], 0, 0, 0);
        if (it + PD < nmine) load(s, it + PD);
      }
    }
  }
  // swapped operands: this lane holds columns 16*u + 4*kq .. +3 of row 16*t + r
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int u = 0; u < NT; ++u)
      *reinterpret_cast<float4*>(&red[wave][(16 * t + r) * TNV + 16 * u + 4 * kq]) =
          make_float4(acc[t][u][0], acc[t][u][1], acc[t][u][2], acc[t][u][3]);
  __syncthreads();
  const bool vst = (ldy % 4) == 0 && (reinterpret_cast<uintptr_t>(y) % 8) == 0;
#pragma unroll
  for (int g = 0; g < NT; ++g) {                            // 256 threads x 4 outputs per pass
    const int o0 = (g * 256 + tid) * 4;
    const int row = o0 / TNV, c4 = o0 % TNV;
    const int gi = i0 + row, gj = j0 + c4;
    if (gi >= M || gj >= N) continue;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int o = o0 + e;
      v[e] = ((red[0][o] + red[1][o]) + red[2][o]) + red[3][o];
      if (gj + e < N) {
        if (bias) v[e] += bias[gj + e];
        if (add_div) v[e] += (float)add_div[(int64_t)(gi / seg) * ld_ad + gj + e];
        if (add_mod) v[e] += (float)add_mod[(int64_t)(gi % seg) * ld_am + gj + e];
      }
      v[e] = ib_act_fwd_c<ACT, true>(v[e]);
    }
    bf16_t* dst = y + (int64_t)gi * ldy + gj;
    if (gj + 4 <= N && vst) {
      bf16x4_t o4;
#pragma unroll
      for (int e = 0; e < 4; ++e) o4[e] = (bf16_t)v[e];
      *reinterpret_cast<bf16x4_t*>(dst) = o4;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (gj + e < N) dst[e] = (bf16_t)v[e];
    }
  }
}

// dx[M,K] = (dz[M,N] w[N,K]) * act'(aux): the same tiling for the backward.  w is k-STRIDED here (its rows are the
// reduction index), so the workgroup first transposes its slice w[:, 16 columns] into LDS (rows beyond N zero-filled);
// dz fragments come straight from global memory.
constexpr int RMAX = 1024, WS = RMAX + 8;
template <int ACT>
__global__ __launch_bounds__(256) void dgrad_smallm_kernel(const bf16_t* __restrict__ dz, int64_t lddz,
                                                           const bf16_t* __restrict__ w, int64_t ldw,
                                                           const bf16_t* __restrict__ aux, int64_t ldaux,
                                                           bf16_t* __restrict__ dx, int64_t lddx, int M, int N) {
  __shared__ __attribute__((aligned(16))) bf16_t wimg[16 * WS];
  __shared__ __attribute__((aligned(16))) float red[4][TM * TN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, kq = lane >> 4;
  const int i0 = blockIdx.y * TM, j0 = blockIdx.x * TN;
  const int nkb = (N + 31) / 32;
  for (int pce = tid; pce < nkb * 64; pce += 256) {        // one 16-byte piece = 8 columns of one reduction row
    const int k = pce >> 1, half = pce & 1;
    bf16x8_t v;
    if (k < N) __builtin_memcpy(&v, __builtin_assume_aligned(w + (int64_t)k * ldw + j0 + 8 * half, 16), 16);
    else
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (bf16_t)0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) wimg[(8 * half + e) * WS + k] = v[e];
  }
  __syncthreads();
  const bf16_t* arow[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) arow[t] = dz + (int64_t)min(i0 + 16 * t + r, M - 1) * lddz;
  const bf16_t* brow = wimg + r * WS;
  const int nmine = wave < nkb ? (nkb - wave + 3) / 4 : 0;
  f32x4_t acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  bf16x8_t fa[PD][4];
  auto load = [&](int s, int it) {
    const int ks = (wave + 4 * it) * 32 + 8 * kq;
#pragma unroll
    for (int t = 0; t < 4; ++t) fa[s][t] = ldfrag(arow[t], ks, N);
  };
#pragma unroll
  for (int s = 0; s < PD; ++s)
    if (s < nmine) load(s, s);
  for (int it0 = 0; it0 < nmine; it0 += PD) {
#pragma unroll
    for (int s = 0; s < PD; ++s) {
      const int it = it0 + s;
      if (it < nmine) {
        bf16x8_t b;
        __builtin_memcpy(&b, __builtin_assume_aligned(brow + (wave + 4 * it) * 32 + 8 * kq, 16), 16);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b, fa[s][t], acc[t], 0, 0, 0);
        if (it + PD < nmine) load(s, it + PD);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t)
    *reinterpret_cast<float4*>(&red[wave][(16 * t + r) * TN + 4 * kq]) = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
  __syncthreads();
  const int row = tid >> 2, c4 = (tid & 3) * 4;
  const int gi = i0 + row, gj = j0 + c4;
  if (gi < M) {
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int o = row * TN + c4 + e;
      v[e] = ((red[0][o] + red[1][o]) + red[2][o]) + red[3][o];
    }
    if constexpr (ACT != IB_ACT_NONE) {
      bf16x4_t a4;
      __builtin_memcpy(&a4, __builtin_assume_aligned(aux + (int64_t)gi * ldaux + gj, 8), 8);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] *= ib_act_bwd_c<ACT, true>((float)a4[e]);
    }
    bf16x4_t o4;
#pragma unroll
    for (int e = 0; e < 4; ++e) o4[e] = (bf16_t)v[e];
    __builtin_memcpy(__builtin_assume_aligned(dx + (int64_t)gi * lddx + gj, 8), &o4, 8);
  }
}

// up to this many 128 x 128 tiles the small tiles win (Groundlink F=10 step: cap 32 0.528 ms, 64 0.489, 128 0.491,
// 256 0.502; the DDIM step at M = 3200, 100 tiles: 492 us of kernels at 32 / 64, 515 at 128)
inline int tile_cap() { static const int cap = ib_ab_int("IB_SMALLM_TILES", 64); return cap; }
}  // namespace smallm
}  // namespace

// few 128 x 128 tiles (tile_cap()), plain epilogue (bias, the two row-broadcast addends, activation), rows 4-byte aligned
int ib_bf16_small_fwd_try(const void* x, int64_t ldx, const void* w, int64_t ldw, const float* bias, const void* add_div,
                          int64_t ld_add_div, const void* add_mod, int64_t ld_add_mod, int seg, int act, void* y, int64_t ldy,
                          const void* z, int64_t M, int64_t N, int64_t K, hipStream_t s) {
  using namespace smallm;
  const int64_t tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
  const bool ok = !smallm_off() && tiles <= tile_cap() && !z && ldx % 2 == 0 && ldw % 2 == 0 && ib_aligned(x, 4) &&
                  ib_aligned(w, 4) && K >= 64;
  if (!ok) return IB_E_UNSUPPORTED;
  IB_PATH(IB_PATH_SMALLM);
  const dim3 grid((unsigned)((N + TN - 1) / TN), (unsigned)((M + TM - 1) / TM)), block(256);
  ib_dispatch_act(act, [&](auto a) {
    hipLaunchKernelGGL((fwd_smallm_kernel<decltype(a)::value, 1>), grid, block, 0, s, (const bf16_t*)x, ldx, (const bf16_t*)w,
                       ldw, bias, (const bf16_t*)add_div, ld_add_div, (const bf16_t*)add_mod, ld_add_mod, seg, (bf16_t*)y, ldy,
                       (int)M, (int)N, (int)K);
  });
  IB_CHECK_LAUNCH();
  return IB_OK;
}

int ib_bf16_small_dgrad_try(const void* dz, int64_t lddz, const void* w, int64_t ldw, int act, const void* aux, int64_t ldaux,
                            const void* addend, void* dx, int64_t lddx, int64_t M, int64_t N, int64_t K, hipStream_t s) {
  using namespace smallm;
  const int64_t tiles = ((M + BM - 1) / BM) * ((K + BN - 1) / BN);       // N = reduction length, K = output columns
  const bool ok = !smallm_off() && tiles <= tile_cap() && !addend && N >= 64 && N <= RMAX && K % 16 == 0 && lddz % 2 == 0 &&
                  ib_aligned(dz, 4) && ldw % 8 == 0 && ib_aligned(w, 16) && lddx % 4 == 0 && ib_aligned(dx, 8) &&
                  (act == IB_ACT_NONE || (aux && ldaux % 4 == 0 && ib_aligned(aux, 8)));
  if (!ok) return IB_E_UNSUPPORTED;
  IB_PATH(IB_PATH_SMALLM);
  const dim3 grid((unsigned)(K / TN), (unsigned)((M + TM - 1) / TM)), block(256);
  ib_dispatch_act(act, [&](auto a) {
    hipLaunchKernelGGL((dgrad_smallm_kernel<decltype(a)::value>), grid, block, 0, s, (const bf16_t*)dz, lddz, (const bf16_t*)w,
                       ldw, (const bf16_t*)aux, ldaux, (bf16_t*)dx, lddx, (int)M, (int)N);
  });
  IB_CHECK_LAUNCH();
  return IB_OK;
}

// ---- skinny dgrad: few rows (a batch of time embeddings), long reduction --------------------------------------------
// dx[M,K] = (dz[M,N] . w[N,K]) * act'(aux), M <= 256.  The tiled kernels give such a problem 8 workgroups that each walk
// the whole reduction alone (measured 40 us for [256, 1024] x [1024, 512], on the step's critical path).  Here a
// workgroup owns 16 OUTPUT COLUMNS and all rows: K/16 workgroups, the w slice [N,16] transposed into LDS once, the dz
// rows streamed straight into MFMA fragments through a 4-deep register ring (each wave its own rows: nothing to share),
// and -- because a workgroup sees every row of its columns -- the bias gradient (column sums of dx) comes out of the
// same launch in a fixed order.
namespace skinny {
constexpr int NMAX = 1024, WS = NMAX + 8, PD = 4;       // w image: 16 columns x (N + 8 pad) bf16, k-contiguous

template <int ACT>
__global__ __launch_bounds__(256) void dgrad_skinny_kernel(const bf16_t* __restrict__ dz, int64_t lddz,
                                                           const bf16_t* __restrict__ w, int64_t ldw,
                                                           const bf16_t* __restrict__ aux, int64_t ldaux,
                                                           bf16_t* __restrict__ dx, int64_t lddx, float* __restrict__ dbias,
                                                           int accumulate, int M, int N) {
  __shared__ __attribute__((aligned(16))) bf16_t wimg[16 * WS];
  __shared__ float red[4][16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c0 = blockIdx.x * 16;
  // w[:, c0 .. c0+16) -> wimg[col][k]: one 16-byte piece = 8 columns of one reduction row
  // (four pieces per thread requested before the first is scattered: a rolled loop was N/128 dependent round trips)
  for (int p0 = tid; p0 < N * 2; p0 += 256 * 4) {
    bf16x8_t v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int pce = min(p0 + 256 * u, N * 2 - 1), k = pce >> 1, half = pce & 1;
      __builtin_memcpy(&v[u], __builtin_assume_aligned(w + (int64_t)k * ldw + c0 + 8 * half, 16), 16);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int pce = p0 + 256 * u, k = pce >> 1, half = pce & 1;
      if (pce < N * 2) {
#pragma unroll
        for (int e = 0; e < 8; ++e) wimg[(8 * half + e) * WS + k] = v[u][e];
      }
    }
  }
  __syncthreads();
  const int mt_total = (M + 15) / 16;
  const int r = lane & 15, kq = lane >> 4;
  const bf16_t* arow[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = min((wave + 4 * j) * 16 + r, M - 1);   // tiles past the last row read valid memory and store nothing
    arow[j] = dz + (int64_t)row * lddz + 8 * kq;
  }
  f32x4_t acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  bf16x8_t ar[PD][4];
  const int nkb = N / 32;                                  // a multiple of PD by the launch conditions
#pragma unroll
  for (int sl = 0; sl < PD; ++sl)
#pragma unroll
    for (int j = 0; j < 4; ++j) __builtin_memcpy(&ar[sl][j], __builtin_assume_aligned(arow[j] + sl * 32, 16), 16);
  const bf16_t* brow = wimg + r * WS + 8 * kq;
  for (int kb0 = 0; kb0 < nkb; kb0 += PD) {
#pragma unroll
    for (int sl = 0; sl < PD; ++sl) {
      const int kb = kb0 + sl;
      bf16x8_t b;
      __builtin_memcpy(&b, __builtin_assume_aligned(brow + kb * 32, 16), 16);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b, ar[sl][j], acc[j], 0, 0, 0);
      const int kn = min(kb + PD, nkb - 1);                // the last PD refills re-read the final block (never used)
#pragma unroll
      for (int j = 0; j < 4; ++j) __builtin_memcpy(&ar[sl][j], __builtin_assume_aligned(arow[j] + kn * 32, 16), 16);
    }
  }
  // swapped operands: this lane holds columns c0 + 4*kq .. +3 of row (tile, r)
  float cs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = (wave + 4 * j) * 16 + r;
    if (wave + 4 * j >= mt_total || row >= M) continue;
    float v[4] = {acc[j][0], acc[j][1], acc[j][2], acc[j][3]};
    if constexpr (ACT != IB_ACT_NONE) {
      bf16x4_t a4;
      __builtin_memcpy(&a4, __builtin_assume_aligned(aux + (int64_t)row * ldaux + c0 + 4 * kq, 8), 8);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] *= ib_act_bwd_c<ACT, true>((float)a4[e]);
    }
    bf16x4_t o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      o[e] = (bf16_t)v[e];
      cs[e] += (float)o[e];                                // the bias gradient is the column sum of the STORED tensor
    }
    __builtin_memcpy(__builtin_assume_aligned(dx + (int64_t)row * lddx + c0 + 4 * kq, 8), &o, 8);
  }
  if (dbias) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) cs[e] += __shfl_xor(cs[e], o, 64);     // the 16 rows of a tile: fixed butterfly
      if (r == 0) red[wave][4 * kq + e] = cs[e];
    }
    __syncthreads();
    if (tid < 16) {
      const float sum = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
      dbias[c0 + tid] = accumulate ? dbias[c0 + tid] + sum : sum;
    }
  }
}
}  // namespace skinny

int ib_skinny_dgrad_try(const void* dz, int64_t lddz, const void* w, int64_t ldw, int act, const void* aux, int64_t ldaux,
                        void* dx, int64_t lddx, float* dbias, int accumulate, int64_t M, int64_t N, int64_t K, int dtype,
                        hipStream_t s) {
  if (dtype != IB_BF16 || M > 256 || N > skinny::NMAX || N % (32 * skinny::PD) != 0 || K % 16 != 0) return IB_E_UNSUPPORTED;
  if (!ib_aligned(dz, 16) || lddz % 8 != 0 || !ib_aligned(w, 16) || ldw % 8 != 0 || !ib_aligned(dx, 8) || lddx % 4 != 0 ||
      (aux && (!ib_aligned(aux, 8) || ldaux % 4 != 0)))
    return IB_E_UNSUPPORTED;
  const dim3 grid((unsigned)(K / 16)), block(256);
  IB_PATH(IB_PATH_SKINNY);
  ib_dispatch_act(act, [&](auto a) {
    hipLaunchKernelGGL((skinny::dgrad_skinny_kernel<decltype(a)::value>), grid, block, 0, s, (const bf16_t*)dz, lddz,
                       (const bf16_t*)w, ldw, (const bf16_t*)aux, ldaux, (bf16_t*)dx, lddx, dbias, accumulate, (int)M, (int)N);
  });
  IB_CHECK_LAUNCH();
  return IB_OK;
}

// ---- weight gradient over a SHORT reduction (a batch of a few hundred rows) -----------------------------------------------
// dw[N,K] (+)= dz[M,N]^T x[M,K] with M <= 1024.  The split-M kernels above exist to find parallelism in a long reduction;
// here the OUTPUT is the large side ([512, 1470] from 256 rows), so 64 x 64 output tiles alone give hundreds of
// workgroups: no split, no slabs, no reduction launch.  Both operands are indexed [reduction][column]: a workgroup stages
// its two [rows][64] slices in LDS (256 rows at a time) and reads MFMA fragments with the transposing ds_read_b64_tr_b16.
// [256 rows; 512 x 1470]: 20.8 us (GEMM + slab reduction) -> one launch.
namespace wsmall {
constexpr int CH = 256, PITCH = 72;       // rows per LDS chunk; image row pitch in elements (64 + 8: 144 B)

__device__ __forceinline__ bf16x8_t frag_tr(const bf16_t* img, int rbase, int lane) {       // img: first row of a 32-row K step
  const int q = (lane & 15) >> 2, pp = lane & 3;
  const int kr = 8 * (lane >> 4) + q;
  return lds_read_tr<0, 4 * PITCH * 2>(lds_off(img) + (kr * PITCH + rbase + 4 * pp) * 2);
}

__global__ __launch_bounds__(256) void wgrad_smallm_kernel(const bf16_t* __restrict__ dz, int64_t lddz,
                                                           const bf16_t* __restrict__ x, int64_t ldx, float* __restrict__ dw,
                                                           int64_t lddw, float* __restrict__ dbias, int accumulate, int M,
                                                           int N, int K) {
  __shared__ __attribute__((aligned(16))) bf16_t aimg[CH * PITCH];
  __shared__ __attribute__((aligned(16))) bf16_t bimg[CH * PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = wave >> 1, wj = wave & 1;
  const int n0 = blockIdx.y * 64, k0 = blockIdx.x * 64;
  f32x4_t acc[2][2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int u = 0; u < 2; ++u) acc[t][u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;
  for (int m0 = 0; m0 < M; m0 += CH) {
    if (m0) __syncthreads();                               // the previous chunk's fragments have been read
    const int rows = min(CH, M - m0), rows32 = (rows + 31) / 32 * 32;
    for (int pce = tid; pce < rows32 * 8; pce += 256) {    // [row][8 pieces of 8 columns], rows past the end zero-filled
      const int m = pce >> 3, c = (pce & 7) * 8;
      bf16x8_t va, vb;
      if (m < rows) {
        va = smallm::ldfrag(dz + (int64_t)(m0 + m) * lddz, n0 + c, N);
        vb = smallm::ldfrag(x + (int64_t)(m0 + m) * ldx, k0 + c, K);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) { va[e] = (bf16_t)0.f; vb[e] = (bf16_t)0.f; }
      }
      __builtin_memcpy(__builtin_assume_aligned(aimg + m * PITCH + c, 16), &va, 16);
      __builtin_memcpy(__builtin_assume_aligned(bimg + m * PITCH + c, 16), &vb, 16);
    }
    __syncthreads();
    // the bias gradient of the same layer = column sums of dz: the first workgroup of every row of tiles has the slice
    // in LDS anyway (one thread per column, rows added in order)
    if (dbias && blockIdx.x == 0 && tid < 64) {
      float sacc = 0.f;
      for (int m = 0; m < rows; ++m) sacc += (float)aimg[m * PITCH + tid];
      bsum += sacc;
    }
    for (int ks = 0; ks < rows32; ks += 32) {
      bf16x8_t fa[2], fb[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) fa[t] = frag_tr(aimg + ks * PITCH, wi * 32 + 16 * t, lane);
#pragma unroll
      for (int u = 0; u < 2; ++u) fb[u] = frag_tr(bimg + ks * PITCH, wj * 32 + 16 * u, lane);
      frags_ready(fa, fb);
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u) acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[u], fa[t], acc[t][u], 0, 0, 0);
    }
  }
  if (dbias && blockIdx.x == 0 && tid < 64 && n0 + tid < N) dbias[n0 + tid] = accumulate ? dbias[n0 + tid] + bsum : bsum;
  // swapped operands: this lane holds output columns (k) 16*u + 4*(lane >> 4) .. +3 of output row (n) 16*t + (lane & 15)
  const bool vst = (lddw % 4) == 0 && (reinterpret_cast<uintptr_t>(dw) % 16) == 0;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int n = n0 + wi * 32 + 16 * t + (lane & 15);
    if (n >= N) continue;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int k = k0 + wj * 32 + 16 * u + 4 * (lane >> 4);
      if (k >= K) continue;
      float* o = dw + (int64_t)n * lddw + k;
      float v[4] = {acc[t][u][0], acc[t][u][1], acc[t][u][2], acc[t][u][3]};
      if (k + 4 <= K && vst) {
        float4 w4 = make_float4(v[0], v[1], v[2], v[3]);
        if (accumulate) { const float4 p4 = *reinterpret_cast<const float4*>(o); w4.x += p4.x; w4.y += p4.y; w4.z += p4.z; w4.w += p4.w; }
        *reinterpret_cast<float4*>(o) = w4;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (k + e < K) o[e] = accumulate ? o[e] + v[e] : v[e];
      }
    }
  }
}

inline bool ok(const void* dz, int64_t lddz, const void* x, int64_t ldx, int64_t M, int dtype) {
  // M <= 1024: with 2560 rows (Groundlink, F = 10) the ten serial LDS chunks per workgroup lose to the split-M kernels
  // (step 0.496 -> 0.789 ms when the limit was raised to 4096)
  return !smallm_off() && dtype == IB_BF16 && M <= 1024 && lddz % 2 == 0 && ldx % 2 == 0 && ib_aligned(dz, 4) && ib_aligned(x, 4);
}
}  // namespace wsmall

// the only launch site of wgrad_smallm_kernel: dw [N, K] (+)= dz^T x, and dbias [N] (+)= the column sums of dz when given.
// The caller has checked its own pointers and pitches; this decides only whether the family takes the problem.
int ib_wgrad_small_try(const void* dz, int64_t lddz, const void* x, int64_t ldx, float* dw, int64_t lddw, float* dbias,
                       int accumulate, int64_t M, int64_t N, int64_t K, int dtype, hipStream_t s) {
  if (!wsmall::ok(dz, lddz, x, ldx, M, dtype)) return IB_E_UNSUPPORTED;
  IB_PATH(IB_PATH_WGRAD_SMALL);
  hipLaunchKernelGGL(wsmall::wgrad_smallm_kernel, dim3((unsigned)((K + 63) / 64), (unsigned)((N + 63) / 64)), dim3(256), 0, s,
                     (const bf16_t*)dz, lddz, (const bf16_t*)x, ldx, dw, lddw, dbias, accumulate, (int)M, (int)N, (int)K);
  IB_CHECK_LAUNCH();
  return IB_OK;
}
