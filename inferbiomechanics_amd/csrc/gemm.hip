// Linear-layer GEMMs for gfx950: one LDS-tiled MFMA kernel family, three operand layouts.
//
//   C[i][j] = sum_k A(i,k) * B(j,k)            128 x 128 output tile per 256-thread workgroup,
//                                              4 waves as 2x2, each wave 64x64 = 4x4 MFMA 16x16 tiles
//   fwd   : A = x  [M,K]  (k-contiguous), B = w  [N,K] (k-contiguous)     y  = act(x w^T + ...)
//   dgrad : A = dz [M,N]  (k-contiguous), B = w  [N,K] (k-STRIDED)        dx = (dz w) * act'(aux)
//   wgrad : A = dz [M,N]  (k-STRIDED)   , B = x  [M,K] (k-STRIDED)        dw = dz^T x   (split over M)
//
// dtype f32  : v_mfma_f32_16x16x4_f32  (exact f32 fma chain -> the parity mode)
// dtype bf16 : v_mfma_f32_16x16x32_bf16, fp32 accumulate (the throughput mode)
//
// LDS images keep the GLOBAL orientation of each operand (so staging is always 16-byte pieces,
// coalesced along the contiguous dimension): k-contiguous operands as [row][k], k-strided operands
// as [k][row].  bf16 fragments of a [k][row] image are read with ds_read_b64_tr_b16 (the hardware
// transposing read), everything else with ds_read_b128 / ds_read_b32.
// The MFMA is issued "swapped" (a = B-tile rows, b = A-tile rows) so that each lane ends up with
// 4 CONSECUTIVE output columns of one output row -> 8/16-byte epilogue stores and bias loads.
#include <type_traits>

#include "wave_prims.h"
#include "gemm_families.h"
#include "time_bwd.h"

namespace {

constexpr int BM = 128, BN = 128, NTHREADS = 256;
constexpr int OPER_BYTES = 18432;  // one operand tile image (max over layouts / dtypes)

template <typename T> struct Tile;
template <> struct Tile<float> {
  static constexpr int BK = 32, VW = 4, KC_STRIDE = 34, KS_STRIDE = 144;
};
template <> struct Tile<bf16_t> {
  static constexpr int BK = 64, VW = 8, KC_STRIDE = 72, KS_STRIDE = 144;
};

enum { EPI_FWD = 0, EPI_DGRAD = 1, EPI_WGRAD = 2 };

// TIMING-ONLY ablation switch (tools/kbench.py --ablate): bit0 skip steady-state global loads, bit1 skip LDS
// stores, bit2 skip MFMAs, bit3 skip the epilogue stores.  Results are wrong when non-zero; never set by product code.
#ifdef IB_AB
int g_ablate = 0;
long long* g_gemm_prof = nullptr;   // TIMING-ONLY (tools/gemm_prof.py): [workgroups][8] wall-clock stamps of the ring kernel
#define IB_ABLATE g_ablate
#else
#define IB_ABLATE 0
#endif

struct GemmParams {
  const void* A; const void* B; int64_t lda, ldb;
  int M, N, K;                 // C is [M,N]; K is the reduction length
  void* C; int64_t ldc;
  void* Z; int64_t ldz;        // fwd: optional pre-activation output
  const float* bias;
  const void* add_div; int64_t ld_add_div;
  const void* add_mod; int64_t ld_add_mod;
  int seg;
  const void* aux; int64_t ldaux;  // dgrad: activation-derivative operand
  const void* addend; int64_t ldadd;  // dgrad: residual-path gradient added in the epilogue
  int act;
  int vecA, vecB, vecC;
  int gldsA, gldsB;            // operand pieces are 16-byte aligned: direct-to-LDS staging is legal (bf16)
  int vecBias, vecAdd, vecAux;   // 16-byte (fp32) / 8-byte (bf16) epilogue operand loads are legal
  int tiles_m, tiles_n;
  int xcd_group;               // give each XCD a contiguous run of logical block ids
  int k_chunk;                 // split over the reduction (wgrad): blockIdx.y * k_chunk
  int64_t slab_stride;         // wgrad: elements between partial slabs (0 when not split)
  int accumulate;
  int ablate;
  long long* prof;
  float* dbias_part;           // wgrad (ring kernel): optional [splits][M] fp32 per-slice row sums of A (= the bias gradient's
                               // split-M partial sums: sum over the slice's rows of dz), written by the column-tile-0 blocks
};

template <typename T>
__device__ __forceinline__ uint4 load_piece(const T* p, int nvalid, bool vec) {
  constexpr int VW = Tile<T>::VW;
  uint4 r = make_uint4(0u, 0u, 0u, 0u);
  if (nvalid >= VW && vec) {
    __builtin_memcpy(&r, __builtin_assume_aligned(p, 4), 16);
  } else if (nvalid > 0) {
    T tmp[VW];
#pragma unroll
    for (int e = 0; e < VW; ++e) tmp[e] = static_cast<T>(0.f);
#pragma unroll
    for (int e = 0; e < VW; ++e)
      if (e < nvalid) tmp[e] = p[e];
    __builtin_memcpy(&r, tmp, 16);
  }
  return r;
}

// global -> registers: 4 x 16-byte pieces per thread per operand tile
template <typename T, bool KC>
__device__ __forceinline__ void load_tile(const T* base, int64_t ld, int row0, int rows_total, int k0,
                                          int k_end, bool vec, uint4 (&r)[4], int tid) {
  constexpr int VW = Tile<T>::VW;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int p = tid + NTHREADS * q;
    if (KC) {
      const int row = p >> 3, kc = p & 7;
      const int gr = row0 + row, gk = k0 + kc * VW;
      const int nvalid = (gr < rows_total) ? min(VW, k_end - gk) : 0;
      r[q] = load_piece<T>(base + (int64_t)gr * ld + gk, nvalid, vec);
    } else {
      constexpr int RG = 128 / VW;
      const int kk = p / RG, rg = p % RG;
      const int gk = k0 + kk, gr = row0 + rg * VW;
      const int nvalid = (gk < k_end) ? min(VW, rows_total - gr) : 0;
      r[q] = load_piece<T>(base + (int64_t)gk * ld + gr, nvalid, vec);
    }
  }
}

// Hoisted form for the steady state: per-thread piece pointers are computed once per workgroup and
// advanced by a constant per K step; no predicates (k-contiguous operands clamp out-of-range rows to the
// last valid row -- those tile rows only feed outputs that are never stored; k-strided operands use this
// path with a per-piece row count: full pieces load 16 bytes, edge pieces are zero-filled element-wise).
template <typename T, bool KC>
__device__ __forceinline__ void init_ptrs(const T* base, int64_t ld, int row0, int rows_total, int k0,
                                          const T* (&ptr)[4], int (&nvr)[4], int tid) {
  constexpr int VW = Tile<T>::VW;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int p = tid + NTHREADS * q;
    if (KC) {
      const int row = p >> 3, kc = p & 7;
      const int gr = min(row0 + row, rows_total - 1);
      ptr[q] = base + (int64_t)gr * ld + k0 + kc * VW;
      nvr[q] = VW;
    } else {
      constexpr int RG = 128 / VW;
      const int kk = p / RG, rg = p % RG;
      const int gr = row0 + rg * VW;
      ptr[q] = base + (int64_t)(k0 + kk) * ld + gr;
      nvr[q] = max(0, min(VW, rows_total - gr));   // rows of this piece inside the matrix (loop-invariant)
    }
  }
}
template <typename T, bool KC>
__device__ __forceinline__ void load_tile_fast(const T* const (&ptr)[4], const int (&nvr)[4], int64_t off,
                                               uint4 (&r)[4]) {
  constexpr int VW = Tile<T>::VW;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (KC || nvr[q] == VW) {
      __builtin_memcpy(&r[q], __builtin_assume_aligned(ptr[q] + off, 4), 16);
    } else {
      r[q] = load_piece<T>(ptr[q] + off, nvr[q], false);   // edge piece of a k-strided operand: zero-filled
    }
  }
}

// registers -> LDS image
template <typename T, bool KC>
__device__ __forceinline__ void store_tile(unsigned char* tile, const uint4 (&r)[4], int tid) {
  constexpr int VW = Tile<T>::VW;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int p = tid + NTHREADS * q;
    if (KC) {
      const int row = p >> 3, kc = p & 7;
      const int byte = (row * Tile<T>::KC_STRIDE + kc * VW) * (int)sizeof(T);
      if (sizeof(T) == 2) {
        *reinterpret_cast<uint4*>(tile + byte) = r[q];
      } else {  // 136-byte rows: only 8-byte aligned
        *reinterpret_cast<uint2*>(tile + byte) = make_uint2(r[q].x, r[q].y);
        *reinterpret_cast<uint2*>(tile + byte + 8) = make_uint2(r[q].z, r[q].w);
      }
    } else {
      constexpr int RG = 128 / VW;
      const int kk = p / RG, rg = p % RG;
      const int byte = (kk * Tile<T>::KS_STRIDE + rg * VW) * (int)sizeof(T);
      *reinterpret_cast<uint4*>(tile + byte) = r[q];
    }
  }
}

// ---- direct-to-LDS staging (bf16): global_load_lds_dwordx4 writes 16 B per lane straight into the LDS
// image (no VGPR round trip, no ds_write: VGPR->LDS stores run at ~80 B/clk/CU and were ~1/3 of a K step).
// One wave-instruction fills 1 KiB of the image at (wave-uniform base + lane*16), so the 18 KiB image
// (128 rows x 144 B, or 64 k-rows x 288 B) is 18 chunks; wave w issues chunks w, w+4, ...  Each lane derives
// WHICH global piece belongs at its LDS slot from the slot's byte offset; lanes that fall into the row padding
// fetch a duplicate piece (the pad bytes are never read).
constexpr int GLDS_CHUNKS = OPER_BYTES / 1024;   // 18

template <bool KC>
__device__ __forceinline__ void glds_offsets(int64_t ld, int row0, int rows_total, int wave, int lane, int64_t (&off)[5]) {
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const int chunk = wave + 4 * j;
    const int o = (chunk < GLDS_CHUNKS ? chunk : 0) * 1024 + lane * 16;
    if (KC) {
      const int row = o / 144, c = min((o % 144) / 16, 7);
      off[j] = (int64_t)min(row0 + row, rows_total - 1) * ld + 8 * c;
    } else {
      const int kk = o / 288, c = min((o % 288) / 16, 15);
      off[j] = (int64_t)kk * ld + row0 + 8 * c;
    }
  }
}
__device__ __forceinline__ void glds_issue(const bf16_t* base, const int64_t (&off)[5], int64_t koff, unsigned char* tile,
                                           int wave) {
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const int chunk = wave + 4 * j;
    if (chunk < GLDS_CHUNKS)
      __builtin_amdgcn_global_load_lds((glb_void_t*)(base + off[j] + koff), (lds_void_t*)(tile + chunk * 1024), 16, 0, 0);
  }
}

// bf16 fragment: 8 consecutive k of tile row (rbase + lane%16), k = kbase + 8*(lane/16) + j
template <bool KC, int KCS = Tile<bf16_t>::KC_STRIDE>
__device__ __forceinline__ bf16x8_t read_frag_bf16(const unsigned char* tile, int rbase, int kbase, int lane) {
  if (KC) {
    const int off = ((rbase + (lane & 15)) * KCS + kbase + 8 * (lane >> 4)) * 2;
    return *reinterpret_cast<const bf16x8_t*>(tile + off);
  } else {
    // [k][row] image, transposing read (wave_prims.h): lane 4q+p of a 16-lane group addresses row (k) q, columns 4p..4p+3
    const int q = (lane & 15) >> 2, pp = lane & 3;
    const int kr = kbase + 8 * (lane >> 4) + q;
    const bf16_t* a0 = reinterpret_cast<const bf16_t*>(tile) + kr * Tile<bf16_t>::KS_STRIDE + rbase + 4 * pp;
    return lds_read_tr16(a0, a0 + 4 * Tile<bf16_t>::KS_STRIDE);
  }
}

template <bool KC>
__device__ __forceinline__ float read_frag_f32(const unsigned char* tile, int rbase, int kbase, int lane) {
  const float* t = reinterpret_cast<const float*>(tile);
  if (KC) return t[(rbase + (lane & 15)) * Tile<float>::KC_STRIDE + kbase + (lane >> 4)];
  return t[(kbase + (lane >> 4)) * Tile<float>::KS_STRIDE + rbase + (lane & 15)];
}

template <typename T, bool A_KC, bool B_KC>
__device__ __forceinline__ void compute_tile(const unsigned char* tA, const unsigned char* tB,
                                             f32x4_t (&acc)[4][4], int lane, int wi, int wj) {
  if constexpr (sizeof(T) == 2) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8_t fa[4], fb[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) fa[t] = read_frag_bf16<A_KC>(tA, wi * 64 + 16 * t, ks * 32, lane);
#pragma unroll
      for (int u = 0; u < 4; ++u) fb[u] = read_frag_bf16<B_KC>(tB, wj * 64 + 16 * u, ks * 32, lane);
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u)
          acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[u], fa[t], acc[t][u], 0, 0, 0);
    }
  } else {
#pragma unroll
    for (int kk = 0; kk < Tile<float>::BK / 4; ++kk) {
      float fa[4], fb[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) fa[t] = read_frag_f32<A_KC>(tA, wi * 64 + 16 * t, kk * 4, lane);
#pragma unroll
      for (int u = 0; u < 4; ++u) fb[u] = read_frag_f32<B_KC>(tB, wj * 64 + 16 * u, kk * 4, lane);
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u)
          acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(fb[u], fa[t], acc[t][u], 0, 0, 0);
    }
  }
}

// raw 4-element operand piece (8 B bf16 / 16 B fp32) kept in registers until all loads are in flight
template <typename T> struct Raw4 { typename std::conditional<sizeof(T) == 2, uint2, uint4>::type v; };
template <typename T>
__device__ __forceinline__ Raw4<T> ldraw4(const T* __restrict__ p, int nv, bool vec) {
  Raw4<T> r;
  if (nv == 4 && vec) {
    r.v = *reinterpret_cast<const decltype(r.v)*>(p);
  } else {
    T tmp[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) tmp[e] = (e < nv) ? p[e] : static_cast<T>(0.f);
    __builtin_memcpy(&r.v, tmp, sizeof(r.v));
  }
  return r;
}
template <typename T>
__device__ __forceinline__ void unraw4(const Raw4<T>& r, float (&v)[4]) {
  T tmp[4];
  __builtin_memcpy(tmp, &r.v, sizeof(r.v));
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = ib_to_f32(tmp[e]);
}

// Epilogue: a lane holds C[i][jb..jb+3] for 16 (t,u) sub-tiles.  Phase 1 issues EVERY operand load (bias,
// row-broadcast adds, activation-derivative operand, residual) so they are all in flight together; phase 2
// does the math and the stores.  (A per-sub-tile load->math->store chain serialises 16 L2 round trips.)
template <typename T, int EPI, int ACT>
__device__ __forceinline__ void epilogue(const GemmParams& p, f32x4_t (&acc)[4][4], int i0, int j0, int wi, int wj,
                                         int lane, int split_id) {
  const int jb0 = j0 + wj * 64 + 4 * (lane >> 4);
  const int ib0 = i0 + wi * 64 + (lane & 15);
  [[maybe_unused]] Raw4<float> rb[4];
  [[maybe_unused]] Raw4<T> r1[4][4], r2[4][4];
  [[maybe_unused]] bool h1 = false, h2 = false;
  if constexpr (EPI == EPI_FWD) {
    h1 = p.add_div != nullptr; h2 = p.add_mod != nullptr;
    if (p.bias) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int jb = jb0 + 16 * u;
        rb[u] = ldraw4<float>(p.bias + jb, max(0, min(4, p.N - jb)), p.vecBias);
      }
    }
  } else if constexpr (EPI == EPI_DGRAD) {
    h1 = (ACT != IB_ACT_NONE); h2 = p.addend != nullptr;
  }
  if constexpr (EPI != EPI_WGRAD) {
    if (h1 || h2) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int i = min(ib0 + 16 * t, p.M - 1);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int jb = jb0 + 16 * u;
          const int nv = max(0, min(4, p.N - jb));
          if constexpr (EPI == EPI_FWD) {
            if (h1) r1[t][u] = ldraw4<T>(reinterpret_cast<const T*>(p.add_div) + (int64_t)(i / p.seg) * p.ld_add_div + jb, nv, p.vecAdd);
            if (h2) r2[t][u] = ldraw4<T>(reinterpret_cast<const T*>(p.add_mod) + (int64_t)(i % p.seg) * p.ld_add_mod + jb, nv, p.vecAdd);
          } else {
            if (h1) r1[t][u] = ldraw4<T>(reinterpret_cast<const T*>(p.aux) + (int64_t)i * p.ldaux + jb, nv, p.vecAux);
            if (h2) r2[t][u] = ldraw4<T>(reinterpret_cast<const T*>(p.addend) + (int64_t)i * p.ldadd + jb, nv, p.vecAdd);
          }
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int i = ib0 + 16 * t;
    if (i >= p.M) continue;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int jb = jb0 + 16 * u;
      if (jb >= p.N) continue;
      const int nv = min(4, p.N - jb);
      float v[4] = {acc[t][u][0], acc[t][u][1], acc[t][u][2], acc[t][u][3]};
      float w4[4];
      if constexpr (EPI == EPI_FWD) {
        if (p.bias) {
          unraw4<float>(rb[u], w4);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += w4[r];
        }
        if (h1) {
          unraw4<T>(r1[t][u], w4);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += w4[r];
        }
        if (h2) {
          unraw4<T>(r2[t][u], w4);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += w4[r];
        }
        if (p.Z) store4<T>(reinterpret_cast<T*>(p.Z) + (int64_t)i * p.ldz + jb, nv, p.vecC, v);
        if constexpr (ACT != IB_ACT_NONE) {
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = ib_act_fwd_c<ACT, sizeof(T) == 2>(v[r]);
        }
        store4<T>(reinterpret_cast<T*>(p.C) + (int64_t)i * p.ldc + jb, nv, p.vecC, v);
      } else if constexpr (EPI == EPI_DGRAD) {
        if constexpr (ACT != IB_ACT_NONE) {
          unraw4<T>(r1[t][u], w4);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] *= ib_act_bwd_c<ACT, sizeof(T) == 2>(w4[r]);
        }
        if (h2) {
          unraw4<T>(r2[t][u], w4);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += w4[r];
        }
        store4<T>(reinterpret_cast<T*>(p.C) + (int64_t)i * p.ldc + jb, nv, p.vecC, v);
      } else {
        float* c = reinterpret_cast<float*>(p.C) + (int64_t)split_id * p.slab_stride + (int64_t)i * p.ldc + jb;
        if (p.accumulate && p.slab_stride == 0) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (r < nv) v[r] += c[r];
        }
        store4<float>(c, nv, p.vecC, v);
      }
    }
  }
}

template <typename T, bool A_KC, bool B_KC, int EPI>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_kernel(GemmParams p) {
  constexpr int BK = Tile<T>::BK;
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * OPER_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = wave >> 1, wj = wave & 1;
  // XCD-aware order: blocks b and b+8 share an XCD (round-robin dispatch), so after the remap a run of
  // consecutive logical ids sits on one XCD.  fwd/dgrad: the tiles_n column tiles of one row panel; wgrad: ALL
  // output tiles of one M-chunk (they re-read the same dz / x chunk -- without this the chunk was fetched by up
  // to 8 L2s: 79 MB fetched for 21 MB algorithmic in the first profile).  Speed only, never correctness.
  const int bid = p.xcd_group ? ib_xcd_remap(blockIdx.x, gridDim.x) : (int)blockIdx.x;
  const int tiles_total = p.tiles_m * p.tiles_n;
  const int split_id = bid / tiles_total, tile_id = bid % tiles_total;
  const int ti = tile_id / p.tiles_n, tj = tile_id % p.tiles_n;
  const int i0 = ti * BM, j0 = tj * BN;
  const int kb = split_id * p.k_chunk;
  const int ke = min(p.K, kb + p.k_chunk);
  const int nk = (ke - kb + BK - 1) / BK;
  const T* A = reinterpret_cast<const T*>(p.A);
  const T* B = reinterpret_cast<const T*>(p.B);

  f32x4_t acc[4][4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[t][u] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // fast (unpredicated, pointer-bumped) staging where legal, generic predicated staging elsewhere
  const bool fastA = p.vecA, fastB = p.vecB;
  const T* pa[4]; const T* pb[4];
  int na[4], nb[4];
  init_ptrs<T, A_KC>(A, p.lda, i0, p.M, kb, pa, na, tid);
  init_ptrs<T, B_KC>(B, p.ldb, j0, p.N, kb, pb, nb, tid);
  const int64_t stepA = A_KC ? BK : (int64_t)BK * p.lda;
  const int64_t stepB = B_KC ? BK : (int64_t)BK * p.ldb;

  // Double-buffered LDS, one barrier per K step.  Per operand and K step the tile is staged either
  //  (g) directly HBM/L2 -> LDS by global_load_lds (bf16, 16-byte-aligned pieces, full K step, and -- for
  //      k-strided operands -- an interior tile), issued BEFORE the MFMA phase of the previous tile, or
  //  (r) through registers (predicated / zero-filled: K tails, edge tiles, unaligned or fp32 operands), loaded
  //      before the MFMA phase and written to LDS after it.
  // (A depth-2 register prefetch was measured slower for the k-strided operands: wgrad +25 %, dgrad +10 %.)
  bool gA = false, gB = false;
  [[maybe_unused]] int64_t oa[5], ob[5];
  if constexpr (sizeof(T) == 2) {
    // measured (tools/kbench.py): direct-to-LDS staging pays for long reductions (K = 2048 forward: 48 -> 41 us)
    // and is neutral-to-slightly-negative below ~16 K steps, where prologue/epilogue dominate
    const bool longk = nk >= 16;
    gA = longk && p.gldsA && (A_KC || i0 + BM <= p.M);
    gB = longk && p.gldsB && (B_KC || j0 + BN <= p.N);
    if (gA) glds_offsets<A_KC>(p.lda, i0, p.M, wave, lane, oa);
    if (gB) glds_offsets<B_KC>(p.ldb, j0, p.N, wave, lane, ob);
  }
  uint4 ra[4], rb[4];
  // returns bit0: A staged through registers, bit1: B staged through registers
  auto stage_issue = [&](int kt, unsigned char* tA, unsigned char* tB) -> int {
    const int k0 = kb + kt * BK;
    const bool fullk = (k0 + BK <= ke);
    int viaregs = 0;
    if constexpr (sizeof(T) == 2) {
      if (gA && fullk) glds_issue(reinterpret_cast<const bf16_t*>(A), oa, A_KC ? (int64_t)k0 : (int64_t)k0 * p.lda, tA, wave);
      else viaregs |= 1;
      if (gB && fullk) glds_issue(reinterpret_cast<const bf16_t*>(B), ob, B_KC ? (int64_t)k0 : (int64_t)k0 * p.ldb, tB, wave);
      else viaregs |= 2;
    } else {
      viaregs = 3;
    }
    if (viaregs & 1) {
      if (fastA && fullk) load_tile_fast<T, A_KC>(pa, na, stepA * kt, ra);
      else load_tile<T, A_KC>(A, p.lda, i0, p.M, k0, ke, p.vecA, ra, tid);
    }
    if (viaregs & 2) {
      if (fastB && fullk) load_tile_fast<T, B_KC>(pb, nb, stepB * kt, rb);
      else load_tile<T, B_KC>(B, p.ldb, j0, p.N, k0, ke, p.vecB, rb, tid);
    }
    return viaregs;
  };
  auto stage_commit = [&](int viaregs, unsigned char* tA, unsigned char* tB) {
    if (viaregs & 1) store_tile<T, A_KC>(tA, ra, tid);
    if (viaregs & 2) store_tile<T, B_KC>(tB, rb, tid);
  };
  if (nk > 0) {
    const int v = stage_issue(0, smem, smem + OPER_BYTES);
    stage_commit(v, smem, smem + OPER_BYTES);
    __syncthreads();
  }
  for (int kt = 0; kt < nk; ++kt) {
    unsigned char* tA = smem + (kt & 1) * 2 * OPER_BYTES;
    unsigned char* tB = tA + OPER_BYTES;
    unsigned char* nA = smem + ((kt + 1) & 1) * 2 * OPER_BYTES;
    unsigned char* nB = nA + OPER_BYTES;
    int v = 0;
#ifdef IB_ABLATE
    if (kt + 1 < nk && !(p.ablate & 1)) v = stage_issue(kt + 1, nA, nB);
    if (!(p.ablate & 4)) compute_tile<T, A_KC, B_KC>(tA, tB, acc, lane, wi, wj);
    if (kt + 1 < nk && !(p.ablate & 2)) stage_commit(v, nA, nB);
#else
    if (kt + 1 < nk) v = stage_issue(kt + 1, nA, nB);
    compute_tile<T, A_KC, B_KC>(tA, tB, acc, lane, wi, wj);
    if (kt + 1 < nk) stage_commit(v, nA, nB);
#endif
    __syncthreads();   // also drains the in-flight global_load_lds (hipcc emits vmcnt(0) before the barrier)
  }
#ifdef IB_ABLATE
  if (p.ablate & 8) return;
#endif

  // ---- epilogue: lane holds C[i][jb..jb+3] for 16 (t,u) sub-tiles.  The activation is a compile-time
  // parameter of the epilogue body (one uniform switch here), so only the selected math is executed.
  if constexpr (EPI == EPI_WGRAD) {
    epilogue<T, EPI, IB_ACT_NONE>(p, acc, i0, j0, wi, wj, lane, split_id);
    return;
  }
  switch (p.act) {
    case IB_ACT_RELU: epilogue<T, EPI, IB_ACT_RELU>(p, acc, i0, j0, wi, wj, lane, split_id); break;
    case IB_ACT_TANH: epilogue<T, EPI, IB_ACT_TANH>(p, acc, i0, j0, wi, wj, lane, split_id); break;
    case IB_ACT_SIGMOID: epilogue<T, EPI, IB_ACT_SIGMOID>(p, acc, i0, j0, wi, wj, lane, split_id); break;
    case IB_ACT_SILU: epilogue<T, EPI, IB_ACT_SILU>(p, acc, i0, j0, wi, wj, lane, split_id); break;
    case IB_ACT_ELU: epilogue<T, EPI, IB_ACT_ELU>(p, acc, i0, j0, wi, wj, lane, split_id); break;
    default: epilogue<T, EPI, IB_ACT_NONE>(p, acc, i0, j0, wi, wj, lane, split_id); break;
  }
}

// ---- ring-pipelined variant (bf16, every operand piece 16-byte aligned, reduction a multiple of 32) -------------
// The kernel above stages ONE K step ahead and its __syncthreads() drains the in-flight loads (vmcnt(0)): every K
// step exposes a full L2/HBM round trip, ~1.2 us per 64-deep step at these sizes.  Here the operands go HBM/L2 -> LDS
// by global_load_lds only, into a ring of four 32-deep stages: three stages (2 x 54 KiB per CU at 2 workgroups/CU) are
// in flight while one is consumed, each wave waits for ITS OWN pieces of the stage with a counted s_waitcnt vmcnt(N),
// and the workgroup barrier is the raw s_barrier (no vmcnt(0) drain).  One barrier per K step:
//   wait(stage kt landed, mine) ; barrier (everyone's landed; everyone is done reading stage kt-1)
//   issue stage kt+3 into the slot stage kt-1 occupied ; MFMAs on stage kt.
// Out-of-range tile rows/columns are CLAMPED onto valid memory (they only feed outputs that are never stored); the
// reduction range itself must be exact (no zero fill with LDS-DMA), so ragged reductions use the kernel above.
namespace ring {
constexpr int BK = 32, NS = 4, KCS = 40;                   // KC image: 128 rows x (32 + 8 pad) bf16 = 10 chunks of 1 KiB
constexpr int KC_BYTES = 128 * KCS * 2, KS_BYTES = BK * Tile<bf16_t>::KS_STRIDE * 2;   // 10240 / 9216
template <bool KC> constexpr int chunks() { return (KC ? KC_BYTES : KS_BYTES) / 1024; }

// per-lane global element offsets of the (up to 3) chunks wave `w` stages for one operand tile
template <bool KC>
__device__ __forceinline__ void offsets(int64_t ld, int row0, int rows_total, int wave, int lane, int64_t (&off)[3]) {
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int chunk = wave + 4 * j;
    const int o = (chunk < chunks<KC>() ? chunk : 0) * 1024 + lane * 16;
    if (KC) {
      const int row = o / (KCS * 2), c = min((o % (KCS * 2)) / 16, 3);
      off[j] = (int64_t)min(row0 + row, rows_total - 1) * ld + 8 * c;
    } else {
      const int kk = o / 288, c = min((o % 288) / 16, 15);
      off[j] = (int64_t)kk * ld + min((int64_t)row0 + 8 * c, ld - 8);
    }
  }
}
template <bool KC>
__device__ __forceinline__ void issue(const bf16_t* base, const int64_t (&off)[3], int64_t koff, unsigned char* tile, int wave) {
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int chunk = wave + 4 * j;
    if (chunk < chunks<KC>())
      __builtin_amdgcn_global_load_lds((glb_void_t*)(base + off[j] + koff), (lds_void_t*)(tile + chunk * 1024), 16, 0, 0);
  }
}
template <bool KC> __device__ __forceinline__ int per_wave(int wave) { return (chunks<KC>() - wave + 3) / 4; }

// LDS fragment reads as inline asm (wave_prims.h): ordered by hand -- the counted vmcnt + barrier above them, one
// lgkmcnt(0) (frags_ready) below them
template <bool KC>
__device__ __forceinline__ bf16x8_t read_frag_asm(const unsigned char* tile, int rbase, int lane) {
  if (KC) {
    return lds_read16<0>(lds_off(tile) + ((rbase + (lane & 15)) * KCS + 8 * (lane >> 4)) * 2);
  } else {
    const int q = (lane & 15) >> 2, pp = lane & 3;
    const int kr = 8 * (lane >> 4) + q;
    return lds_read_tr<0, 4 * Tile<bf16_t>::KS_STRIDE * 2>(lds_off(tile) + (kr * Tile<bf16_t>::KS_STRIDE + rbase + 4 * pp) * 2);
  }
}
__device__ __forceinline__ void wait_vmcnt(int n) {      // n is wave-uniform, one of {0, 4, 5, 6, 8, 10, 12}
  switch (n) {
    case 0: wait_vm<0>(); break;
    case 4: wait_vm<4>(); break;
    case 5: wait_vm<5>(); break;
    case 6: wait_vm<6>(); break;
    case 8: wait_vm<8>(); break;
    case 10: wait_vm<10>(); break;
    default: wait_vm<12>(); break;
  }
}
}  // namespace ring

template <bool A_KC, bool B_KC>
constexpr int ring_lds_bytes() {
  return ring::NS * ((A_KC ? ring::KC_BYTES : ring::KS_BYTES) + (B_KC ? ring::KC_BYTES : ring::KS_BYTES));
}
// blk / nblk: this problem's block id and block count (== blockIdx.x / gridDim.x unless several problems share a launch)
template <bool A_KC, bool B_KC, int EPI>
__device__ __forceinline__ void gemm_ring_body(const GemmParams& p, unsigned char* smem, int blk, int nblk) {
  using namespace ring;
  constexpr int A_BYTES = A_KC ? KC_BYTES : KS_BYTES, B_BYTES = B_KC ? KC_BYTES : KS_BYTES, STAGE = A_BYTES + B_BYTES;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wi = wave >> 1, wj = wave & 1;
  const int bid = p.xcd_group ? ib_xcd_remap(blk, nblk) : blk;
  const int tiles_total = p.tiles_m * p.tiles_n;
  const int split_id = bid / tiles_total, tile_id = bid % tiles_total;
  const int ti = tile_id / p.tiles_n, tj = tile_id % p.tiles_n;
  const int i0 = ti * BM, j0 = tj * BN;
  const int kb = split_id * p.k_chunk;
  const int ke = min(p.K, kb + p.k_chunk);
  const int nk = (ke - kb) / BK;                            // exact by the launch conditions
  const bf16_t* A = reinterpret_cast<const bf16_t*>(p.A);
  const bf16_t* B = reinterpret_cast<const bf16_t*>(p.B);

  f32x4_t acc[4][4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[t][u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  // weight gradient: the bias gradient rides along.  sum_k A(i,k) = one more MFMA per row tile against an all-ones
  // fragment (+25 % matrix work in the blocks of column tile 0, left wave column only): it replaces a column-sum launch
  // over the whole dz matrix per Linear layer.
  [[maybe_unused]] f32x4_t accb[4];
  [[maybe_unused]] bool do_bias = false;
  [[maybe_unused]] bf16x8_t ones;
  if constexpr (EPI == EPI_WGRAD) {
    do_bias = p.dbias_part != nullptr && tj == 0 && wj == 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) accb[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = (bf16_t)1.0f;
  }

  IB_STAMP(p.prof, 8, 0, tid == 0);
  int64_t oa[3], ob[3];
  offsets<A_KC>(p.lda, i0, p.M, wave, lane, oa);
  offsets<B_KC>(p.ldb, j0, p.N, wave, lane, ob);
  const int per = per_wave<A_KC>(wave) + per_wave<B_KC>(wave);   // this wave's LDS-DMA instructions per stage
  auto stage = [&](int kt) {
    unsigned char* tA = smem + (kt % NS) * STAGE;
    const int k0 = kb + kt * BK;
    issue<A_KC>(A, oa, A_KC ? (int64_t)k0 : (int64_t)k0 * p.lda, tA, wave);
    issue<B_KC>(B, ob, B_KC ? (int64_t)k0 : (int64_t)k0 * p.ldb, tA + A_BYTES, wave);
  };
  for (int s = 0; s < NS - 1 && s < nk; ++s) stage(s);
  IB_STAMP(p.prof, 8, 1, tid == 0);
  for (int kt = 0; kt < nk; ++kt) {
    wait_vmcnt(min(nk - 1 - kt, NS - 2) * per);             // my pieces of stage kt have landed
    __builtin_amdgcn_s_barrier();                            // everyone's have; everyone finished reading stage kt-1
    if (kt == 0) IB_STAMP(p.prof, 8, 2, tid == 0);
    if (kt + NS - 1 < nk) stage(kt + NS - 1);
    const unsigned char* tA = smem + (kt % NS) * STAGE;
    const unsigned char* tB = tA + A_BYTES;
    bf16x8_t fa[4], fb[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) fa[t] = read_frag_asm<A_KC>(tA, wi * 64 + 16 * t, lane);
#pragma unroll
    for (int u = 0; u < 4; ++u) fb[u] = read_frag_asm<B_KC>(tB, wj * 64 + 16 * u, lane);
    frags_ready(fa, fb);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int u = 0; u < 4; ++u)
        acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[u], fa[t], acc[t][u], 0, 0, 0);
    if constexpr (EPI == EPI_WGRAD) {
      if (do_bias) {
#pragma unroll
        for (int t = 0; t < 4; ++t) accb[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, fa[t], accb[t], 0, 0, 0);
      }
    }
  }
  IB_STAMP(p.prof, 8, 3, tid == 0);
  if constexpr (EPI == EPI_WGRAD) {
    if (do_bias && (lane >> 4) == 0) {         // every output column holds the same sum: column 0 of each row tile
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int i = i0 + wi * 64 + 16 * t + (lane & 15);
        if (i < p.M) p.dbias_part[(int64_t)split_id * p.M + i] = accb[t][0];
      }
    }
    epilogue<bf16_t, EPI, IB_ACT_NONE>(p, acc, i0, j0, wi, wj, lane, split_id);
    IB_STAMP(p.prof, 8, 4, tid == 0);
    return;
  }
  switch (p.act) {
    case IB_ACT_RELU: epilogue<bf16_t, EPI, IB_ACT_RELU>(p, acc, i0, j0, wi, wj, lane, split_id); break;
    case IB_ACT_TANH: epilogue<bf16_t, EPI, IB_ACT_TANH>(p, acc, i0, j0, wi, wj, lane, split_id); break;
    case IB_ACT_SIGMOID: epilogue<bf16_t, EPI, IB_ACT_SIGMOID>(p, acc, i0, j0, wi, wj, lane, split_id); break;
    case IB_ACT_SILU: epilogue<bf16_t, EPI, IB_ACT_SILU>(p, acc, i0, j0, wi, wj, lane, split_id); break;
    case IB_ACT_ELU: epilogue<bf16_t, EPI, IB_ACT_ELU>(p, acc, i0, j0, wi, wj, lane, split_id); break;
    default: epilogue<bf16_t, EPI, IB_ACT_NONE>(p, acc, i0, j0, wi, wj, lane, split_id); break;
  }
  IB_STAMP(p.prof, 8, 4, tid == 0);
}

template <bool A_KC, bool B_KC, int EPI>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_ring_kernel(GemmParams p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[ring_lds_bytes<A_KC, B_KC>()];
  gemm_ring_body<A_KC, B_KC, EPI>(p, smem, (int)blockIdx.x, (int)gridDim.x);
}

// several weight-gradient problems in ONE launch (a training step's dW GEMMs are independent and each is short: one
// launch saves their kernel boundaries and the streams / joins that ran them side by side)
constexpr int WG_MAX = 6;
struct WgradMulti { GemmParams p[WG_MAX]; int blk0[WG_MAX + 1]; int n; };
__global__ __launch_bounds__(NTHREADS, 2) void gemm_ring_wgrad_multi_kernel(WgradMulti m) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[ring_lds_bytes<false, false>()];
  int e = 0;
  for (int j = 1; j < m.n; ++j)
    if ((int)blockIdx.x >= m.blk0[j]) e = j;
  gemm_ring_body<false, false, EPI_WGRAD>(m.p[e], smem, (int)blockIdx.x - m.blk0[e], m.blk0[e + 1] - m.blk0[e]);
}

// out[e] (+)= sum_s slab[s][e]   (fixed order -> bitwise reproducible).  float4 per thread, 4 slabs in flight.
__global__ __launch_bounds__(256) void slab_reduce_kernel(const float* __restrict__ slabs, int nslab, int64_t slab_stride,
                                                          float* __restrict__ out, int64_t ldo, int rows, int cols,
                                                          int accumulate, int vec) {
  const int64_t n = (int64_t)rows * cols;
  if (vec) {   // cols % 4 == 0, slab_stride % 4 == 0, ldo % 4 == 0, 16-byte aligned bases
    const int64_t n4 = n >> 2;
    for (int64_t e4 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e4 < n4; e4 += (int64_t)gridDim.x * blockDim.x) {
      const float4* p = reinterpret_cast<const float4*>(slabs) + e4;
      const int64_t st4 = slab_stride >> 2;
      float4 s = ib_slab_sum4(p, st4, nslab);
      const int64_t e = e4 << 2;
      const int r = (int)(e / cols), c0 = (int)(e % cols);
      float4* o = reinterpret_cast<float4*>(out + (int64_t)r * ldo + c0);
      if (accumulate) { const float4 t = *o; s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w; }
      *o = s;
    }
    return;
  }
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    float s = 0.f;
    for (int k = 0; k < nslab; ++k) s += slabs[(int64_t)k * slab_stride + e];
    const int r = (int)(e / cols), c = (int)(e % cols);
    float* o = out + (int64_t)r * ldo + c;
    *o = accumulate ? (*o + s) : s;
  }
}

template <typename T> bool vec_load_ok(const void* p, int64_t ld) {
  return ib_aligned(p, 4) && ((ld * (int64_t)sizeof(T)) % 4 == 0);
}
template <typename T> bool glds_ok(const void* p, int64_t ld) {
  return sizeof(T) == 2 && ib_aligned(p, 16) && (ld % 8 == 0);
}
template <typename T> bool vec_store_ok(const void* p, int64_t ld) {
  return ib_aligned(p, 4 * sizeof(T)) && (ld % 4 == 0);
}

// `group`: number of problems sharing the launch (ib_linear_wgrad_slabs_multi).  Each gets ~512 / group workgroups,
// i.e. the LAUNCH fills the chip twice over instead of every problem doing so: half the slab bytes written here and
// read back by the reduction (headline step, 4 problems: 0.2403 -> 0.2354 ms at 128 per problem; 96: 0.243, 64: 0.258)
int wgrad_split(int64_t M, int64_t N, int64_t K, int* chunk_out, int group = 1) {
  // reduction length is M; output tiles over [N, K]
  const int64_t tiles = ((N + BM - 1) / BM) * ((K + BN - 1) / BN);
  static const int env_target = ib_ab_int("IB_WGRAD_TARGET", 0);
  const int target = env_target ? env_target : (group <= 1 ? 256 : (group >= 4 ? 128 : 512 / group));
  // ~1 workgroup per CU: with the ring-pipelined main loop fewer, longer slices win (half the slab traffic; measured
  // step 0.310 -> 0.305 ms against 2 per CU).  IB_WGRAD_TARGET: tuning override.
  int64_t want = (target + tiles - 1) / tiles;
  if (want < 1) want = 1;
  if (want > 32) want = 32;
  int64_t chunk = (M + want - 1) / want;
  chunk = ((chunk + 63) / 64) * 64;  // multiple of both BKs
  if (chunk < 64) chunk = 64;
  const int64_t split = (M + chunk - 1) / chunk;
  *chunk_out = (int)chunk;
  return (int)split;
}

// ring kernel: bf16 (gldsA / gldsB are set for no other dtype), every staged piece 16-byte aligned, exact reduction tiling
// of the whole reduction p.K and of each split's p.k_chunk, >= 2 K steps of 32
bool ring_ok(const GemmParams& p) {
  static const int off = ib_ab_int("IB_NO_RING", 0);
  return !off && p.gldsA && p.gldsB && p.K % 32 == 0 && p.k_chunk % 32 == 0 && p.K >= 64 && p.lda >= 8 && p.ldb >= 8;
}

// the fields that do not depend on the operand layout, for a problem whose A, B, M, N are set: staging legality of the
// two operands for element type T (no direct-to-LDS staging in fp32), tile counts, the measurement hooks
template <typename T>
void fill_common(GemmParams& p) {
  p.ablate = IB_ABLATE; p.prof = IB_AB_PROF(g_gemm_prof);
  p.vecA = vec_load_ok<T>(p.A, p.lda); p.vecB = vec_load_ok<T>(p.B, p.ldb);
  p.gldsA = glds_ok<T>(p.A, p.lda); p.gldsB = glds_ok<T>(p.B, p.ldb);
  p.tiles_n = (p.N + BN - 1) / BN; p.tiles_m = (p.M + BM - 1) / BM;
}

// `blocks` workgroups of the ring kernel where it qualifies (bf16, ring_ok), of the register-staged kernel elsewhere
template <typename T, bool A_KC, bool B_KC, int EPI>
int launch_ring_or_generic(const GemmParams& p, int blocks, hipStream_t s) {
  if constexpr (sizeof(T) == 2) {
    if (ring_ok(p)) {
      IB_PATH(IB_PATH_RING);
      hipLaunchKernelGGL((gemm_ring_kernel<A_KC, B_KC, EPI>), dim3(blocks), dim3(NTHREADS), 0, s, p);
      IB_CHECK_LAUNCH();
      return IB_OK;
    }
  }
  IB_PATH(IB_PATH_GENERIC);
  hipLaunchKernelGGL((gemm_kernel<T, A_KC, B_KC, EPI>), dim3(blocks), dim3(NTHREADS), 0, s, p);
  IB_CHECK_LAUNCH();
  return IB_OK;
}

template <typename T>
int launch_fwd(GemmParams& p, hipStream_t s) {
  fill_common<T>(p);
  p.vecC = vec_store_ok<T>(p.C, p.ldc) && (!p.Z || vec_store_ok<T>(p.Z, p.ldz));
  p.vecBias = !p.bias || ib_aligned(p.bias, 16);
  p.vecAdd = (!p.add_div || vec_store_ok<T>(p.add_div, p.ld_add_div)) &&
             (!p.add_mod || vec_store_ok<T>(p.add_mod, p.ld_add_mod));
  p.k_chunk = p.K; p.slab_stride = 0; p.xcd_group = 1;
  return launch_ring_or_generic<T, true, true, EPI_FWD>(p, p.tiles_m * p.tiles_n, s);
}

template <typename T>
int launch_dgrad(GemmParams& p, hipStream_t s) {
  fill_common<T>(p);
  p.vecC = vec_store_ok<T>(p.C, p.ldc);
  p.vecAux = !p.aux || vec_store_ok<T>(p.aux, p.ldaux);
  p.vecAdd = !p.addend || vec_store_ok<T>(p.addend, p.ldadd);
  p.k_chunk = p.K; p.slab_stride = 0; p.xcd_group = 1;
  return launch_ring_or_generic<T, true, false, EPI_DGRAD>(p, p.tiles_m * p.tiles_n, s);
}

}  // namespace

#ifdef IB_AB
extern "C" int ib_debug_set_ablate(int mask) { g_ablate = mask; return IB_OK; }
extern "C" int ib_debug_set_gemm_prof(void* buf) { g_gemm_prof = reinterpret_cast<long long*>(buf); return IB_OK; }
#else       // measurement builds only (lib/ab/libib_hip_ab.so)
extern "C" int ib_debug_set_ablate(int) { return IB_E_UNSUPPORTED; }
extern "C" int ib_debug_set_gemm_prof(void*) { return IB_E_UNSUPPORTED; }
#endif

extern "C" int ib_linear_fwd(const void* x, int64_t ldx, const void* w, int64_t ldw, const float* bias,
                             const void* add_div, int64_t ld_add_div, const void* add_mod,
                             int64_t ld_add_mod, int64_t seg, int act, void* y, int64_t ldy, void* z,
                             int64_t ldz, int64_t M, int64_t N, int64_t K, int dtype, ib_stream_t stream) {
  if (!x || !w || !y || M <= 0 || N <= 0 || K <= 0 || ldx < K || ldw < K || ldy < N) return IB_E_ARG;
  if ((add_div || add_mod) && seg <= 0) return IB_E_ARG;
  if (z && ldz < N) return IB_E_ARG;
  if (act < IB_ACT_NONE || act > IB_ACT_ELU) return IB_E_ARG;
  GemmParams p{};
  p.A = x; p.lda = ldx; p.B = w; p.ldb = ldw; p.M = (int)M; p.N = (int)N; p.K = (int)K;
  p.C = y; p.ldc = ldy; p.Z = z; p.ldz = ldz; p.bias = bias;
  p.add_div = add_div; p.ld_add_div = ld_add_div; p.add_mod = add_mod; p.ld_add_mod = ld_add_mod;
  p.seg = (int)(seg > 0 ? seg : 1); p.act = act;
  if (dtype == IB_BF16 && !add_div && !add_mod && !z) {       // large-M training shapes: the 256 x 128 NT kernel
    const int rc = ib_gemm_nt_try(x, ldx, w, ldw, y, ldy, bias, act, nullptr, 0, IB_ACT_NONE, nullptr, 0, M, N, K, ib_s(stream));
    if (rc != IB_E_UNSUPPORTED) return rc;
  }
  if (dtype == IB_F32 && !add_div && !add_mod) {              // the reference's own batch sizes in fp32: reduction-split tiles
    const int rc = ib_f32_small_fwd_try((const float*)x, ldx, (const float*)w, ldw, bias, act, (float*)y, ldy, (float*)z, ldz,
                                        M, N, K, ib_s(stream));
    if (rc != IB_E_UNSUPPORTED) return rc;
  }
  if (dtype == IB_BF16) {                                     // a few hundred rows: 64 x 16 tiles (gemm_small.hip)
    const int rc = ib_bf16_small_fwd_try(x, ldx, w, ldw, bias, add_div, ld_add_div, add_mod, ld_add_mod, p.seg, act, y, ldy, z,
                                         M, N, K, ib_s(stream));
    if (rc != IB_E_UNSUPPORTED) return rc;
  }
  if (dtype == IB_F32) return launch_fwd<float>(p, ib_s(stream));
  if (dtype == IB_BF16) return launch_fwd<bf16_t>(p, ib_s(stream));
  return IB_E_DTYPE;
}

extern "C" int ib_linear_dgrad(const void* dz, int64_t lddz, const void* w, int64_t ldw, int act_below,
                               const void* aux, int64_t ldaux, const void* addend, int64_t ldadd, void* dx,
                               int64_t lddx, int64_t M, int64_t N, int64_t K, int dtype, ib_stream_t stream) {
  if (!dz || !w || !dx || M <= 0 || N <= 0 || K <= 0 || lddz < N || ldw < K || lddx < K) return IB_E_ARG;
  if (addend && ldadd < K) return IB_E_ARG;
  if (act_below != IB_ACT_NONE && (!aux || ldaux < K)) return IB_E_ARG;
  if (act_below < IB_ACT_NONE || act_below > IB_ACT_ELU) return IB_E_ARG;
  // C[M,K] = sum_n dz[m][n] * w[n][k]:  reduction length N, B(j=k, kk=n) = w[n*ldw + k]  (k-strided)
  GemmParams p{};
  p.A = dz; p.lda = lddz; p.B = w; p.ldb = ldw; p.M = (int)M; p.N = (int)K; p.K = (int)N;
  p.C = dx; p.ldc = lddx; p.aux = aux; p.ldaux = ldaux; p.act = act_below; p.seg = 1;
  p.addend = addend; p.ldadd = ldadd;
  if (dtype == IB_F32) {
    const int rc = ib_f32_small_dgrad_try((const float*)dz, lddz, (const float*)w, ldw, act_below, (const float*)aux, ldaux,
                                          (const float*)addend, ldadd, (float*)dx, lddx, M, N, K, ib_s(stream));
    if (rc != IB_E_UNSUPPORTED) return rc;
  }
  if (dtype == IB_BF16) {
    const int rc = ib_bf16_small_dgrad_try(dz, lddz, w, ldw, act_below, aux, ldaux, addend, dx, lddx, M, N, K, ib_s(stream));
    if (rc != IB_E_UNSUPPORTED) return rc;
  }
  if (dtype == IB_F32) return launch_dgrad<float>(p, ib_s(stream));
  if (dtype == IB_BF16) return launch_dgrad<bf16_t>(p, ib_s(stream));
  return IB_E_DTYPE;
}

// The same product with the weight handed over TRANSPOSED (wt[K,N], k-contiguous along the reduction): both operands are
// then "NT" and large-M problems take the 256 x 128 kernel of gemm_nt.hip.  IB_E_UNSUPPORTED (nothing launched) when the
// problem does not qualify -- callers fall back to ib_linear_dgrad with the untransposed weight.
extern "C" int ib_linear_dgrad_wt(const void* dz, int64_t lddz, const void* wt, int64_t ldwt, int act_below, const void* aux,
                                  int64_t ldaux, const void* addend, int64_t ldadd, void* dx, int64_t lddx, int64_t M,
                                  int64_t N, int64_t K, int dtype, ib_stream_t stream) {
  if (!dz || !wt || !dx || M <= 0 || N <= 0 || K <= 0 || lddz < N || ldwt < N || lddx < K) return IB_E_ARG;
  if (addend && ldadd < K) return IB_E_ARG;
  if (act_below != IB_ACT_NONE && (!aux || ldaux < K)) return IB_E_ARG;
  if (dtype != IB_BF16) return IB_E_UNSUPPORTED;
  // C[M,K] = sum_n dz[m][n] * wt[k][n]
  return ib_gemm_nt_try(dz, lddz, wt, ldwt, dx, lddx, nullptr, IB_ACT_NONE, aux, ldaux, act_below, addend, ldadd, M, K, N,
                        ib_s(stream));
}

extern "C" int ib_linear_dgrad_skinny(const void* dz, int64_t lddz, const void* w, int64_t ldw, int act_below,
                                      const void* aux, int64_t ldaux, void* dx, int64_t lddx, float* dbias, int accumulate,
                                      int64_t M, int64_t N, int64_t K, int dtype, ib_stream_t stream) {
  if (!dz || !w || !dx || M <= 0 || N <= 0 || K <= 0 || lddz < N || ldw < K || lddx < K) return IB_E_ARG;
  if (act_below != IB_ACT_NONE && (!aux || ldaux < K)) return IB_E_ARG;
  if (act_below < IB_ACT_NONE || act_below > IB_ACT_ELU) return IB_E_ARG;
  return ib_skinny_dgrad_try(dz, lddz, w, ldw, act_below, aux, ldaux, dx, lddx, dbias, accumulate, M, N, K, dtype, ib_s(stream));
}

extern "C" size_t ib_linear_wgrad_workspace(int64_t M, int64_t N, int64_t K) {
  int chunk;
  const int split = wgrad_split(M, N, K, &chunk);
  return split > 1 ? (size_t)split * (size_t)N * (size_t)K * sizeof(float) : 0;
}

namespace {
// fills the GemmParams of dW = dz^T x (split over M); returns the error code, *split_out on success
int wgrad_params(const void* dz, int64_t lddz, const void* x, int64_t ldx, float* dw, int64_t lddw, int accumulate,
                 void* workspace, size_t workspace_bytes, int64_t M, int64_t N, int64_t K, int dtype, bool slabs_only,
                 GemmParams& p, int* split_out, int group = 1) {
  if (!dz || !x || M <= 0 || N <= 0 || K <= 0 || lddz < N || ldx < K) return IB_E_ARG;
  if (!slabs_only && (!dw || lddw < K)) return IB_E_ARG;
  if (dtype != IB_F32 && dtype != IB_BF16) return IB_E_DTYPE;
  int chunk;
  const int split = wgrad_split(M, N, K, &chunk, group);
  const bool to_ws = slabs_only || split > 1;
  const size_t need = to_ws ? (size_t)split * (size_t)N * (size_t)K * sizeof(float) : 0;
  if (need > 0 && (!workspace || workspace_bytes < need)) return IB_E_WORKSPACE;
  // C[N,K] = sum_m dz[m][n] * x[m][k]: A(i=n, kk=m) = dz[m*lddz + n], B(j=k, kk=m) = x[m*ldx + k]
  p = GemmParams{};
  p.A = dz; p.lda = lddz; p.B = x; p.ldb = ldx; p.M = (int)N; p.N = (int)K; p.K = (int)M;
  p.seg = 1; p.act = IB_ACT_NONE; p.accumulate = accumulate;
  if (dtype == IB_F32) fill_common<float>(p); else fill_common<bf16_t>(p);
  p.k_chunk = chunk;
  // all tiles of one M-chunk on one XCD only while that chunk's dz + x slices fit comfortably in the XCD's 4 MiB
  // L2 (measured: [12800,512,300] 42 -> 36 us grouped, but [12800,1536,512] 48 -> 63 us: 5.2 MB per chunk thrashes)
  p.xcd_group = ((int64_t)chunk * (N + K) * (dtype == IB_BF16 ? 2 : 4) <= (2 << 20)) ? 1 : 0;
  if (to_ws) {
    p.C = workspace; p.ldc = K; p.slab_stride = (int64_t)N * K; p.accumulate = 0;
  } else {
    p.C = dw; p.ldc = lddw; p.slab_stride = 0;
  }
  p.vecC = ib_aligned(p.C, 16) && (p.ldc % 4 == 0) && (p.slab_stride % 4 == 0);
  *split_out = split;
  return IB_OK;
}

// the split-M weight-gradient GEMM.  slabs_only: always write fp32 partial slabs [split][N][K] into the workspace
// (even for split == 1) and leave the reduction to ib_slab_reduce_multi (one launch for several gradients).
int wgrad_gemm(const void* dz, int64_t lddz, const void* x, int64_t ldx, float* dw, int64_t lddw, int accumulate,
               void* workspace, size_t workspace_bytes, int64_t M, int64_t N, int64_t K, int dtype, hipStream_t s,
               bool slabs_only, int* split_out) {
  GemmParams p;
  int split;
  const int rc = wgrad_params(dz, lddz, x, ldx, dw, lddw, accumulate, workspace, workspace_bytes, M, N, K, dtype,
                              slabs_only, p, &split);
  if (rc != IB_OK) return rc;
  const int blocks = p.tiles_m * p.tiles_n * split;
  const int lrc = dtype == IB_F32 ? launch_ring_or_generic<float, false, false, EPI_WGRAD>(p, blocks, s)
                                  : launch_ring_or_generic<bf16_t, false, false, EPI_WGRAD>(p, blocks, s);
  if (lrc != IB_OK) return lrc;
  if (split_out) *split_out = split;
  if (!slabs_only && split > 1) {
    const int64_t n = (int64_t)N * K;
    const int rvec = (K % 4 == 0) && (lddw % 4 == 0) && ib_aligned(workspace, 16) && ib_aligned(dw, 16);
    hipLaunchKernelGGL(slab_reduce_kernel, dim3(ib_grid_1d(rvec ? n / 4 : n, 256)), dim3(256), 0, s,
                       reinterpret_cast<const float*>(workspace), split, (int64_t)N * K, dw, lddw, (int)N, (int)K,
                       accumulate, rvec);
    IB_CHECK_LAUNCH();
  }
  return IB_OK;
}

// the problem count and the per-problem arrays of a grouped weight-gradient entry
bool wgrad_group_args_ok(int n, const void* const* dz, const int64_t* lddz, const void* const* x, const int64_t* ldx,
                         void* const* workspace, const size_t* workspace_bytes, const int32_t* nslab_out, const int64_t* M,
                         const int64_t* N, const int64_t* K) {
  return n > 0 && n <= WG_MAX && dz && lddz && x && ldx && workspace && workspace_bytes && nslab_out && M && N && K;
}

}  // namespace

extern "C" int ib_linear_wgrad(const void* dz, int64_t lddz, const void* x, int64_t ldx, float* dw,
                               int64_t lddw, int accumulate, void* workspace, size_t workspace_bytes,
                               int64_t M, int64_t N, int64_t K, int dtype, ib_stream_t stream) {
  if (dz && x && dw && M > 0 && N > 0 && K > 0 && lddz >= N && ldx >= K && lddw >= K) {     // short reduction: one pass
    const int rc = ib_wgrad_small_try(dz, lddz, x, ldx, dw, lddw, nullptr, accumulate, M, N, K, dtype, ib_s(stream));
    if (rc != IB_E_UNSUPPORTED) return rc;
  }
  return wgrad_gemm(dz, lddz, x, ldx, dw, lddw, accumulate, workspace, workspace_bytes, M, N, K, dtype, ib_s(stream),
                    false, nullptr);
}

extern "C" int ib_linear_wgrad_bias(const void* dz, int64_t lddz, const void* x, int64_t ldx, float* dw, int64_t lddw,
                                    float* dbias, int accumulate, int64_t M, int64_t N, int64_t K, int dtype,
                                    ib_stream_t stream) {
  if (!dz || !x || !dw || !dbias || M <= 0 || N <= 0 || K <= 0 || lddz < N || ldx < K || lddw < K) return IB_E_ARG;
  if (dtype == IB_F32)                                      // the reference's batch sizes in fp32 (gemm_f32_small.hip)
    return ib_f32_small_wgrad_bias_try((const float*)dz, lddz, (const float*)x, ldx, dw, lddw, dbias, accumulate, M, N, K,
                                       ib_s(stream));
  return ib_wgrad_small_try(dz, lddz, x, ldx, dw, lddw, dbias, accumulate, M, N, K, dtype, ib_s(stream));
}

extern "C" size_t ib_linear_wgrad_slabs_workspace(int64_t M, int64_t N, int64_t K) {
  int chunk;
  int split = wgrad_split(M, N, K, &chunk);
  const int tn = ib_gemm_tn_splits(M, N, K, 1);              // the 256 x 128 kernel (gemm_tn.hip) splits finest when alone
  if (tn > split) split = tn;
  return (size_t)split * (size_t)N * (size_t)K * sizeof(float);
}

extern "C" int ib_linear_wgrad_slabs(const void* dz, int64_t lddz, const void* x, int64_t ldx, void* workspace,
                                     size_t workspace_bytes, int* nslab_out, int64_t M, int64_t N, int64_t K,
                                     int dtype, ib_stream_t stream) {
  if (!nslab_out) return IB_E_ARG;
  if (dz && x && workspace && M > 0 && N > 0 && K > 0 && lddz >= N && ldx >= K && K % 4 == 0 &&
      workspace_bytes >= (size_t)N * K * sizeof(float) && ib_aligned(workspace, 16)) {
    // short reduction: the one-pass kernel writes the whole gradient as a single "slab"
    const int rc = ib_wgrad_small_try(dz, lddz, x, ldx, reinterpret_cast<float*>(workspace), K, nullptr, 0, M, N, K, dtype,
                                      ib_s(stream));
    if (rc == IB_OK) *nslab_out = 1;
    if (rc != IB_E_UNSUPPORTED) return rc;
  }
  if (dtype == IB_BF16 && dz && x && workspace && lddz >= N && ldx >= K) {      // long reduction: the 256 x 128 kernel
    const void* dzs[1] = {dz}; const void* xs[1] = {x}; void* wss[1] = {workspace};
    const int64_t la[1] = {lddz}, lx[1] = {ldx}, Ms[1] = {M}, Ns[1] = {N}, Ks[1] = {K};
    const size_t wb[1] = {workspace_bytes};
    int32_t ns = 0;
    const int rc = ib_gemm_tn_multi(1, dzs, la, xs, lx, wss, wb, nullptr, &ns, Ms, Ns, Ks, ib_s(stream));
    if (rc != IB_E_UNSUPPORTED) { *nslab_out = ns; return rc; }
  }
  return wgrad_gemm(dz, lddz, x, ldx, nullptr, 0, 0, workspace, workspace_bytes, M, N, K, dtype, ib_s(stream), true,
                    nslab_out);
}

extern "C" int ib_linear_wgrad_slabs_multi(int n, const void* const* dz, const int64_t* lddz, const void* const* x,
                                           const int64_t* ldx, void* const* workspace, const size_t* workspace_bytes,
                                           int32_t* nslab_out, const int64_t* M, const int64_t* N, const int64_t* K,
                                           int dtype, ib_stream_t stream) {
  return ib_linear_wgrad_slabs_multi_bias(n, dz, lddz, x, ldx, workspace, workspace_bytes, nullptr, nslab_out, M, N, K, dtype,
                                          stream);
}

extern "C" int ib_linear_wgrad_slabs_multi_bias(int n, const void* const* dz, const int64_t* lddz, const void* const* x,
                                                const int64_t* ldx, void* const* workspace, const size_t* workspace_bytes,
                                                float* const* dbias_part, int32_t* nslab_out, const int64_t* M,
                                                const int64_t* N, const int64_t* K, int dtype, ib_stream_t stream) {
  if (!wgrad_group_args_ok(n, dz, lddz, x, ldx, workspace, workspace_bytes, nslab_out, M, N, K)) return IB_E_ARG;
  if (dtype != IB_BF16) return IB_E_UNSUPPORTED;
  {   // long reductions: the 256 x 128 LDS-DMA kernel (half the operand re-reads of the 128 x 128 tiles)
    const int rc = ib_gemm_tn_multi(n, dz, lddz, x, ldx, workspace, workspace_bytes, dbias_part, nslab_out, M, N, K,
                                    ib_s(stream));
    if (rc != IB_E_UNSUPPORTED) return rc;
  }
  WgradMulti m{};
  m.n = n;
  int blocks = 0;
  for (int j = 0; j < n; ++j) {
    int split;
    const int rc = wgrad_params(dz[j], lddz[j], x[j], ldx[j], nullptr, 0, 0, workspace[j], workspace_bytes[j], M[j], N[j],
                                K[j], dtype, true, m.p[j], &split, n);
    if (rc != IB_OK) return rc;
    if (!ring_ok(m.p[j])) return IB_E_UNSUPPORTED;   // caller falls back to single launches
    m.p[j].dbias_part = dbias_part ? dbias_part[j] : nullptr;      // [IB_WGRAD_MAX_SPLIT][N] fp32, rows 0 .. split-1 written
    nslab_out[j] = split;
    m.blk0[j] = blocks;
    blocks += m.p[j].tiles_m * m.p[j].tiles_n * split;
  }
  m.blk0[n] = blocks;
  IB_PATH(IB_PATH_RING_MULTI);
  hipLaunchKernelGGL(gemm_ring_wgrad_multi_kernel, dim3(blocks), dim3(NTHREADS), 0, ib_s(stream), m);
  IB_CHECK_LAUNCH();
  return IB_OK;
}

// The grouped weight-gradient launch with the time-MLP's hidden-layer backward (ib_time_mlp_bwd) riding along as extra
// workgroups of the SAME launch (csrc/gemm_tn.hip).  IB_E_UNSUPPORTED = nothing launched: the caller issues
// ib_linear_wgrad_slabs_multi and ib_time_mlp_bwd separately.
extern "C" int ib_linear_wgrad_slabs_multi_tb(int n, const void* const* dz, const int64_t* lddz, const void* const* x,
                                              const int64_t* ldx, void* const* workspace, const size_t* workspace_bytes,
                                              int32_t* nslab_out, const int64_t* M, const int64_t* N, const int64_t* K,
                                              int dtype, const void* de, int64_t ld_de, const void* w2, int64_t ldw2,
                                              const void* zu, int64_t ldzu, const void* s_rows, int64_t lds, float* dw1_slabs,
                                              float* db1_slabs, int64_t B, int64_t temb, int64_t hidden, int64_t out,
                                              ib_stream_t stream) {
  if (!wgrad_group_args_ok(n, dz, lddz, x, ldx, workspace, workspace_bytes, nslab_out, M, N, K)) return IB_E_ARG;
  if (dtype != IB_BF16 || !ib_time_mlp_bwd_supported(temb, hidden, out)) return IB_E_UNSUPPORTED;
  if (!de || !w2 || !zu || !s_rows || !dw1_slabs || !db1_slabs || B <= 0) return IB_E_ARG;
  if (ld_de < out || ldw2 < hidden || ldzu < hidden || lds < temb || ld_de % 8 || ldw2 % 8 || lds % 8) return IB_E_ARG;
  if (!ib_al16({de, w2, s_rows, dw1_slabs, db1_slabs}) || !ib_aligned(zu, 2)) return IB_E_ARG;
  TimeBwdParams tb{(const bf16_t*)de, ld_de, (const bf16_t*)w2, ldw2, (const bf16_t*)zu, ldzu, (const bf16_t*)s_rows, lds,
                   dw1_slabs, db1_slabs, (int)B, (int)out, (int)hidden};
  return ib_gemm_tn_multi(n, dz, lddz, x, ldx, workspace, workspace_bytes, nullptr, nslab_out, M, N, K, ib_s(stream), &tb,
                          (int)temb);
}

// ---- y = LayerNorm(res + x W^T + b) for small token counts (the DDIM sampler: M = B*T = 3200): the GEMM is split over
// K into fp32 slabs so that a [3200, 512, 2048] problem fills the chip (25 x 4 tiles x 4 slices instead of 100
// workgroups walking 64 K steps each), and the slab reduction IS the LayerNorm kernel (bias + residual + statistics +
// affine), so the separate LayerNorm launch and the bf16 round trip of the GEMM output disappear.
namespace {
// N = 4 * LPR * NCH columns; LPR lanes per row, a lane holds NCH float4 (columns (c * LPR + l) * 4 ..).  Wide rows use a
// whole wave per row (3200 rows = 12 waves per CU; with 16 lanes per row the launch was 3 waves per CU and each lane
// walked 32 dependent-ish loads: 17 us for 26 MB)
template <int LPR, int NCH>
__global__ __launch_bounds__(256) void slab_ln_kernel(const float* __restrict__ slabs, int nslab, int64_t slab_stride,
                                                      const float* __restrict__ bias, const bf16_t* __restrict__ res,
                                                      int64_t ldres, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, bf16_t* __restrict__ y, int64_t ldy,
                                                      bf16_t* __restrict__ a_out, float* __restrict__ mean,
                                                      float* __restrict__ rstd, int M, float eps) {
  constexpr int N = 4 * LPR * NCH, RPB = 256 / LPR;
  const int l = threadIdx.x % LPR;
  const int row = blockIdx.x * RPB + threadIdx.x / LPR;
  if (row >= M) return;
  // Slabs in batches of up to SB requested together (predicated on the count), added strictly in slab order.  As a rolled
  // loop -- one slab per trip, the trip count a runtime value -- this was `nslab` memory round trips in sequence: at the
  // sampler's M = 200 (16 slabs of the FFN output projection) 10 of the Linear + LayerNorm pair's 17 us.
  constexpr int SB = NCH <= 2 ? 8 : 4;
  float4 v[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) v[c] = make_float4(0.f, 0.f, 0.f, 0.f);
  const float* srow = slabs + (int64_t)row * N + l * 4;
  for (int k0 = 0; k0 < nslab; k0 += SB) {
    float4 w[SB][NCH];
#pragma unroll
    for (int e = 0; e < SB; ++e)
      if (k0 + e < nslab) {
#pragma unroll
        for (int c = 0; c < NCH; ++c)
          w[e][c] = *reinterpret_cast<const float4*>(srow + (int64_t)(k0 + e) * slab_stride + c * LPR * 4);
      }
#pragma unroll
    for (int e = 0; e < SB; ++e)
      if (k0 + e < nslab) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          if (k0 + e == 0) v[c] = w[e][c];          // the first slab is taken as it is (0 + x would turn -0 into +0)
          else { v[c].x += w[e][c].x; v[c].y += w[e][c].y; v[c].z += w[e][c].z; v[c].w += w[e][c].w; }
        }
      }
  }
  float s1 = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = (c * LPR + l) * 4;
    float4 t = v[c];
    if (bias) { const float4 b = *reinterpret_cast<const float4*>(bias + col); t.x += b.x; t.y += b.y; t.z += b.z; t.w += b.w; }
    if (a_out) {      // the GEMM output itself (what the per-op plan stores between the two launches), bf16
      bf16x4_t o; o[0] = (bf16_t)t.x; o[1] = (bf16_t)t.y; o[2] = (bf16_t)t.z; o[3] = (bf16_t)t.w;
      *reinterpret_cast<bf16x4_t*>(a_out + (int64_t)row * N + col) = o;
      t.x = (float)o[0]; t.y = (float)o[1]; t.z = (float)o[2]; t.w = (float)o[3];
    }
    if (res) {
      const bf16x4_t r = *reinterpret_cast<const bf16x4_t*>(res + (int64_t)row * ldres + col);
      t.x += (float)r[0]; t.y += (float)r[1]; t.z += (float)r[2]; t.w += (float)r[3];
    }
    v[c] = t;
    s1 += (t.x + t.y) + (t.z + t.w);
  }
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) s1 += __shfl_xor(s1, o, 64);
  const float mu = s1 * (1.f / N);
  float s2 = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const float a = v[c].x - mu, b = v[c].y - mu, cc = v[c].z - mu, d = v[c].w - mu;
    s2 += (a * a + b * b) + (cc * cc + d * d);
  }
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) s2 += __shfl_xor(s2, o, 64);
  const float rs = 1.f / sqrtf(s2 * (1.f / N) + eps);
  if (l == 0) {
    if (mean) mean[row] = mu;
    if (rstd) rstd[row] = rs;
  }
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = (c * LPR + l) * 4;
    const float4 g = *reinterpret_cast<const float4*>(gamma + col), b = *reinterpret_cast<const float4*>(beta + col);
    bf16x4_t o;
    o[0] = (bf16_t)((v[c].x - mu) * rs * g.x + b.x); o[1] = (bf16_t)((v[c].y - mu) * rs * g.y + b.y);
    o[2] = (bf16_t)((v[c].z - mu) * rs * g.z + b.z); o[3] = (bf16_t)((v[c].w - mu) * rs * g.w + b.w);
    *reinterpret_cast<bf16x4_t*>(y + (int64_t)row * ldy + col) = o;
  }
}

int linear_ln_split(int64_t M, int64_t N, int64_t K, int* chunk_out) {
  const int64_t tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
  int64_t want = (384 + tiles - 1) / tiles;              // ~1.5 workgroups per CU
  if (want > K / 128) want = K / 128;                      // at least four 32-deep K steps per slice
  if (want < 1) want = 1;
  int64_t chunk = ((K + want - 1) / want + 31) / 32 * 32;
  *chunk_out = (int)chunk;
  return (int)((K + chunk - 1) / chunk);
}
}  // namespace

// the reduction / LayerNorm launch on its own, for N = 512: slabs of another producer (linln_panel.hip's feed-forward launch)
int ib_slab_ln512_launch(const float* slabs, int nslab, int64_t slab_stride, const float* bias, const void* res, int64_t ldres,
                         const float* gamma, const float* beta, void* y, int64_t ldy, int64_t M, float eps, hipStream_t s) {
  hipLaunchKernelGGL((slab_ln_kernel<64, 2>), dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, slabs, nslab, slab_stride, bias,
                     reinterpret_cast<const bf16_t*>(res), ldres, gamma, beta, reinterpret_cast<bf16_t*>(y), ldy,
                     (bf16_t*)nullptr, (float*)nullptr, (float*)nullptr, (int)M, eps);
  IB_CHECK_LAUNCH();
  return IB_OK;
}

extern "C" size_t ib_linear_ln_fwd_workspace(int64_t M, int64_t N, int64_t K) {
  int chunk;
  int split = linear_ln_split(M, N, K, &chunk);
  const int nt = ib_gemm_nt_splitk_splits(M, N, K);            // the 256 x 128 kernel's split-K form may use more slabs
  if (nt > split) split = nt;
  return (size_t)split * (size_t)M * (size_t)N * sizeof(float);
}

extern "C" int ib_linear_ln_fwd(const void* x, int64_t ldx, const void* w, int64_t ldw, const float* bias, const void* res,
                                int64_t ldres, const float* gamma, const float* beta, void* y, int64_t ldy, void* a_out,
                                float* mean, float* rstd, void* workspace, size_t workspace_bytes, int64_t M, int64_t N,
                                int64_t K, float eps, int dtype, ib_stream_t stream) {
  if (!x || !w || !gamma || !beta || !y || !workspace || M <= 0 || N <= 0 || K <= 0 || ldx < K || ldw < K || ldy < N)
    return IB_E_ARG;
  if (res && ldres < N) return IB_E_ARG;
  // the widths slab_ln_kernel is instantiated for (the switch below): refused here, before anything is launched
  const bool width_ok = N == 64 || N == 128 || N == 256 || N == 512 || N == 1024;
  if (dtype != IB_BF16 || !width_ok || K % 32 != 0) return IB_E_UNSUPPORTED;
  int chunk;
  int split = linear_ln_split(M, N, K, &chunk);
  if (!ib_al16({workspace, gamma, beta, bias}) || !ib_aligned(y, 8) || ldy % 4 != 0 || !ib_aligned(res, 8) ||
      (res && ldres % 4 != 0) || !ib_aligned(a_out, 8))
    return IB_E_ARG;
  hipStream_t s = ib_s(stream);
  // a few thousand rows (the sampler at B = 16: [3200, 512, 2048]): the 256 x 128 LDS-DMA kernel in split-K form -- 52 tiles x
  // 4 splits = 208 work items of 8 K steps instead of 400 ring-kernel workgroups of 16 short steps
  bool gemm_done = false;
  const int nts = ib_gemm_nt_splitk_splits(M, N, K);
  if (nts >= 2 && dtype == IB_BF16 && workspace_bytes >= (size_t)nts * M * N * sizeof(float)) {
    const int rc = ib_gemm_nt_splitk(x, ldx, w, ldw, reinterpret_cast<float*>(workspace), nts, M, N, K, s);
    if (rc == IB_OK) { gemm_done = true; split = nts; }
    else if (rc != IB_E_UNSUPPORTED) return rc;
  }
  if (workspace_bytes < (size_t)split * M * N * sizeof(float)) return IB_E_WORKSPACE;
  GemmParams p{};
  p.A = x; p.lda = ldx; p.B = w; p.ldb = ldw; p.M = (int)M; p.N = (int)N; p.K = (int)K;
  p.seg = 1; p.act = IB_ACT_NONE;
  fill_common<bf16_t>(p);
  p.k_chunk = chunk; p.xcd_group = 1;
  p.C = workspace; p.ldc = N; p.slab_stride = (int64_t)M * N; p.accumulate = 0; p.vecC = 1;
  if (!gemm_done) {
    if (!ring_ok(p)) return IB_E_UNSUPPORTED;
    IB_PATH(IB_PATH_LINLN);
    hipLaunchKernelGGL((gemm_ring_kernel<true, true, EPI_WGRAD>), dim3(p.tiles_m * p.tiles_n * split), dim3(NTHREADS), 0, s, p);
    IB_CHECK_LAUNCH();
  }
#define IB_SLAB_LN(LPR, NCH)                                                                                            \
  hipLaunchKernelGGL((slab_ln_kernel<LPR, NCH>), dim3((unsigned)((M + 256 / LPR - 1) / (256 / LPR))), dim3(256), 0, s,     \
                     reinterpret_cast<const float*>(workspace), split, (int64_t)M * N, bias,                               \
                     reinterpret_cast<const bf16_t*>(res), ldres, gamma, beta, reinterpret_cast<bf16_t*>(y), ldy,           \
                     reinterpret_cast<bf16_t*>(a_out), mean, rstd, (int)M, eps)
  switch (N) {
    case 64: IB_SLAB_LN(16, 1); break; case 128: IB_SLAB_LN(16, 2); break; case 256: IB_SLAB_LN(64, 1); break;
    case 512: IB_SLAB_LN(64, 2); break; case 1024: IB_SLAB_LN(64, 4); break;
    default: return IB_E_UNSUPPORTED;          // not reached: width_ok above admits exactly these five
  }
#undef IB_SLAB_LN
  IB_CHECK_LAUNCH();
  return IB_OK;
}
