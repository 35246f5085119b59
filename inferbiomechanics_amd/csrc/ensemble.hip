// [BUILD-DEFINED] order statistics of a posterior ensemble (include/ib_hip_ensemble.h): per element of a column window of
// x [B, K, rows, ld] the K members are sorted and reduced to three interpolated quantiles and, where a truth y is given, to
// the rank of the truth, the interval's hit flag and the fair ensemble CRPS (Ferro 2014).
//
// One lane owns one element (b, r, c), grid-stride.  Its members lie rows * ld apart, so the lanes of a wave read consecutive
// columns of one row at every member.  The members live in registers: a bitonic network over KP = the power of two at or above
// K, padded with +inf, fully unrolled -- every index into s[] is a compile-time constant, so the array never goes to
// scratch.  Two rules keep it that way and keep the padding out of the results:
//   - an order statistic at a runtime index is PICKED by unrolled selects (pick), never indexed;
//   - every term of the two sums is predicated on i < K inside the unrolled loop (0 * inf is NaN).
// A compare-exchange selects on (a < b) both ways, so the values are permuted, never dropped or duplicated.  All arithmetic is
// fp32 with contraction off: tests/ensemble_restatement.py states the same operations in the same order.  Plain stores, no
// LDS, no atomics; x is only read.
#include "ib_common.h"
#include "launch.h"
#include "../../include/ib_hip_ensemble.h"

namespace {

struct EnsembleArgs {
  const void* x; const float* y;
  float* q_lo; float* q_med; float* q_hi; float* crps; uint8_t* rank; uint8_t* inside;
  int64_t B, rows, ld, c0, w;
  int K, i_lo, i_med, i_hi;
  float f_lo, f_med, f_hi;
};

// ascending (UP) or descending order of the pair
template <bool UP>
__device__ __forceinline__ void cmp_exchange(float& a, float& b) {
  const bool lt = b < a;
  const float lo = lt ? b : a, hi = lt ? a : b;
  a = UP ? lo : hi;
  b = UP ? hi : lo;
}

template <int KP, int LK, int LJ>
__device__ __forceinline__ void bitonic_stage(float (&s)[KP]) {
  constexpr int k = 1 << LK, j = 1 << LJ;
#pragma unroll
  for (int i = 0; i < KP; ++i) {
    const int l = i ^ j;
    if (l > i) {
      if ((i & k) == 0) cmp_exchange<true>(s[i], s[l]); else cmp_exchange<false>(s[i], s[l]);
    }
  }
  if constexpr (LJ > 0) bitonic_stage<KP, LK, LJ - 1>(s);
}

template <int KP, int LK = 1>
__device__ __forceinline__ void bitonic_sort(float (&s)[KP]) {
  if constexpr ((1 << LK) <= KP) {
    bitonic_stage<KP, LK, LK - 1>(s);
    bitonic_sort<KP, LK + 1>(s);
  }
}

// v, as a value the optimiser cannot trace back to the array element it was loaded from (no instruction is emitted)
__device__ __forceinline__ float in_register(float v) {
  asm("" : "+v"(v));
  return v;
}

// s[i] for a runtime i in 0 .. KP - 1: a tree of selects on the bits of i, KP - 1 selects over log2(KP) uniform conditions.
// The operands go through in_register: a select between two loads of s[] is otherwise folded into one load at a selected
// index before the array has been split into registers, and the whole array then lives in scratch or LDS.
template <int KP>
__device__ __forceinline__ float pick(const float (&s)[KP], int i) {
  if constexpr (KP == 1) {
    return s[0];
  } else {
    float t[KP / 2];
    const bool odd = (i & 1) != 0;
#pragma unroll
    for (int j = 0; j < KP / 2; ++j) t[j] = odd ? in_register(s[2 * j + 1]) : in_register(s[2 * j]);
    return pick<KP / 2>(t, i >> 1);
  }
}

template <int KP>
__device__ __forceinline__ float quantile(const float (&s)[KP], int i, float f, int K) {
#pragma clang fp contract(off)
  const float a = pick<KP>(s, i), b = pick<KP>(s, i + 1 < K ? i + 1 : K - 1);
  const float d = b - a;
  const float m = f * d;
  return a + m;
}

template <typename TY, int KP>
__global__ __launch_bounds__(256) void ensemble_order_kernel(EnsembleArgs p) {
#pragma clang fp contract(off)
  const TY* __restrict__ x = (const TY*)p.x;
  const int64_t per_b = p.rows * p.w, total = p.B * per_b;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    // K and the member stride are made the iteration's own (no instruction is emitted): the conditions, offsets and weights
    // derived from them, a few per member, are then computed inside the iteration and not all held in scalar registers
    // across the loop
    int K = p.K;
    int64_t member = p.rows * p.ld;
    asm volatile("" : "+s"(K), "+s"(member));
    const int64_t b = e / per_b, rem = e - b * per_b, r = rem / p.w, c = rem - r * p.w;
    const TY* src = x + (b * K * p.rows + r) * p.ld + p.c0 + c;
    float s[KP];
#pragma unroll
    for (int i = 0; i < KP; ++i) s[i] = i < K ? ib_to_f32(src[i * member]) : __builtin_inff();
    bitonic_sort<KP>(s);
    const float lo = quantile<KP>(s, p.i_lo, p.f_lo, K), hi = quantile<KP>(s, p.i_hi, p.f_hi, K);
    p.q_lo[e] = lo;
    p.q_med[e] = quantile<KP>(s, p.i_med, p.f_med, K);
    p.q_hi[e] = hi;
    if (p.y) {                                                          // uniform over the launch
      const float y = p.y[e];
      float A = 0.f, G = 0.f;
      int below = 0;
#pragma unroll
      for (int i = 0; i < KP; ++i) {
        if (i < K) {                                                    // the padding takes no part: 0 * inf is NaN
          const float d = s[i] - y;
          A = A + __builtin_fabsf(d);
          const float t = (float)(2 * i - K + 1) * s[i];
          G = G + t;
          below += s[i] < y ? 1 : 0;
        }
      }
      const float fk = (float)K;
      float score = A / fk;
      if (K > 1) score = score - G / (float)(K * (K - 1));
      p.crps[e] = score;
      p.rank[e] = (uint8_t)below;
      p.inside[e] = (uint8_t)((lo <= y && y <= hi) ? 1 : 0);
    }
  }
}

}  // namespace

extern "C" int ib_ensemble_order(const void* x, const float* y, float* q_lo, float* q_med, float* q_hi, float* crps,
                                 uint8_t* rank, uint8_t* inside, int64_t B, int64_t K, int64_t rows, int64_t ld, int64_t c0,
                                 int64_t w, int32_t i_lo, float f_lo, int32_t i_med, float f_med, int32_t i_hi, float f_hi,
                                 int dtype, ib_stream_t stream) {
  if (!x || !q_lo || !q_med || !q_hi) return IB_E_ARG;
  const int given = (y != nullptr) + (crps != nullptr) + (rank != nullptr) + (inside != nullptr);
  if (given != 0 && given != 4) return IB_E_ARG;                       // the score comes whole or not at all
  if (B <= 0 || K < 1 || rows <= 0 || w <= 0 || c0 < 0 || c0 + w > ld) return IB_E_ARG;
  for (const int32_t i : {i_lo, i_med, i_hi})
    if (i < 0 || i >= K) return IB_E_ARG;
  if (!ib_dtype_known(dtype)) return IB_E_DTYPE;
  if (K > IB_ENSEMBLE_KMAX) return IB_E_UNSUPPORTED;
  const EnsembleArgs p{x, y, q_lo, q_med, q_hi, crps, rank, inside, B, rows, ld, c0, w,
                       (int)K, i_lo, i_med, i_hi, f_lo, f_med, f_hi};
  const int grid = ib_grid_1d(B * rows * w, 256);
  return ib_dispatch_dtype(dtype, [&](auto tag) {
    using TY = decltype(tag);
    auto go = [&](auto kp) {
      hipLaunchKernelGGL((ensemble_order_kernel<TY, decltype(kp)::value>), dim3(grid), dim3(256), 0, ib_s(stream), p);
    };
    if (K <= 1) go(ib_width<1>{});
    else if (K <= 2) go(ib_width<2>{});
    else if (K <= 4) go(ib_width<4>{});
    else if (K <= 8) go(ib_width<8>{});
    else if (K <= 16) go(ib_width<16>{});
    else if (K <= 32) go(ib_width<32>{});
    else go(ib_width<64>{});
  });
}
