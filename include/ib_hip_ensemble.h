/* Order statistics of a posterior ensemble: the seventh header of the C-ABI of libib_hip.so (csrc/ensemble.hip).
 * Conventions as in ib_hip.h (device pointers, a negative IB_E_* code on error, the stream last).  It is a header of its own
 * so that the other six and what is pinned to them stay as they are.  The binding parses it with the parser of ib_hip.h. */
#ifndef IB_HIP_ENSEMBLE_H
#define IB_HIP_ENSEMBLE_H

#include "ib_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IB_ENSEMBLE_KMAX 64

/* x is [B, K, rows, ld] in `dtype` (fp32 or bf16).  Element (b, r, c), c in 0 .. w - 1, has its K members at
 * x[b, k, r, c0 + c]; y and every output are contiguous [B, rows, w].  x is only read, and nothing outside the outputs is
 * written.  All arithmetic is fp32 without contraction; bf16 widens exactly.  Per element:
 *   s       the K members sorted ascending, by compare-exchanges that select on (a < b): values are permuted, never dropped.
 *   Q(i, f) = s[i] + f * (s[min(i + 1, K - 1)] - s[i]), three roundings as written; q_lo = Q(i_lo, f_lo), q_med =
 *           Q(i_med, f_med), q_hi = Q(i_hi, f_hi).  The host computes (i, f) (diffusion/ensemble.py quantile_position).
 *   rank    #{k : x_k < y}, in 0 .. K: a tie counts as not less.
 *   inside  (q_lo <= y && y <= q_hi).
 *   crps    the fair ensemble CRPS (Ferro 2014): A / K - (K > 1 ? G / (K (K - 1)) : 0), A = sum_i |s_i - y|,
 *           G = sum_i (2 i - K + 1) * s_i (= sum_{i<j} (s_j - s_i)), both summed in sorted order i = 0 .. K - 1, one product
 *           and one add per term.
 * y, crps, rank and inside are all NULL (quantiles only) or all given; any mix: IB_E_ARG.  x, q_lo, q_med or q_hi NULL,
 * B, rows or w <= 0, K < 1, c0 < 0, c0 + w > ld, an i_* outside 0 .. K - 1: IB_E_ARG.  An unknown dtype: IB_E_DTYPE.
 * K > IB_ENSEMBLE_KMAX: IB_E_UNSUPPORTED. */
int ib_ensemble_order(const void* x, const float* y, float* q_lo, float* q_med, float* q_hi, float* crps, uint8_t* rank,
                      uint8_t* inside, int64_t B, int64_t K, int64_t rows, int64_t ld, int64_t c0, int64_t w,
                      int32_t i_lo, float f_lo, int32_t i_med, float f_med, int32_t i_hi, float f_hi, int dtype,
                      ib_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* IB_HIP_ENSEMBLE_H */
