/* Keeping the predicted x0 of a sampling step inside per-column bounds, and the record of the range each column takes: the
 * eighth header of the C-ABI of libib_hip.so (csrc/clip.hip).  Conventions as in ib_hip.h (device pointers, a negative IB_E_*
 * code on error, the stream last), which it includes.  A null pointer or a bad size is IB_E_ARG, an unknown dtype
 * IB_E_DTYPE, and nothing is launched.  It is a header of its own so that the other seven and what is pinned to them stay as
 * they are.  The binding parses it with the parser of ib_hip.h.
 *
 * The two clip entries sit between the denoiser's forward and the update launch of a sampling step and rewrite the noise
 * prediction eps alone.  State x and eps are [B, T, ld] of `dtype` (bf16 widens exactly), D <= ld feature columns; mask
 * (uint8 [T, ld], may be NULL: none) marks observed elements; lo, hi are fp32 [D].  Column c is BOUNDED iff lo[c] and hi[c] are
 * finite and hi[c] > lo[c]; an element is FREE iff c < D and its mask byte is 0.  Only free elements of bounded columns are
 * counted or changed; pad columns D <= c < ld are never read for arithmetic and never written.  coef is fp32
 * [table_rows, 4], row s = (ia, sa, a, is) = (1 / sqrt(ab), sqrt(1 - ab) / sqrt(ab), sqrt(ab), 1 / sqrt(1 - ab)) at the
 * step's level; s = *step_dev (step_dev NULL: step), clamped to the table, as in the update kernels.  All arithmetic is
 * fp32 without contraction, the same form at every vector width and dtype:
 *   p  = ia * x;   x0 = fma(-sa, e, p)
 *   x0c = the clipped prediction (below);   x0c == x0: the element's eps is NOT written
 *   else  r = fma(-a, x0c, x);   e' = r * is;   eps <- round_to_dtype(e')
 * Inputs are assumed finite. */
#ifndef IB_HIP_CLIP_H
#define IB_HIP_CLIP_H

#include "ib_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* x0c = min(max(x0, lo[c]), hi[c]).  One thread per vector: 8 elements when ld % 8 == 0 and x and eps are 16-byte aligned,
 * else 1; a vector that holds an observed, unbounded or pad element is handled element by element. */
int ib_x0_clip_range(const void* x, void* eps, const uint8_t* mask, const float* lo, const float* hi, const float* coef,
                     int64_t table_rows, int32_t step, const int32_t* step_dev, int64_t B, int64_t T, int64_t D, int64_t ld,
                     int dtype, ib_stream_t stream);

/* Dynamic thresholding (Saharia et al. 2022) per window and in per-column units.  m, h, ih are fp32 [D]: the centre
 * (lo + hi) / 2, the half width (hi - lo) / 2 and its reciprocal.
 *   u  = (x0 - m[c]) * ih[c]                       (two roundings)
 *   q  = the k-th smallest |u| over the window's free bounded elements (1 <= k <= their number n; k > n counts as n)
 *   sw = max(q, 1);   uc = min(max(u, -sw), sw) / sw;   x0c = (uc == u) ? x0 : fma(h[c], uc, m[c])
 * q is selected exactly (a radix select over the bit pattern of |u|), so the result does not depend on the order in which
 * elements are visited.  One workgroup per window.  k outside 1 .. T * D: IB_E_ARG. */
int ib_x0_clip_dynamic(const void* x, void* eps, const uint8_t* mask, const float* lo, const float* hi, const float* coef,
                       int64_t table_rows, int32_t step, const int32_t* step_dev, const float* m, const float* h,
                       const float* ih, int64_t k, int64_t B, int64_t T, int64_t D, int64_t ld, int dtype,
                       ib_stream_t stream);

/* out fp32 [D, 2] = per column (minimum, maximum) over the N * T rows of a window table [N, pitch] of `dtype`, window n
 * holding T contiguous rows of D values from n * pitch (pitch >= T * D; the pad behind them is not read).  Two launches:
 * each of G workgroups reduces a chunk of rows into partial fp32 [G, D, 2], then the partials are reduced.  Plain
 * comparisons, no float atomics: the result is exact.  1 <= G. */
int ib_column_range(const void* table, int64_t N, int64_t T, int64_t D, int64_t pitch, float* partial, int64_t G, float* out,
                    int dtype, ib_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* IB_HIP_CLIP_H */
