/* Per-column standardisation z = (x - mean_c) / scale_c of the diffusion windows: the moments of a window table and the
 * affine map between raw and standardised units.  The ninth header of the C-ABI of libib_hip.so (csrc/standardize.hip).
 * Conventions as in ib_hip.h (device pointers, a negative IB_E_* code on error, the stream last), which it includes.  A null
 * pointer or a bad size is IB_E_ARG, an unknown dtype IB_E_DTYPE, and nothing is launched.  It is a header of its own so
 * that the other eight and what is pinned to them stay as they are.  The binding parses it with the parser of ib_hip.h.
 *
 * The moments are one pass of fp64 sums about a per-column shift (the caller passes the first frame of the first window),
 * which keeps S2/count - md*md free of the cancellation an offset column would cause.  No float atomics anywhere: every sum
 * has a fixed order, so a result is bit-reproducible run to run. */
#ifndef IB_HIP_STANDARDIZE_H
#define IB_HIP_STANDARDIZE_H

#include "ib_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* acc fp64 [G, D, 2] += per column (sum d, sum d*d) over the n*T rows of src [n, pitch] (`dtype`; window i holds T contiguous
 * rows of D values from i*pitch, pitch >= T*D, the pad is never read), d = (double)x - (double)shift[c].  Workgroup g adds
 * its rows' sums into slot g only, in a fixed order: no float atomics, bit-reproducible run to run.  The caller zeroes acc
 * once and may call this for chunk after chunk with the same G, D, shift.  shift is fp32 [D].  1 <= G <= 65535. */
int ib_column_moments_accum(const void* src, int64_t n, int64_t T, int64_t D, int64_t pitch, const float* shift,
                            double* acc, int64_t G, int dtype, ib_stream_t stream);

/* per column, in fp64, slots summed in order g = 0 .. G-1:  md = S1/count;  var = max(S2/count - md*md, 0) (population);
 * mean[c] = (float)(shift[c] + md);  s = (float)sqrt(var);  scale[c] = s > min_std ? s : 1.0f;
 * inv[c] = (float)(1.0 / (double)scale[c])   -- from the fp32 scale, so a checkpoint's (mean, scale) gives the same inv.
 * mean, scale, inv are fp32 [D]; count is the number of rows accumulated (the sum of n*T over the calls). */
int ib_column_moments_finalize(const double* acc, int64_t G, int64_t D, int64_t count, const float* shift, float min_std,
                               float* mean, float* scale, float* inv, ib_stream_t stream);

/* element (i, t, c), c0 <= c < c0+w, of N windows x T rows: src at i*src_win + t*src_row + c, dst likewise (a cache table:
 * win = pitch, row = D; a sampler state [B, T, ld]: win = T*ld, row = ld).  a, b are fp32 indexed by the column c itself
 * (at least c0+w long).  fp32 arithmetic, fp contract off, one form at every width and dtype pair:
 *   mode 0 (standardise):    d = x - a[c];  y = d * b[c]          (a = mean, b = inv; two roundings)
 *   mode 1 (de-standardise): y = fma(x, b[c], a[c])               (a = mean, b = scale; a NULL: y = x * b[c])
 * then y rounded to dst_dtype.  src == dst with equal dtype and strides is allowed (in place).  Columns outside
 * [c0, c0+w) and pads are neither read for arithmetic nor written.  8 elements per thread where rows, c0, w and both
 * bases allow 16-byte (bf16) / 32-byte (fp32) vectors, else 1.  Whole dense rows (c0 = 0, w = row on both sides,
 * w <= 2048, such bases) are taken as flat runs instead, 8 consecutive values per thread whatever w is: one run when the
 * windows are dense too (win = T*row), else one per window when both win are multiples of 8.  row >= c0+w and
 * win >= (T-1)*row + c0+w on both sides; a NULL in mode 0 is IB_E_ARG. */
int ib_column_affine(const void* src, int src_dtype, int64_t src_win, int64_t src_row, void* dst, int dst_dtype,
                     int64_t dst_win, int64_t dst_row, const float* a, const float* b, int64_t N, int64_t T,
                     int64_t c0, int64_t w, int mode, ib_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* IB_HIP_STANDARDIZE_H */
