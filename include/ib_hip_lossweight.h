/* Weighting the diffusion loss by noise level, and a report of the unweighted error per band of noise level, inside the loss
 * launch of the fused training step (csrc/loss_weight.hip): each window's squared error is multiplied by wtab[t] of its own noise
 * level t (loss_weight.LossWeight: uniform, Min-SNR-gamma of Hang et al. 2023, or a table of the caller's), and the same pass
 * keeps the unweighted sum and its split over IB_LOSS_LEVEL_BUCKETS bands of t -- no launch of their own, nothing read back per
 * step.  The fourteenth header of the C-ABI of libib_hip.so.  Conventions as in ib_hip.h (device pointers, a negative IB_E_* code
 * on error, the stream last).  It is a header of its own so that the other thirteen and what is pinned to them stay as they are:
 * csrc/loss.hip and its entries are untouched, and a trainer without a weight launches them as ever.  The binding parses it with
 * the parser of ib_hip.h.
 *
 * The arithmetic.  pred / dpred are [rows, cols] with leading dimensions, target is contiguous, as for ib_mse_loss_partial_cond.
 * Row r belongs to window r / rows_per_window; t is the trainer's int64 [rows / rows_per_window], wtab fp32 [n_levels].  A level
 * outside [0, n_levels) cannot be seen from the host: the kernels clamp it into the range before they index with it.
 *   tl = clamp(t[window], 0, n_levels - 1),  w = wtab[tl],  band k = tl * IB_LOSS_LEVEL_BUCKETS / n_levels  (integers)
 *   per scored element (column c >= cond_cols), in fp32:
 *     q = a - b
 *     dpred = round_T((q * gscale) * w)      two multiplies in that order, gscale = 2.f / (float)(rows * (cols - cond_cols))
 *     sw = fmaf(q * w, q, sw)   su = fmaf(q, q, su)   sb[k] = fmaf(q, q, sb[k])
 *   conditioning columns (c < cond_cols) get dpred = +0 on every launch; columns beyond cols are not touched.
 * At w = 1 dpred is bitwise ib_mse_loss_partial_cond's and sw is bitwise su.
 *
 * The order of the sums is that of ib_mse_loss_partial_cond: ib_mse_loss_workspace(n) / 4 workgroups of 256 threads, each thread
 * its elements in grid-stride order, then the wave, then the four waves in order.  Workgroup g writes its 2 + NB sums
 * {sw, su, sb[0 .. NB)} to workspace[g (2 + NB) ...]; the finalize adds each column over the workgroups as ib_mse_loss_finalize
 * adds its one.  No atomics: every number is bit-reproducible. */
#ifndef IB_HIP_LOSSWEIGHT_H
#define IB_HIP_LOSSWEIGHT_H

#include "ib_hip.h"

#define IB_LOSS_LEVEL_BUCKETS 8

#ifdef __cplusplus
extern "C" {
#endif

/* IB_LOSS_LEVEL_BUCKETS as the library was compiled with it (a host query) */
int ib_loss_level_buckets(void);

/* bytes of the partial sums of a launch over n = rows * cols elements: (2 + NB) floats per workgroup; n <= 0 -> 0 */
size_t ib_mse_loss_weighted_workspace(int64_t n);

/* The partial launch.  dpred may be null (sums only).  IB_E_ARG, nothing launched: a null pred / target / t / wtab, rows, cols or
 * rows_per_window <= 0, rows % rows_per_window != 0, n_levels < 1, cond_cols outside [0, cols), a leading dimension below cols.
 * IB_E_WORKSPACE: a null workspace or fewer than ib_mse_loss_weighted_workspace(rows * cols) bytes.  cond_cols = 0 runs the
 * same kernel.  4 columns per thread where cols, the leading dimensions and the pointers allow 4-element accesses, else 1. */
int ib_mse_loss_weighted_partial(const void* pred, int64_t ld_pred, const void* target, void* dpred, int64_t ld_dpred,
                                 const int64_t* t, const float* wtab, int n_levels, int64_t rows_per_window, void* workspace,
                                 size_t workspace_bytes, int64_t rows, int64_t cols, int64_t cond_cols, int dtype,
                                 ib_stream_t stream);

/* One workgroup finishes what a partial launch over n_launch = rows * cols elements left.  result, fp32 [2 + 2 NB]:
 *   [0] sw * (1 / n_mean), the weighted mean -- a plain mean, not divided by the sum of the weights
 *   [1] su * (1 / n_mean), the unweighted mean             (n_mean = rows * (cols - cond_cols), the reciprocal rounded to fp32)
 *   [2, 2 + NB) the band sums of squared error
 *   [2 + NB, 2 + 2 NB) the number of the n_windows windows of t in each band, counted here in integers
 * accum, fp64 [2 + 2 NB], may be null: accum[j] += (double)result[j] for every j in index order by one thread -- a running total
 * over replayed steps that nothing reads back.  IB_E_ARG: a null workspace / t / result, n_windows < 1, n_levels < 1,
 * n_launch <= 0, n_mean outside (0, n_launch]; IB_E_WORKSPACE: fewer bytes than the partial launch wrote. */
int ib_mse_loss_weighted_finalize(const void* workspace, size_t workspace_bytes, const int64_t* t, int64_t n_windows,
                                  int n_levels, float* result, double* accum, int64_t n_launch, int64_t n_mean,
                                  ib_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* IB_HIP_LOSSWEIGHT_H */
