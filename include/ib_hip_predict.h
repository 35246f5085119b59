/* What the denoiser predicts: the noise eps (the default, and the only form before this header), the clean window x0, or
 * v = alpha_t eps - sigma_t x0 (Salimans & Ho 2022), with alpha_t = sqrt(ab_t), sigma_t = sqrt(1 - ab_t)  (csrc/predict.hip).
 * Two launches: the loss launch of a training step under x0 / v, which forms the target in registers, and the conversion of
 * a buffer of network outputs into noise predictions, which a sampling step runs between the forward and the update, so no
 * update kernel changes.  The fifteenth header of the C-ABI of libib_hip.so.  Conventions as in ib_hip.h (device pointers, a
 * negative IB_E_* code on error, the stream last).  It is a header of its own so that the other fourteen and what is pinned to
 * them stay as they are: csrc/loss.hip and csrc/loss_weight.hip are untouched, and an eps model launches what it always did.
 * The binding parses it with the parser of ib_hip.h.
 *
 *   kind   the network's output o approximates    noise prediction from o and the state x_t
 *   0 eps  eps                                     o
 *   1 x0   x0                                      (x_t - alpha_t o) / sigma_t
 *   2 v    alpha_t eps - sigma_t x0                alpha_t o + sigma_t x_t
 *
 * Both kernels use one spelled fp32 form at every vector width and dtype (`fp contract(off)`, every fma written out).  The
 * per-level tables are fp32 [n_levels]; a level outside [0, n_levels) is clamped into the range before it indexes anything.
 *
 * ib_mse_loss_pred_partial is ib_mse_loss_weighted_partial (ib_hip_lossweight.h) with the target formed from x0, eps and the
 * window's level and a second per-level table on the reported sums.  tl = clamp(t[window], 0, n_levels - 1), w = wtab[tl],
 * u = utab[tl], a = sqrt_ab[tl], s = sqrt_1mab[tl], band k = tl * IB_LOSS_LEVEL_BUCKETS / n_levels.  Per scored element
 * (column c >= cond_cols), in fp32:
 *     target = eps                               (kind 0)
 *            = x0                                (kind 1)
 *            = fmaf(a, eps, -(s * x0))           (kind 2; s * x0 rounded first)
 *     q = pred - target
 *     dpred = round_T((q * gscale) * w)          gscale = 2.f / (float)(rows * (cols - cond_cols))
 *     sw = fmaf(q * w, q, sw)   su = fmaf(q * u, q, su)   sb[k] = fmaf(q * u, q, sb[k])
 * Conditioning columns get dpred = +0 on every launch; columns beyond cols are not touched.  Geometry, grid-stride order, the
 * wave and workgroup sums, the 2 + NB sums per workgroup and their place in the workspace, and the 4-wide / 1-wide rule are
 * the weighted entry's, so ib_mse_loss_weighted_workspace sizes the workspace and ib_mse_loss_weighted_finalize finishes the
 * launch unchanged.  No atomics.  At kind 0 with utab all ones dpred and every sum are bitwise the weighted entry's.
 * utab makes the reported sums the squared error of the implied noise prediction, sqrt(u) q, whatever the network predicts:
 * u = 1 for eps, ab / (1 - ab) for x0, ab for v (prediction.eps_units64).
 *
 * ib_pred_to_eps rewrites out, [B, T, ld] with D <= ld feature columns, from network outputs into noise predictions, given
 * the state x of the same layout; t is int64 [B], the level of each window.  With a = sqrt_ab[tl], s = sqrt_1mab[tl],
 * is = inv_sqrt_1mab[tl] (1 / sqrt(1 - ab) made in float64 and cast once: no division on the device):
 *     kind 2:  e = fmaf(a, o, s * x)             (s * x rounded first)
 *     kind 1:  r = fmaf(-a, o, x);  e = r * is   (the form of the x0 clip's rewrite, ib_hip_clip.h)
 *     out <- round_T(e)
 * One thread per 8 elements when ld % 8 == 0 and both pointers are 16-byte aligned, else per element; a vector that holds a
 * pad column D <= c < ld is done element by element.  Pad columns are never written; every column < D is. */
#ifndef IB_HIP_PREDICT_H
#define IB_HIP_PREDICT_H

#include "ib_hip.h"

#define IB_PRED_EPS 0
#define IB_PRED_X0 1
#define IB_PRED_V 2

#ifdef __cplusplus
extern "C" {
#endif

/* The loss launch under a prediction kind.  dpred may be null (sums only).  IB_E_ARG, nothing launched: a null pred / x0 / eps /
 * t / wtab / utab / sqrt_ab / sqrt_1mab, kind outside 0 .. 2, and whatever ib_mse_loss_weighted_partial refuses.
 * IB_E_WORKSPACE: a null workspace or fewer than ib_mse_loss_weighted_workspace(rows * cols) bytes.  IB_E_DTYPE: dtype. */
int ib_mse_loss_pred_partial(const void* pred, int64_t ld_pred, const void* x0, const void* eps, void* dpred, int64_t ld_dpred,
                             const int64_t* t, const float* wtab, const float* utab, const float* sqrt_ab,
                             const float* sqrt_1mab, int n_levels, int64_t rows_per_window, void* workspace,
                             size_t workspace_bytes, int64_t rows, int64_t cols, int64_t cond_cols, int kind, int dtype,
                             ib_stream_t stream);

/* The conversion, in place in out.  IB_E_ARG, nothing launched: a null pointer, kind other than 1 or 2 (a caller launches
 * nothing for eps), n_levels < 1, B, T or D <= 0, ld < D, B * T * ld beyond 2^62.  IB_E_DTYPE: dtype. */
int ib_pred_to_eps(const void* x, void* out, const int64_t* t, const float* sqrt_ab, const float* sqrt_1mab,
                   const float* inv_sqrt_1mab, int n_levels, int kind, int64_t B, int64_t T, int64_t D, int64_t ld, int dtype,
                   ib_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* IB_HIP_PREDICT_H */
