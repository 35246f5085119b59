/* A temporal-difference (velocity) term on the predicted clean window, inside the loss launch of the fused training step
 * (csrc/velocity.hip): beside the weighted squared error of the network's output the launch scores the error of the frame
 * difference of the implied x0 (the "geometric loss" of MDM, Tevet et al. 2023), the first loss of the library that couples
 * rows.  The sixteenth header of the C-ABI of libib_hip.so.  Conventions as in ib_hip.h (device pointers, a negative IB_E_*
 * code on error, the stream last).  It is a header of its own so that the other fifteen and what is pinned to them stay as they
 * are: csrc/loss.hip, csrc/loss_weight.hip and csrc/predict.hip are untouched, and a trainer without the term launches what it
 * always did.  The binding parses it with the parser of ib_hip.h.
 *
 * For every prediction kind the error of the implied x0 is a per-window constant times the error q = o - target of the output
 * (target as in ib_hip_predict.h):  x0hat - x0 = c_t q  with  c_t^2 = 1 / snr (eps), 1 (x0), 1 - ab (v).  So the term needs q of
 * neighbouring frames and two per-level tables, never x_t (velocity_loss.VelocityLoss.tables):
 *     vtab[t] = lambda m_t c_t^2     the weight of the term in output units, m_t = min(snr_t, gamma) or the caller's table
 *     xtab[t] = c_t^2                puts the reported error in x0 units
 *
 * The arithmetic.  pred / dpred are [rows, cols] with leading dimensions, x0 / eps contiguous; row r is frame f = r % T of
 * window b = r / T, T = rows_per_window >= 2.  tl = clamp(t[b], 0, n_levels - 1), w = wtab[tl], u = utab[tl], v = vtab[tl],
 * x = xtab[tl], a = sqrt_ab[tl], s = sqrt_1mab[tl], band k = tl * IB_LOSS_LEVEL_BUCKETS / n_levels.  Per scored element (column
 * c >= cond_cols), in fp32, one spelled form at every vector width and dtype (`fp contract(off)`, every fma written out):
 *     q[f]  = pred - target(kind)                  the forms of ib_hip_predict.h
 *     dn    = q[f+1] - q[f]   for f < T-1,  0 at f = T-1
 *     dp    = q[f] - q[f-1]   for f > 0,    0 at f = 0           (bitwise the dn of frame f-1)
 *     dm    = (q[f] * gscale) * w                  gscale = 2.f / (float)(rows * (cols - cond_cols))
 *     dv    = ((dp - dn) * vscale) * v             vscale = 2.f / (float)((rows - rows / T) * (cols - cond_cols))
 *     dpred = round_T(dm + dv)
 *     sw = fmaf(q * w, q, sw)   su = fmaf(q * u, q, su)   sb[k] = fmaf(q * u, q, sb[k])
 *     for f < T-1:   sv = fmaf(dn * v, dn, sv)   sx = fmaf(dn * x, dn, sx)   sxb[k] = fmaf(dn * x, dn, sxb[k])
 * The optimised loss is sw / n + sv / n_v, n = rows (cols - cond_cols), n_v = (rows - rows / T)(cols - cond_cols); dpred is its
 * gradient.  Differences never cross a window boundary.  Conditioning columns get dpred = +0 on every launch; columns beyond
 * cols are not touched.  With vtab all zero dpred compares equal to ib_mse_loss_pred_partial's.
 *
 * Geometry.  A window's frames are cut into chunks of FC = IB_VEL_FRAME_CHUNK; a thread owns one vector of V columns (4 where
 * cols, the leading dimensions and the pointers allow 4-element accesses, else 1: the rule of ib_mse_loss_pred_partial) of one
 * chunk of one window, unit i = (b * ceil(T / FC) + chunk) * (cols / V) + vector, so a wave's loads of one frame are
 * contiguous.  The thread reads the level and the tables once, loads the chunk's FC frames and one halo frame on each side
 * before it uses any, and keeps every q in registers.  A halo frame's q is recomputed, not exchanged: it is bitwise what the
 * neighbouring chunk computes, and every dn is summed once, by the owner of frame f.  Where a chunk has no frame to load -- the
 * halo outside the window, the frames past a short last chunk -- the load is aimed at the window's nearest frame and its value
 * is not used: the loads stay unconditional and in flight together.  The launch reads at most (FC + 2) / FC times the bytes of
 * ib_mse_loss_pred_partial.
 *
 * The order of the sums.  ib_vel_loss_workspace(rows, cols, T) / (4 (4 + 2 NB)) workgroups of 256 threads -- a count that does
 * not depend on V; each thread its units in grid-stride order, in a unit the frames in order, in a frame the columns in order,
 * per element the three error sums and then the three velocity sums; then the wave (four DPP adds, the four row totals in
 * order), then the four waves in order.  Workgroup g writes its (2 + NB) + (2 + NB) sums {sw, su, sb[0 .. NB), sv, sx,
 * sxb[0 .. NB)} to workspace[g (4 + 2 NB) ...].  No atomics: two launches give the same bits. */
#ifndef IB_HIP_VELOCITY_H
#define IB_HIP_VELOCITY_H

#include "ib_hip.h"
#include "ib_hip_lossweight.h"
#include "ib_hip_predict.h"

#define IB_VEL_FRAME_CHUNK 8

/* places in the result of ib_vel_loss_finalize, NB = IB_LOSS_LEVEL_BUCKETS; [0, 2 + 2 NB) is laid out as the result of
 * ib_mse_loss_weighted_finalize */
#define IB_VEL_R_TOTAL 0                                   /* sw / n + sv / n_v: the optimised loss */
#define IB_VEL_R_EPS 1                                     /* su / n: the unweighted eps-MSE */
#define IB_VEL_R_BANDS 2                                   /* NB band sums of it */
#define IB_VEL_R_COUNTS (2 + IB_LOSS_LEVEL_BUCKETS)        /* NB window counts */
#define IB_VEL_R_MSE (2 + 2 * IB_LOSS_LEVEL_BUCKETS)       /* sw / n: the weighted MSE term alone */
#define IB_VEL_R_VEL (3 + 2 * IB_LOSS_LEVEL_BUCKETS)       /* sv / n_v: the velocity term */
#define IB_VEL_R_X0 (4 + 2 * IB_LOSS_LEVEL_BUCKETS)        /* sx / n_v: the velocity error in x0 units */
#define IB_VEL_R_X0_BANDS (5 + 2 * IB_LOSS_LEVEL_BUCKETS)  /* NB band sums of it */
#define IB_VEL_RESULT_LEN (5 + 3 * IB_LOSS_LEVEL_BUCKETS)

#ifdef __cplusplus
extern "C" {
#endif

/* IB_VEL_FRAME_CHUNK as the library was compiled with it (a host query) */
int ib_vel_loss_frame_chunk(void);

/* bytes of the partial sums of a launch over [rows, cols] in windows of rows_per_window frames: (4 + 2 NB) floats per
 * workgroup; 0 where the launch would be refused for its shape */
size_t ib_vel_loss_workspace(int64_t rows, int64_t cols, int64_t rows_per_window);

/* The partial launch: the arguments of ib_mse_loss_pred_partial plus vtab and xtab.  dpred may be null (sums only).  IB_E_ARG,
 * nothing launched: a null pred / x0 / eps / t / any of the six tables, kind outside 0 .. 2, rows_per_window < 2, and whatever
 * ib_mse_loss_pred_partial refuses.  IB_E_WORKSPACE: a null workspace or fewer than ib_vel_loss_workspace(rows, cols,
 * rows_per_window) bytes.  IB_E_DTYPE: dtype. */
int ib_vel_loss_partial(const void* pred, int64_t ld_pred, const void* x0, const void* eps, void* dpred, int64_t ld_dpred,
                        const int64_t* t, const float* wtab, const float* utab, const float* vtab, const float* xtab,
                        const float* sqrt_ab, const float* sqrt_1mab, int n_levels, int64_t rows_per_window, void* workspace,
                        size_t workspace_bytes, int64_t rows, int64_t cols, int64_t cond_cols, int kind, int dtype,
                        ib_stream_t stream);

/* One workgroup finishes what a partial launch of the same rows, cols and rows_per_window left: each of the 4 + 2 NB columns
 * of the partials is added thread-strided and then by a tree, as ib_mse_loss_weighted_finalize adds its 2 + NB, and the
 * n_windows = rows / rows_per_window windows of t are counted per band in integers.  result, fp32 [IB_VEL_RESULT_LEN], by the
 * IB_VEL_R_* places above; the reciprocals 1 / n and 1 / n_v are rounded to fp32, the total is mse + vel in fp32.  accum, fp64
 * [IB_VEL_RESULT_LEN], may be null: accum[j] += (double)result[j] for every j in index order by one thread.  IB_E_ARG: a null
 * workspace / t / result, n_levels < 1, a shape the partial launch refuses; IB_E_WORKSPACE: fewer bytes than it wrote. */
int ib_vel_loss_finalize(const void* workspace, size_t workspace_bytes, const int64_t* t, int n_levels, float* result,
                         double* accum, int64_t rows, int64_t cols, int64_t cond_cols, int64_t rows_per_window,
                         ib_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* IB_HIP_VELOCITY_H */
