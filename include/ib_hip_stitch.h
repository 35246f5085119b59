/* Stitched trial sampling: the second header of the C-ABI of libib_hip.so (csrc/stitch.hip).  Conventions as in ib_hip.h
 * (device pointers, a negative IB_E_* code on error, the stream last); it is a header of its own so that ib_hip.h and what
 * is pinned to it stay as they are.  The binding parses it with the parser of ib_hip.h.
 *
 * A trial of F frames is denoised as W overlapping windows of T frames.  The state stays the window batch the denoiser plan
 * consumes: x, eps, x0, z are [N, W, T, ld] in `dtype` for N trials with the same layout (row pitch ld >= D, zero pad
 * columns stay 0), hist is the same shape in fp32, mask is uint8 [T, ld].  Device tables describe the layout:
 *   start int32 [W]                    first trial frame of window w, strictly increasing, start[W-1] + T == F
 *   cover int32 [F, 2]                 per trial frame: the first covering window and how many cover it (they are consecutive,
 *                                      1 .. IB_STITCH_KMAX)
 *   wn    fp32  [F, IB_STITCH_KMAX]    the blend weights of the covering windows in window order, summing to 1 per frame
 * start and cover are trusted: the caller owns their validity (the Python binding checks them).
 * A copy of trial element (n, f, c) is x[n, w, f - start[w], c] for a window w that covers f.  INVARIANT: all copies of an
 * element are bitwise equal before and after every call, in x, hist and z (the caller makes x, hist, x0, z and the mask
 * consistent at the start; the mask is read at the first copy). */
#ifndef IB_HIP_STITCH_H
#define IB_HIP_STITCH_H

#include "ib_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IB_STITCH_KMAX 8

/* The DDIM update (eta = 0) of the stitched loop, coef fp32 [num_steps, 2].  Per trial element: eb = the blend of the
 * covering windows' eps (one window: its eps as it is; more: wn[f][0] e_0, then fmaf(wn[f][k], e_k, eb) for k ascending, in
 * fp32), then x <- coef[s][0] * x + coef[s][1] * eb over the first copy's x, written to every copy.  x0, z, mask and obs_coef
 * (fp32 [num_steps + 1, 2]) are all NULL for the unconditional loop or all given for the masked one (any mix: IB_E_ARG): an
 * element with mask != 0 is then obs_coef[s+1][0] * x0 + obs_coef[s+1][1] * z, as ib_ddim_cond_step computes it.  s, step_dev
 * and t_out (int64 [N * W]) as in ib_ddim_step.  16-byte accesses when ld % 8 == 0 and the buffers are aligned as
 * ib_ddim_cond_step asks, element-wise otherwise; the rounding of the update is chosen by column, so all copies round
 * alike.  With W == 1 (F == T) the call equals ib_ddim_step / ib_ddim_cond_step bit for bit when ld % 8 == 0 or the flat
 * kernels run element-wise.  T * ld >= 2^31: IB_E_UNSUPPORTED. */
int ib_stitch_ddim_step(void* x, const void* eps, const void* x0, const void* z, const uint8_t* mask, const float* coef,
                        const float* obs_coef, const int64_t* timesteps, int64_t num_steps, int32_t step,
                        const int32_t* step_dev, int64_t* t_out, const int32_t* start, const int32_t* cover,
                        const float* wn, int64_t N, int64_t W, int64_t T, int64_t F, int64_t D, int64_t ld, int dtype,
                        ib_stream_t stream);
/* The DPM-Solver++(2M) update of the stitched loop, coef fp32 [num_steps, 5] = (A, E, C, hx, he): as ib_stitch_ddim_step
 * with x <- A x + E eb + C hist (hist read from the first copy, only by rows with C != 0) and hist <- hx x + he eb written to
 * every copy (not at a vector of observed elements only; what hist holds at observed elements is unspecified).  With W == 1
 * it equals ib_dpmpp_step / ib_dpmpp_cond_step under the same conditions. */
int ib_stitch_dpmpp_step(void* x, const void* eps, float* hist, const void* x0, const void* z, const uint8_t* mask,
                         const float* coef, const float* obs_coef, const int64_t* timesteps, int64_t num_steps,
                         int32_t step, const int32_t* step_dev, int64_t* t_out, const int32_t* start,
                         const int32_t* cover, const float* wn, int64_t N, int64_t W, int64_t T, int64_t F, int64_t D,
                         int64_t ld, int dtype, ib_stream_t stream);
/* The stochastic DDIM / DDPM update (eta > 0) of the stitched loop, coef fp32 [num_steps, 3] = (cx, ce, sigma) as
 * ib_ddim_step_noise takes them.  Width rule, blend (eb), choice of the update's rounding by column and the pinned value of a
 * sigma == 0 row are ib_stitch_ddim_step's: a row with sigma == 0 (uniform over the launch: every row of an eta = 0 table,
 * the last row of any table) IS that update bit for bit and leaves z untouched.
 * Otherwise the normal z' of trial element (n, f, d) at step s is Box-Muller over Philox4x32-10 at counter
 * ((f * D + d) >> 2, s, trial_id[n], domain 2), key = seed, words paired as in ib_ddim_step_noise: (x, y) -> elements 0, 1 and
 * (z, w) -> elements 2, 3 of the block.  f is the TRIAL frame, so every copy of an element gets the same normal by
 * construction: the draw is a function of (seed, trial_id[n], s, f, d) alone -- not of the batch position, N, the row pitch,
 * the vector width or the window layout -- and with W == 1 it is ib_ddim_step_noise's with window id = trial id.  Pad columns
 * (d >= D) get no noise.
 *   free element:      x <- fmaf(sigma, z', cx * x + ce * eb), written to every copy
 *   observed element:  (x0, z, mask, obs_coef [num_steps + 1, 2], obs_noise_coef [num_steps, 2]; mask != 0) the stored noise b,
 *                      read from the first copy of z, becomes b' = round_to_dtype(fmaf(r, b, q * z')), (r, q) =
 *                      obs_noise_coef[s], written to EVERY copy of z, and x <- fmaf(ox, x0, oz * b'), (ox, oz) =
 *                      obs_coef[s + 1], written to every copy of x -- the arithmetic of ib_ddim_cond_step_noise.  z is
 *                      read-write; a free element's z is left as it is.
 * x0, z, mask, obs_coef and obs_noise_coef are all NULL (the unconditional loop) or all given; any mix: IB_E_ARG.  trial_id
 * (device, int64 [N], each in 0 .. 2^32 - 1) NULL: IB_E_ARG.  s, step_dev and t_out (int64 [N * W]) as in
 * ib_stitch_ddim_step, and so the other refusals.  F * D >= 2^31: IB_E_UNSUPPORTED (the block index is one 32-bit counter
 * word). */
int ib_stitch_ddim_step_noise(void* x, const void* eps, const void* x0, void* z, const uint8_t* mask, const float* coef,
                              const float* obs_coef, const float* obs_noise_coef, const int64_t* timesteps,
                              int64_t num_steps, int32_t step, const int32_t* step_dev, int64_t* t_out, const int32_t* start,
                              const int32_t* cover, const float* wn, const int64_t* trial_id, uint64_t seed, int64_t N,
                              int64_t W, int64_t T, int64_t F, int64_t D, int64_t ld, int dtype, ib_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* IB_HIP_STITCH_H */
