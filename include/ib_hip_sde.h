/* Stochastic second-order sampling: the fourth header of the C-ABI of libib_hip.so (csrc/sde.hip).  Conventions as in
 * ib_hip.h (device pointers, a negative IB_E_* code on error, the stream last) and the state, the layout tables and the
 * copies INVARIANT of ib_hip_stitch.h, which it includes: x, eps, x0, z are the window batch [N, W, T, ld] in `dtype`, hist
 * the same shape in fp32, mask uint8 [T, ld], start / cover / wn the layout of a trial of F frames.  It is a header of its
 * own so that the other three and what is pinned to them stay as they are.  The binding parses it with the parser of
 * ib_hip.h. */
#ifndef IB_HIP_SDE_H
#define IB_HIP_SDE_H

#include "ib_hip_stitch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The SDE-DPM-Solver++(2M) update (Lu et al. 2022; the stochastic form of ib_stitch_dpmpp_step) of the stitched loop, coef
 * fp32 [num_steps, 6] = (A, E, C, hx, he, G).  Width rule, blend (eb), choice of the update's rounding by column, s, step_dev
 * and t_out (int64 [N * W]) are ib_stitch_ddim_step's.  Per free trial element, in this order:
 *   o = A x + E eb                      (the rounding form of ib_stitch_ddim_step)
 *   o = fmaf(C, hist, o)                only in a row with C != 0 (uniform over the launch); hist read from the first copy
 *   o = fmaf(G, z', o)                  only in a row with G != 0 (uniform over the launch), on logical columns
 * and hist <- fmaf(hx, x, he * eb) is written to every copy by every row (not at a vector of observed elements only; what
 * hist holds at observed elements is unspecified).  z' is ib_stitch_ddim_step_noise's draw unchanged: Box-Muller over
 * Philox4x32-10 at counter ((f * D + d) >> 2, s, trial_id[n], domain 2), key = seed, f the TRIAL frame, words paired (x, y) ->
 * elements 0, 1 and (z, w) -> elements 2, 3 of the block; pad columns (d >= D) get no noise.  So a table with G == 0 in
 * every row IS ib_stitch_dpmpp_step bit for bit, and a table with C == 0 in every row IS ib_stitch_ddim_step_noise in x and
 * z for the same (cx, ce, sigma) = (A, E, G).
 *   observed element (x0, z, mask, obs_coef [num_steps + 1, 2], obs_noise_coef [num_steps, 2]; mask != 0):
 *     G != 0 row: the stored noise b, read from the first copy of z, becomes b' = round_to_dtype(fmaf(r, b, q * z')),
 *                 (r, q) = obs_noise_coef[s], written to EVERY copy of z, and x <- fmaf(ox, x0, oz * b'), (ox, oz) =
 *                 obs_coef[s + 1], written to every copy of x; a free element's z is left as it is.
 *     G == 0 row: x <- obs_coef[s + 1] (x0, z) as ib_stitch_ddim_step pins it; z is left untouched.
 * x0, z, mask, obs_coef and obs_noise_coef are all NULL (the unconditional loop) or all given; any mix: IB_E_ARG.  hist and
 * trial_id (device, int64 [N], each in 0 .. 2^32 - 1) NULL: IB_E_ARG.  T * ld >= 2^31 or F * D >= 2^31: IB_E_UNSUPPORTED.
 * With W == 1 (F == T, start = {0}, cover = {0, 1}, wn[f][0] = 1) it is the per-window update with window id = trial id. */
int ib_sde_dpmpp_step(void* x, const void* eps, float* hist, const void* x0, void* z, const uint8_t* mask,
                      const float* coef, const float* obs_coef, const float* obs_noise_coef, const int64_t* timesteps,
                      int64_t num_steps, int32_t step, const int32_t* step_dev, int64_t* t_out, const int32_t* start,
                      const int32_t* cover, const float* wn, const int64_t* trial_id, uint64_t seed, int64_t N, int64_t W,
                      int64_t T, int64_t F, int64_t D, int64_t ld, int dtype, ib_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* IB_HIP_SDE_H */
