/* Stochastic stitched trial sampling: the third header of the C-ABI of libib_hip.so (csrc/stitch_noise.hip).  Conventions as
 * in ib_hip_stitch.h (device pointers, a negative IB_E_* code on error, the stream last); a header of its own so that
 * ib_hip.h, ib_hip_stitch.h and what is pinned to them stay as they are.  The binding parses it with the parser of ib_hip.h
 * into its own table.  State, layout tables (start, cover, wn) and the INVARIANT (all copies of a trial element are bitwise
 * equal before and after every call, in x and in z) are those of ib_hip_stitch.h. */
#ifndef IB_HIP_STITCH_NOISE_H
#define IB_HIP_STITCH_NOISE_H

#include "ib_hip_stitch.h"

#ifdef __cplusplus
extern "C" {
#endif

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
#endif /* IB_HIP_STITCH_NOISE_H */
