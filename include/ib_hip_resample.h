/* RePaint resampling of the masked sampling loops (Lugmayr et al. 2022, Algorithm 1): the sixth header of the C-ABI of
 * libib_hip.so (csrc/resample.hip).  Conventions as in ib_hip.h (device pointers, a negative IB_E_* code on error, the stream
 * last) and the state, the layout tables and the copies INVARIANT of ib_hip_stitch.h, which it includes: x, x0, z are the
 * window batch [N, W, T, ld] in `dtype`, mask uint8 [T, ld] read at the first copy, start / cover the layout of a trial of F
 * frames.  A per-window loop is W = 1 with the one-window layout (F == T, start = {0}, cover = {0, 1}), the window ids as
 * trial ids, as ib_sde_dpmpp_step is used.  It is a header of its own so that the other five and what is pinned to them stay
 * as they are.  The binding parses it with the parser of ib_hip.h. */
#ifndef IB_HIP_RESAMPLE_H
#define IB_HIP_RESAMPLE_H

#include "ib_hip_stitch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The jump of a resampled loop: the state, which stands at POSITION s = step + *step_dev (step_dev NULL: step alone) of a loop
 * of num_steps updates -- position p < num_steps is the noise level of timesteps[p], position num_steps is alpha_bar = 1 --,
 * is diffused back `back` levels to position q = s - back with fresh noise.  coef fp32 [num_steps + 1, 2], row p = (cx, cz) =
 * (sqrt(rho), sqrt(1 - rho)), rho = alpha_bar(p - back) / alpha_bar(p) (schedule.resample_coefficients; rows p < back are
 * never read).
 *   free trial element (n, f, d):  x <- round_to_dtype(fmaf(cz, z', cx * x)), (cx, cz) = coef[s], x read from the first copy
 *                      and the result written to every copy.  z' is Box-Muller over Philox4x32-10 at counter
 *                      ((f * D + d) >> 2, visit, trial_id[n], domain 4), key = seed, words paired as in
 *                      ib_stitch_ddim_step_noise: (x, y) -> elements 0, 1 and (z, w) -> elements 2, 3 of the block.  f is the
 *                      TRIAL frame: the draw is a function of (seed, trial_id[n], visit, f, d) alone -- not of the batch
 *                      position, N, the row pitch, the vector width or the window layout.  Pad columns (d >= D) get no noise:
 *                      cx * x, so 0 stays 0.
 *   observed element:  (x0, z, mask, obs_coef [num_steps + 1, 2]; mask != 0) x <- obs_coef[q][0] * x0 + obs_coef[q][1] * z in
 *                      the rounding form, by column and width, in which ib_stitch_ddim_step pins obs_coef[s + 1]: for q >= 1 it
 *                      is, bit for bit, what the eta = 0 update that first arrived at position q wrote.  z is not written.
 * t_out (int64 [N * W]) receives timesteps[q].  The step counter is NOT touched: the caller follows with
 * ib_counter_add(counter, -back).  Width rule: ib_stitch_ddim_step's (16-byte accesses when ld % 8 == 0 and the buffers are
 * aligned, element-wise otherwise).  `visit` is the ordinal of the jump within the sampling call, so every jump of a call
 * draws fresh noise.
 * x0, z, mask and obs_coef are all NULL (every element is free) or all given; any mix: IB_E_ARG.  x, coef, timesteps, t_out,
 * start, cover or trial_id (device, int64 [N], each in 0 .. 2^32 - 1) NULL: IB_E_ARG; back < 1: IB_E_ARG.  T * ld >= 2^31 or
 * F * D >= 2^31: IB_E_UNSUPPORTED.  A launch whose s lies outside back .. num_steps reads no table row and writes nothing (the
 * position lives on the device, so the host cannot refuse it). */
int ib_resample_renoise(void* x, const void* x0, const void* z, const uint8_t* mask, const float* coef,
                        const float* obs_coef, const int64_t* timesteps, int64_t num_steps, int32_t step,
                        const int32_t* step_dev, int32_t back, uint32_t visit, int64_t* t_out,
                        const int32_t* start, const int32_t* cover, const int64_t* trial_id, uint64_t seed,
                        int64_t N, int64_t W, int64_t T, int64_t F, int64_t D, int64_t ld, int dtype,
                        ib_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* IB_HIP_RESAMPLE_H */
