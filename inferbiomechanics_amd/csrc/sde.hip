// [BUILD-DEFINED] the SDE-DPM-Solver++(2M) update of the stitched loop (include/ib_hip_sde.h): stitch_step.h's
// stitch_step_kernel with MODE 3, the second-order multistep update with its fp32 history and the step noise per trial
// element with the stored noise of observed elements, together.  stitch.hip's head comment states the update.  A source
// file of its own: its twelve kernels are instantiated here, and stitch.hip's count stays what its test pins.
#include "stitch_step.h"
#include "../../include/ib_hip_sde.h"

extern "C" int ib_sde_dpmpp_step(void* x, const void* eps, float* hist, const void* x0, void* z, const uint8_t* mask,
                                 const float* coef, const float* obs_coef, const float* obs_noise_coef,
                                 const int64_t* timesteps, int64_t num_steps, int32_t step, const int32_t* step_dev,
                                 int64_t* t_out, const int32_t* start, const int32_t* cover, const float* wn,
                                 const int64_t* trial_id, uint64_t seed, int64_t N, int64_t W, int64_t T, int64_t F,
                                 int64_t D, int64_t ld, int dtype, ib_stream_t stream) {
  return stitch_launch<3>(x, eps, hist, x0, z, mask, coef, obs_coef, obs_noise_coef, timesteps, num_steps, step, step_dev,
                          t_out, start, cover, wn, trial_id, seed, N, W, T, F, D, ld, dtype, stream);
}
