// [BUILD-DEFINED] stitched sampler updates (include/ib_hip_stitch.h): the DDIM, DPM-Solver++(2M) and stochastic (eta > 0)
// DDIM / DDPM updates of a trial of F frames that is denoised as W overlapping windows of T frames (MultiDiffusion /
// DiffCollage stitching).  The state stays the window batch the denoiser plan consumes, x [N, W, T, ld]; a trial element
// (n, f, c) has one copy x[n, w, f - start[w], c] in every window w that covers frame f.  INVARIANT: all copies of a trial
// element are bitwise equal before and after every launch.  The update blends the noise predictions of the covering
// windows, updates the element once and writes the one result to every copy.  ONE kernel template (stitch_step.h) holds
// the loop, so the updates cannot drift apart: MODE 0 = ddim, 1 = dpm, 2 = noise, 3 = dpm and noise together (sde.hip's
// entry point), and what only some of them do sits behind `if constexpr` on MODE's bits.  The flat updates of diffusion.hip
// take their rounding forms from the same header (sampler_elem.h), which is why one window here equals them bit for bit.
//
// One thread owns V consecutive columns of one trial row (n, f): it alone reads and writes the copies of those elements, so
// the update is in place with no LDS and no atomics.  Per launch it reads count x the eps bytes of a row (count = windows
// that cover the frame, <= IB_STITCH_KMAX), x (and hist, x0, z where used) once from the first copy, and writes x (and hist,
// or z at observed elements of a noisy row) count times.
//
// WIDTH AND ROUNDING, stated once.  V = 8 (16-byte accesses) when ld % 8 == 0 and ib_sampler_geom (launch_geom.h, called
// unchanged with per = T * ld) allows 8-wide kernels on the window buffers: a vector then never crosses a frame row.
// Otherwise V = 1.  The form of ddim_mix is chosen by COLUMN: the 8-wide form ddim_mix<T, 8>(c & 7, ...) whenever
// ib_sampler_geom's mix8 holds for the window buffers, the lone-element form otherwise.  A copy's flat offset differs from
// window to window, its column does not, so all copies of an element round alike; for ld % 8 == 0 column and flat offset
// agree modulo 8, so it is also what the 8-wide kernels of diffusion.hip do.  The blend is fp32 in window order,
// eb = wn[0] e_0, eb = fmaf(wn[k], e_k, eb); a frame with one covering window takes that window's eps bits with no multiply.
// An observed element (mask != 0) is obs_coef[s + 1] (x0, z) of the first copy: obs_pin8 in a vector, obs_pin1 alone.
//
// NOISE (MODE 2).  coef rows are (cx, ce, sigma) as ib_ddim_step_noise takes them.  sigma == 0 is uniform over the launch:
// that row runs the deterministic update (ib_stitch_ddim_step bit for bit) and leaves z untouched.  Otherwise the normal z'
// of trial element (n, f, d) at step s is Box-Muller over Philox4x32-10 (philox.h) at counter
// ((f * D + d) >> 2, s, trial_id[n], kDomainStep), key = seed, the words paired as in diffusion.hip ((x, y) -> elements 0, 1
// and (z, w) -> elements 2, 3 of the block).  f is the TRIAL frame: every copy of an element gets the same normal by
// construction, and with W == 1 the key is the per-window sampler's with window id = trial id.  Pad columns (d >= D) get
// no noise.  A free element is fmaf(sigma, z', ddim_mix(...)).  An observed element updates its stored noise, read from the
// first copy of z, to b' = round_to_dtype(fmaf(r, b, q z')) with (r, q) = obs_noise_coef[s], written to every copy of z, and
// is pinned to fmaf(ox, a, oz b') with (ox, oz) = obs_coef[s + 1] -- the arithmetic of ddim_cond_step_noise_kernel.  A free
// element of a mixed vector gets back the z it had.
//
// DPM AND NOISE (MODE 3, ib_sde_dpmpp_step of sde.hip).  coef rows are (A, E, C, hx, he, G).  Per free element
// o = ddim_mix(A, x, E, eb), then fmaf(C, hist, o) in a row with C != 0, then fmaf(G, z', o) in a row with G != 0 on logical
// columns -- both branches uniform over the launch -- and hist = fmaf(hx, x, he * eb) goes to every copy; z' and the observed
// elements are MODE 2's, with G in sigma's place.  It is the same statements as MODE 1 and MODE 2, so a table with G == 0
// everywhere is ib_stitch_dpmpp_step and one with C == 0 everywhere ib_stitch_ddim_step_noise, bit for bit.
#include "stitch_step.h"

extern "C" int ib_stitch_ddim_step(void* x, const void* eps, const void* x0, const void* z, const uint8_t* mask,
                                   const float* coef, const float* obs_coef, const int64_t* timesteps, int64_t num_steps,
                                   int32_t step, const int32_t* step_dev, int64_t* t_out, const int32_t* start,
                                   const int32_t* cover, const float* wn, int64_t N, int64_t W, int64_t T, int64_t F,
                                   int64_t D, int64_t ld, int dtype, ib_stream_t stream) {
  return stitch_launch<0>(x, eps, nullptr, x0, const_cast<void*>(z), mask, coef, obs_coef, nullptr, timesteps, num_steps,
                          step, step_dev, t_out, start, cover, wn, nullptr, 0, N, W, T, F, D, ld, dtype, stream);
}

extern "C" int ib_stitch_dpmpp_step(void* x, const void* eps, float* hist, const void* x0, const void* z,
                                    const uint8_t* mask, const float* coef, const float* obs_coef, const int64_t* timesteps,
                                    int64_t num_steps, int32_t step, const int32_t* step_dev, int64_t* t_out,
                                    const int32_t* start, const int32_t* cover, const float* wn, int64_t N, int64_t W,
                                    int64_t T, int64_t F, int64_t D, int64_t ld, int dtype, ib_stream_t stream) {
  return stitch_launch<1>(x, eps, hist, x0, const_cast<void*>(z), mask, coef, obs_coef, nullptr, timesteps, num_steps,
                          step, step_dev, t_out, start, cover, wn, nullptr, 0, N, W, T, F, D, ld, dtype, stream);
}

extern "C" int ib_stitch_ddim_step_noise(void* x, const void* eps, const void* x0, void* z, const uint8_t* mask,
                                         const float* coef, const float* obs_coef, const float* obs_noise_coef,
                                         const int64_t* timesteps, int64_t num_steps, int32_t step, const int32_t* step_dev,
                                         int64_t* t_out, const int32_t* start, const int32_t* cover, const float* wn,
                                         const int64_t* trial_id, uint64_t seed, int64_t N, int64_t W, int64_t T, int64_t F,
                                         int64_t D, int64_t ld, int dtype, ib_stream_t stream) {
  return stitch_launch<2>(x, eps, nullptr, x0, z, mask, coef, obs_coef, obs_noise_coef, timesteps, num_steps, step,
                          step_dev, t_out, start, cover, wn, trial_id, seed, N, W, T, F, D, ld, dtype, stream);
}
