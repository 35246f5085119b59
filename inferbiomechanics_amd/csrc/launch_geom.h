// Launch geometry of the diffusion entry points (diffusion.hip): which vector width a launch takes.  Plain C++ over
// <stdint.h> alone, no HIP header, so a host compiler builds it by itself: tests/host/launch_geom_check.cpp sweeps every
// rule here against the seven predicates the launchers used to spell out one by one.
#pragma once
#include <stdint.h>

// a null pointer (an argument the entry point does not have) counts as aligned
static inline bool ib_aligned(const void* p, unsigned bytes) { return !p || reinterpret_cast<uintptr_t>(p) % bytes == 0; }

// THE WIDTH RULE of the sampler updates, for all seven of them (ib_ddim_step, ib_ddim_cond_step, ib_ddim_cond_init,
// ib_ddim_step_noise, ib_ddim_cond_step_noise, ib_dpmpp_step, ib_dpmpp_cond_step).
//   mix8: ib_ddim_step takes its 8-wide kernel on (n, x, eps).  Every other update hands it to its element-wise kernel,
//         which then rounds as that 8-wide kernel does: a sigma = 0 row, a C = 0 row and the free elements of a masked
//         update equal ib_ddim_step bit for bit whichever width either launch took.
//   v8:   this launch takes its own 8-wide kernel: mix8, and every further operand allows 16-byte vectors (the mask 8-byte
//         words), and no vector straddles two windows.
// n elements in all; per = elements per window (T * ld) where the update has a per-window structure (a mask, step noise),
// 0 where it has none (which asks nothing: 0 % 8 == 0).  An operand the entry point does not have is null.  A new
// operand gets its term HERE.
struct SamplerGeom { int64_t per, n; bool mix8, v8; };
static inline SamplerGeom ib_sampler_geom(int64_t n, int64_t per, const void* x, const void* eps, const void* hist,
                                          const void* x0, const void* z, const void* mask) {
  SamplerGeom g;
  g.per = per; g.n = n;
  g.mix8 = n % 8 == 0 && ib_aligned(x, 16) && ib_aligned(eps, 16);
  g.v8 = g.mix8 && per % 8 == 0 && ib_aligned(hist, 16) && ib_aligned(x0, 16) && ib_aligned(z, 16) && ib_aligned(mask, 8);
  return g;
}

// ib_q_sample and ib_q_sample_cond: 4 consecutive columns per thread (8 B bf16 / 16 B fp32) of rows of D columns, x_t at
// pitch ld_xt
static inline bool ib_q_sample_v4(int64_t D, int64_t ld_xt, int elemsize, const void* x0, const void* eps, const void* x_t) {
  const unsigned bytes = 4u * (unsigned)elemsize;
  return D % 4 == 0 && ld_xt % 4 == 0 && ib_aligned(x0, bytes) && ib_aligned(eps, bytes) && ib_aligned(x_t, bytes);
}

// step noise of an 8-wide update: an 8-vector is two whole Philox blocks (step_noise<8, true>) when D % 4 == 0 and every
// row starts on a multiple of 8, or there is no pitch
static inline bool ib_step_noise_blk(int64_t D, int64_t ld) { return D % 4 == 0 && (ld == D || ld % 8 == 0); }
