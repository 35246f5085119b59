// The counter-based generator shared by the diffusion draw (noise.hip) and the stochastic sampler update (diffusion.hip):
// Philox4x32-10 (Salmon et al., SC'11) and Box-Muller over its words.  counter = (block, step, stream, domain), key = the
// 64-bit seed.  The domains keep the streams of one (seed, step, stream) apart: 0 = the eps / start draw, 1 = timesteps,
// 2 = the noise term of a sampling step (there `stream` is the window id and `step` the sampling step), 3 = the condition
// dropout of a training step (cfg.hip: `block` is the window's place in the batch, one decision per window), 4 = the re-noise
// of a resampling jump (resample.hip: `stream` is the trial id and `step` the ordinal of the jump within the sampling call).
#pragma once
#include "ib_common.h"

namespace {

constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u, kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;
constexpr uint32_t kDomainEps = 0u, kDomainT = 1u, kDomainStep = 2u, kDomainDrop = 3u;

struct U4 { uint32_t x, y, z, w; };

__device__ __forceinline__ U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(kM0, c.x), lo0 = kM0 * c.x;
    const uint32_t hi1 = __umulhi(kM1, c.z), lo1 = kM1 * c.z;
    c = U4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    k0 += kW0; k1 += kW1;
  }
  return c;
}

// (w, w') -> two N(0,1): u1 = (w + 1) / 2^32 in (0, 1], u2 = w' / 2^32 in [0, 1)
__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float& z0, float& z1) {
  // -2 ln u1 = -2 ln2 * log2(u1); u1 from the top 24 bits + 1 so the float conversion is exact and never 0
  const float u1 = (float)((a >> 8) + 1u) * 0x1.0p-24f;
  const float u2 = (float)(b >> 8) * 0x1.0p-24f;                  // revolutions: v_sin / v_cos take x / (2 pi)
  const float r = __builtin_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1));
  z0 = r * __builtin_amdgcn_cosf(u2);
  z1 = r * __builtin_amdgcn_sinf(u2);
}

}  // namespace
