// Exhaustive host-side check of csrc/launch_geom.h: the one width rule against the seven predicates the launchers of
// csrc/diffusion.hip spelled out before they were folded (written out below as they stood: they are the oracle), the
// q_sample and step-noise block rules likewise, and the safety property of an 8-wide launch stated directly.  Includes only
// launch_geom.h; tests/test_launch_geom_cpu.py builds it with the host compiler and the address + undefined-behaviour
// sanitizers and runs it.  Prints the number of combinations checked; exits non-zero at the first mismatch.
#include "launch_geom.h"

#include <stdio.h>
#include <stdlib.h>

namespace {

struct Old { int64_t per, n; bool mix8, v8; };

bool al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) % 16) == 0; }

// ---- the seven predicates as the entry points had them
Old old_ddim_step(int64_t n, const void* x, const void* eps) {
  const bool v8 = (n % 8 == 0) && al16(x) && al16(eps);
  return Old{0, n, v8, v8};                          // its 8-wide kernel IS what mix8 names
}
Old old_ddim_cond_step(int64_t B, int64_t T, int64_t ld, const void* x, const void* eps, const void* x0, const void* z,
                       const uint8_t* mask) {
  const int64_t per = T * ld, n = B * per;
  const bool mix8 = (n % 8 == 0) && al16(x) && al16(eps);
  const bool v8 = mix8 && (per % 8 == 0) && al16(x0) && al16(z) && (reinterpret_cast<uintptr_t>(mask) % 8) == 0;
  return Old{per, n, mix8, v8};
}
Old old_ddim_cond_init(int64_t B, int64_t T, int64_t ld, const void* x, const void* x0, const void* z, const uint8_t* mask) {
  const int64_t per = T * ld, n = B * per;
  const bool v8 = (per % 8 == 0) && al16(x) && al16(x0) && al16(z) && (reinterpret_cast<uintptr_t>(mask) % 8) == 0;
  return Old{per, n, false, v8};                     // the start state has no update: the kernel is handed mix8 = 0
}
Old old_noise_launch(int64_t B, int64_t T, int64_t ld, const void* x, const void* eps, const void* x0, const void* z,
                     const uint8_t* mask) {         // both *_noise entries; the unmasked one passes null x0, z, mask
  Old L;
  L.per = T * ld; L.n = B * L.per;
  L.mix8 = (L.n % 8 == 0) && al16(x) && al16(eps);
  L.v8 = L.mix8 && (L.per % 8 == 0) && al16(x0) && al16(z) && (reinterpret_cast<uintptr_t>(mask) % 8) == 0;
  return L;
}
Old old_dpmpp_step(int64_t n, const void* x, const void* eps, const float* hist) {
  const bool mix8 = (n % 8 == 0) && al16(x) && al16(eps);
  const bool v8 = mix8 && al16(hist);
  return Old{0, n, mix8, v8};
}
Old old_dpmpp_cond_step(int64_t B, int64_t T, int64_t ld, const void* x, const void* eps, const float* hist, const void* x0,
                        const void* z, const uint8_t* mask) {
  const int64_t per = T * ld, n = B * per;
  const bool mix8 = (n % 8 == 0) && al16(x) && al16(eps);
  const bool v8 = mix8 && (per % 8 == 0) && al16(hist) && al16(x0) && al16(z) && (reinterpret_cast<uintptr_t>(mask) % 8) == 0;
  return Old{per, n, mix8, v8};
}
bool old_q_sample_v4(int64_t D, int64_t ld_xt, int dtype_is_bf16, const void* x0, const void* eps, const void* x_t) {
  const int es = dtype_is_bf16 ? 2 : 4;
  auto al = [&](const void* q) { return (reinterpret_cast<uintptr_t>(q) % (4 * es)) == 0; };
  return (D % 4 == 0) && (ld_xt % 4 == 0) && al(x0) && al(eps) && al(x_t);
}
bool old_blk(int64_t D, int64_t ld) { return (D % 4 == 0) && (ld == D || ld % 8 == 0); }

long long checked = 0;

void fail(const char* what, int64_t n, int64_t per) {
  printf("MISMATCH %s at n = %lld, per = %lld after %lld combinations\n", what, (long long)n, (long long)per, checked);
  exit(1);
}

// `init`: ib_ddim_cond_init, which takes the width from the rule and hands its kernel mix8 = 0 whatever the rule says
void same(const char* what, const Old& o, const SamplerGeom& g, bool init = false) {
  ++checked;
  if (o.per != g.per || o.n != g.n || o.v8 != g.v8 || o.mix8 != (init ? false : g.mix8)) fail(what, o.n, o.per);
}

// v8 sends 16-byte vector accesses to every operand there is, 8-byte words to the mask, and m0 = e0 % per to the mask and
// the generator: what must hold then, from the arguments alone
void safe(const char* what, const SamplerGeom& g, bool windows, const void* x, const void* eps, const void* hist,
          const void* x0, const void* z, const void* mask) {
  if (!g.v8) return;
  const void* vec[5] = {x, eps, hist, x0, z};
  for (const void* p : vec)
    if (p && reinterpret_cast<uintptr_t>(p) % 16 != 0) fail(what, g.n, g.per);
  if (mask && reinterpret_cast<uintptr_t>(mask) % 8 != 0) fail(what, g.n, g.per);
  if (g.n % 8 != 0) fail(what, g.n, g.per);
  if (windows && g.per % 8 != 0) fail(what, g.n, g.per);
}

}  // namespace

int main() {
  // one live buffer: every pointer handed to a rule is an address inside it (none is dereferenced)
  alignas(64) static unsigned char buf[6 * 64];
  const int OFF[5] = {0, 2, 4, 8, 16};                // byte offsets of x, eps, hist, x0, z from a 64-byte boundary
  const int MOFF[4] = {0, 1, 4, 8};                   // ... of the mask
  const void* const none = nullptr;

  for (int ix = 0; ix < 5; ++ix)
  for (int ie = 0; ie < 5; ++ie)
  for (int ih = 0; ih < 5; ++ih)
  for (int i0 = 0; i0 < 5; ++i0)
  for (int iz = 0; iz < 5; ++iz) {
    const void* x = buf + OFF[ix];
    const void* eps = buf + 64 + OFF[ie];
    const float* hist = reinterpret_cast<const float*>(buf + 128 + OFF[ih]);
    const void* x0 = buf + 192 + OFF[i0];
    const void* z = buf + 256 + OFF[iz];

    // no per-window structure: n in 1..64
    for (int64_t n = 1; n <= 64; ++n) {
      if (ih == 0 && i0 == 0 && iz == 0) {            // (operands the entry does not have: one pass, not 125)
        const SamplerGeom g = ib_sampler_geom(n, 0, x, eps, none, none, none, none);
        same("ib_ddim_step", old_ddim_step(n, x, eps), g);
        safe("ib_ddim_step", g, false, x, eps, none, none, none, none);
      }
      if (i0 == 0 && iz == 0) {
        const SamplerGeom g = ib_sampler_geom(n, 0, x, eps, hist, none, none, none);
        same("ib_dpmpp_step", old_dpmpp_step(n, x, eps, hist), g);
        safe("ib_dpmpp_step", g, false, x, eps, hist, none, none, none);
      }
    }

    // windows of per = T * ld elements: B in 1..3, per in 1..40 (T = 1, ld = per and, where per is even, T = 2)
    for (int64_t B = 1; B <= 3; ++B)
    for (int64_t per = 1; per <= 40; ++per)
    for (int64_t T = 1; T <= 2; ++T) {
      if (per % T) continue;
      const int64_t ld = per / T, n = B * per;
      if (ih == 0 && i0 == 0 && iz == 0) {
        const SamplerGeom g = ib_sampler_geom(n, per, x, eps, none, none, none, none);
        same("ib_ddim_step_noise", old_noise_launch(B, T, ld, x, eps, none, nullptr, nullptr), g);
        safe("ib_ddim_step_noise", g, true, x, eps, none, none, none, none);
      }
      for (int im = 0; im < 4; ++im) {
        const uint8_t* mask = buf + 320 + MOFF[im];
        if (ih == 0) {
          SamplerGeom g = ib_sampler_geom(n, per, x, eps, none, x0, z, mask);
          same("ib_ddim_cond_step", old_ddim_cond_step(B, T, ld, x, eps, x0, z, mask), g);
          same("ib_ddim_cond_step_noise", old_noise_launch(B, T, ld, x, eps, x0, z, mask), g);
          safe("ib_ddim_cond_step", g, true, x, eps, none, x0, z, mask);
          if (ie == 0) {
            g = ib_sampler_geom(n, per, x, none, none, x0, z, mask);
            same("ib_ddim_cond_init", old_ddim_cond_init(B, T, ld, x, x0, z, mask), g, true);
            safe("ib_ddim_cond_init", g, true, x, none, none, x0, z, mask);
          }
        }
        const SamplerGeom g = ib_sampler_geom(n, per, x, eps, hist, x0, z, mask);
        same("ib_dpmpp_cond_step", old_dpmpp_cond_step(B, T, ld, x, eps, hist, x0, z, mask), g);
        safe("ib_dpmpp_cond_step", g, true, x, eps, hist, x0, z, mask);
      }
    }
  }

  // ib_aligned itself: null is aligned to anything
  for (unsigned bytes = 1; bytes <= 16; bytes *= 2) {
    ++checked;
    if (!ib_aligned(nullptr, bytes)) fail("ib_aligned(null)", 0, bytes);
    for (unsigned o = 0; o < 32; ++o, ++checked)
      if (ib_aligned(buf + o, bytes) != (o % bytes == 0)) fail("ib_aligned", o, bytes);
  }

  // q_sample: D, ld_xt in 1..40 (ld_xt >= D), both element sizes, the three pointers at every offset
  for (int bf16 = 0; bf16 < 2; ++bf16)
  for (int ix = 0; ix < 5; ++ix)
  for (int ie = 0; ie < 5; ++ie)
  for (int it = 0; it < 5; ++it)
  for (int64_t D = 1; D <= 40; ++D)
  for (int64_t ld = D; ld <= 40; ++ld, ++checked) {
    const void *x0 = buf + OFF[ix], *eps = buf + 64 + OFF[ie], *xt = buf + 128 + OFF[it];
    const bool v4 = ib_q_sample_v4(D, ld, bf16 ? 2 : 4, x0, eps, xt);
    if (v4 != old_q_sample_v4(D, ld, bf16, x0, eps, xt)) fail("q_sample v4", D, ld);
    if (v4 && (D % 4 || ld % 4 || (OFF[ix] | OFF[ie] | OFF[it]) % (bf16 ? 8 : 16))) fail("q_sample v4 safety", D, ld);
  }

  // the block rule of the step noise
  for (int64_t D = 1; D <= 40; ++D)
  for (int64_t ld = D; ld <= 48; ++ld, ++checked)
    if (ib_step_noise_blk(D, ld) != old_blk(D, ld)) fail("blk", D, ld);

  printf("launch_geom_check: %lld combinations checked, all equal\n", checked);
  return 0;
}
