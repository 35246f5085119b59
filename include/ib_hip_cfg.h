/* Classifier-free guidance (Ho & Salimans 2021): the fifth header of the C-ABI of libib_hip.so (csrc/cfg.hip).  Conventions
 * as in ib_hip.h (device pointers, a negative IB_E_* code on error, the stream last), which it includes.  The NULL CONDITION of
 * a denoiser conditioned on the first cond_cols columns of every frame (ib_q_sample_cond) is those columns all +0.  One entry
 * trains it (condition dropout), two are the seam of the guided sampling step.  A null pointer or a bad size is IB_E_ARG, an
 * unknown dtype IB_E_DTYPE, and nothing is launched.  It is a header of its own so that the other four and what is pinned to
 * them stay as they are.  The binding parses it with the parser of ib_hip.h. */
#ifndef IB_HIP_CFG_H
#define IB_HIP_CFG_H

#include "ib_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ib_q_sample_cond with a drop decision per window (its first fourteen arguments are that entry's; 0 <= cond_cols < D).
 * Window b is DROPPED iff (uint64)word0 < drop_threshold, word0 the first word of Philox4x32-10 at counter
 * (b, step + *step_dev, stream_id, domain 3), key = seed (step_dev NULL: step alone); drop_threshold in [0, 2^32] is
 * floor(p * 2^32), so 2^32 drops every window and 0 none.  The decision depends on (seed, step, stream_id, b) alone, not on B,
 * the pitch or the vector width.
 *   free columns c >= cond_cols:  ib_q_sample_cond's bits, exactly (the same width rule and the same rounding form)
 *   conditioning columns:         x0's bits in a kept window, +0 in a dropped one
 * drop_threshold == 0: the generator is not run and x_t is ib_q_sample_cond's bit for bit.  dropped_out (uint8 [B], may be
 * NULL) receives 1 for a dropped window and 0 for a kept one.  drop_threshold > 2^32: IB_E_ARG. */
int ib_q_sample_cond_drop(const void* x0, const void* eps, const int64_t* t, const float* sqrt_ab, const float* sqrt_1mab,
                          void* x_t, int64_t ld_xt, int64_t B, int64_t T, int64_t D, int64_t table_rows, int64_t cond_cols,
                          uint64_t seed, int32_t step, const int32_t* step_dev, uint32_t stream_id, uint64_t drop_threshold,
                          uint8_t* dropped_out, int dtype, ib_stream_t stream);

/* The guided noise prediction, in place over the pitched noise buffer eps [2B, T, ld]: windows 0 .. B-1 hold eps_c (the
 * conditional prediction), windows B .. 2B-1 eps_u (the prediction under the null condition).  Every element of the first
 * half, pad columns included, becomes, in fp32 with no contraction,
 *   d = ec - eu;  q = s * d;  g = ec + q;  round_to_dtype(g)
 * -- three roundings exactly as written.  The second half is not written.  A pad column that is +0 in both halves stays +0
 * for any finite s.  n = T * ld elements per window. */
int ib_cfg_combine(void* eps, float s, int64_t B, int64_t n, int dtype, ib_stream_t stream);

/* The guided step's input: over the state x [2B, T, ld] and the timestep vector t (int64 [2B]), the free columns
 * cond_cols <= c < D of window b are copied (bits, no arithmetic) to window B + b, and t[B + b] = t[b], b = 0 .. B-1.
 * Conditioning columns c < cond_cols and pad columns c >= D of the second half are never written: zero from allocation, they
 * are the null condition.  0 <= cond_cols < D <= ld. */
int ib_cfg_mirror(void* x, int64_t* t, int64_t B, int64_t T, int64_t D, int64_t ld, int64_t cond_cols, int dtype,
                  ib_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* IB_HIP_CFG_H */
