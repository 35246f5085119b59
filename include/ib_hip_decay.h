/* Decoupled weight decay (Loshchilov & Hutter; with Adam: torch.optim.AdamW) of the fused optimizer, applied INSIDE the
 * optimizer kernel to the parameter it has already loaded -- no pass over memory and no launch of its own, the rate of the
 * launch's own step under a replayed hipGraph, once per parameter per step however the step's launches divide the flat buffer.
 * The eleventh header of the C-ABI of libib_hip.so (csrc/optim.hip).  Conventions as in ib_hip.h (device pointers, a negative
 * IB_E_* code on error, the stream last); it includes ib_hip_sched.h, whose arguments its entries repeat.  It is a header of its
 * own so that the other ten and what is pinned to them stay as they are.  The binding parses it with the parser of ib_hip.h.
 *
 * The arithmetic.  lr_s is the fp32 rate the launch uses: lr, or the schedule's value (ib_hip_sched.h) where a schedule is
 * given.  wd = weight_decay >= 0, fp32.  For an element that is decayed:
 *   f  = (float)(1.0 - (double)lr_s * (double)wd)     in double, rounded to fp32 once
 *   p' = p * f                                        ONE fp32 multiply rounded on its own, never contracted into what follows
 *   p_new, s1, s2 = the update of `opt` applied to (p', g), the one the entries without decay apply to (p, g)
 * for all six optimizers.  An element that is not decayed gets that update of (p, g), bit for bit.  The bf16 shadow is
 * refreshed from p_new and the EMA advanced from p_new, as without decay.
 *
 * Which elements.  A table of n ranges [start_k, start_k + len_k) in GLOBAL coordinates of the flat parameter buffer, sorted and
 * disjoint, held in DEVICE memory and built once (ib_decay_table_build); every launch passes the same pointer plus `origin`, the
 * global offset of its p[0], so a captured graph holds constants.  The decision is per quad of 4 elements (a flat layout that
 * aligns every parameter to 16 bytes or more never lets a quad straddle two parameters): a start is a multiple of 4, a length
 * that is no multiple of 4 counts as rounded up to one (the padding behind a parameter belongs to it), and the n % 4 tail
 * elements of the plain form belong to quad n / 4.  The kernel finds a quad's range as it finds its gradient source: a
 * wave-uniform binary search from the wave's first element, then a short walk per lane.
 * Ranges of source kind 3 (updated by an earlier launch of this step) are left untouched: not decayed a second time.  Column-sum
 * ranges (kind 2) are decayed like any other; the padding lanes behind a ragged one keep their bits. */
#ifndef IB_HIP_DECAY_H
#define IB_HIP_DECAY_H

#include "ib_hip_sched.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of device memory a table of n ranges takes (n >= 0; never 0, so that an empty table can be allocated too); n < 0 -> 0 */
size_t ib_decay_table_bytes(int n);

/* Validates n ranges given as HOST arrays start[n], len[n] and uploads them to table_dev (ib_decay_table_bytes(n) bytes, 16-byte
 * aligned) on the stream; the host arrays may be released on return.  n = 0 uploads an empty table.  The only place the table can
 * be validated -- the step entries see a device pointer: n < 0, a null table_dev, null arrays with n > 0, a start that is
 * negative or no multiple of 4, a length <= 0, ranges that are unsorted or overlap (the rounded-up end of one beyond the start of
 * the next) -> IB_E_ARG, nothing is uploaded. */
int ib_decay_table_build(const int64_t* start, const int64_t* len, int n, void* table_dev, ib_stream_t stream);

/* ib_optim_step_sched / ib_optim_step_sources_sched (every argument as there; ema == NULL means no EMA) with decoupled weight
 * decay on the quads of p that the table covers: quad q of the launch is decayed if the global element origin + 4 q lies in a
 * range.  A constant schedule without warmup (sched_kind == IB_SCHED_CONSTANT, sched_warmup == 0) runs at the host's lr like the
 * entries without a schedule: lr_s = lr.  weight_decay == 0 or table_n == 0 decays nothing; p, s1, s2, the shadow and ema are
 * then bitwise those of the entry without decay.  weight_decay negative or NaN, table_n < 0, a null table_dev with table_n > 0,
 * origin negative or no multiple of 4, and every argument error of the _sched entries -> IB_E_ARG, nothing is launched. */
int ib_optim_step_decay(int opt, float* p, const float* g, float* s1, float* s2, int64_t n, float lr,
                        float grad_scale, int32_t step, int32_t* step_dev, int32_t* ticket, void* shadow_bf16,
                        float* ema, float ema_decay, int ema_warmup, int sched_kind, int32_t sched_warmup,
                        int32_t sched_total, float sched_min_ratio, float weight_decay, const void* table_dev,
                        int table_n, int64_t origin, ib_stream_t stream);
int ib_optim_step_sources_decay(int opt, float* p, const float* g, float* s1, float* s2, int64_t n, float lr,
                                float grad_scale, int32_t step, int32_t* step_dev, int32_t* ticket, void* shadow_bf16,
                                int nsrc, const int64_t* start, const int64_t* len, const int32_t* kind,
                                const void* const* base, const int64_t* stride, const int32_t* count, const float* scale,
                                const float* loss_col, int64_t loss_ld, int64_t loss_rows, float loss_scale,
                                float* loss_out, float* ema, float ema_decay, int ema_warmup, int sched_kind,
                                int32_t sched_warmup, int32_t sched_total, float sched_min_ratio, float weight_decay,
                                const void* table_dev, int table_n, int64_t origin, ib_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* IB_HIP_DECAY_H */
