/* Learning-rate schedules of the fused optimizer: warmup, then constant, linear or cosine decay, evaluated INSIDE the optimizer
 * kernel from the step number the launch already uses for the bias corrections -- so a replayed hipGraph follows the device
 * step counter.  The tenth header of the C-ABI of libib_hip.so (csrc/optim.hip).  Conventions as in ib_hip.h (device pointers,
 * a negative IB_E_* code on error, the stream last), which it includes.  It is a header of its own so that the other nine and
 * what is pinned to them stay as they are.  The binding parses it with the parser of ib_hip.h.
 *
 * The schedule.  s is the 1-based step number of the launch (*step_dev + 1 with a ticket, *step_dev + step with a counter,
 * step without one), w = sched_warmup >= 0, T = sched_total, m = sched_min_ratio in [0, 1].  All arithmetic is in double,
 * every operation rounded on its own (no fused multiply-add), only the result is rounded to fp32:
 *   f = s / w                                   if s <= w
 *   f = 1                                       if s >  w and kind == IB_SCHED_CONSTANT
 *   u = min(1, (s - w) / (T - w))               otherwise (T > w)
 *   f = m + (1 - m) * (1 - u)                   IB_SCHED_LINEAR
 *   f = m + (1 - m) * (0.5 * (1 + cos(pi * u))) IB_SCHED_COSINE
 *   lr_s = (float)((double)lr * f)
 * Step 1 runs at lr / w, step w at lr, step T and every later one at m * lr.  s - w is formed in double. */
#ifndef IB_HIP_SCHED_H
#define IB_HIP_SCHED_H

#include "ib_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IB_SCHED_CONSTANT 0
#define IB_SCHED_LINEAR 1
#define IB_SCHED_COSINE 2

/* ib_optim_step_ema / ib_optim_step_sources_ema (every argument as there) whose rate is lr_s of the schedule above instead of
 * lr: the kernel replaces lr once at its head and is otherwise the same update, so p, s1, s2, the shadow and ema are bitwise
 * those of the _ema entry called with lr = lr_s (ib_lr_schedule_eval gives that value).  ema == NULL is allowed here and
 * means no EMA (ema_decay and ema_warmup are then ignored).  sched_kind outside 0..2, sched_warmup < 0, sched_kind != 0 with
 * sched_total <= sched_warmup, sched_min_ratio outside [0, 1] or NaN -> IB_E_ARG, nothing is launched. */
int ib_optim_step_sched(int opt, float* p, const float* g, float* s1, float* s2, int64_t n, float lr,
                        float grad_scale, int32_t step, int32_t* step_dev, int32_t* ticket, void* shadow_bf16,
                        float* ema, float ema_decay, int ema_warmup, int sched_kind, int32_t sched_warmup,
                        int32_t sched_total, float sched_min_ratio, ib_stream_t stream);
int ib_optim_step_sources_sched(int opt, float* p, const float* g, float* s1, float* s2, int64_t n, float lr,
                                float grad_scale, int32_t step, int32_t* step_dev, int32_t* ticket, void* shadow_bf16,
                                int nsrc, const int64_t* start, const int64_t* len, const int32_t* kind,
                                const void* const* base, const int64_t* stride, const int32_t* count, const float* scale,
                                const float* loss_col, int64_t loss_ld, int64_t loss_rows, float loss_scale,
                                float* loss_out, float* ema, float ema_decay, int ema_warmup, int sched_kind,
                                int32_t sched_warmup, int32_t sched_total, float sched_min_ratio, ib_stream_t stream);

/* out[i] = lr_s at s = steps[i], i < n: one small launch of the device function the optimizer kernel itself calls (a probe
 * for tests and tools).  steps int32 [n], out fp32 [n]; the argument checks above, a null pointer or n <= 0 -> IB_E_ARG. */
int ib_lr_schedule_eval(float lr, int kind, int32_t warmup, int32_t total, float min_ratio, const int32_t* steps,
                        float* out, int64_t n, ib_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* IB_HIP_SCHED_H */
