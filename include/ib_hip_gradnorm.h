/* Clipping the gradient to a maximum global L2 norm (torch.nn.utils.clip_grad_norm_) inside the fused optimizer step: the norm
 * is taken on the device by one streaming launch, the clip coefficient never leaves the device, and the optimizer launch applies
 * it to the gradient it has already loaded -- a replayed hipGraph follows it with no host write and no host decision per step.
 * The thirteenth header of the C-ABI of libib_hip.so (csrc/optim.hip).  Conventions as in ib_hip.h (device pointers, a negative
 * IB_E_* code on error, the stream last); it includes ib_hip_decay.h, whose arguments its step entry repeats.  It is a header of
 * its own so that the other twelve and what is pinned to them stay as they are ("clip" is the x0 clip of ib_hip_clip.h, hence the
 * name).  The binding parses it with the parser of ib_hip.h.
 *
 * The arithmetic.  g is the flat fp32 gradient of n elements (under data parallelism the all-reduced SUM), grad_scale the factor
 * the optimizer folds in already (1 / world), max_norm > 0 (+inf allowed: measure, never clip).
 *   total  = sum of (double)g_i * (double)g_i       every product exact in double, accumulated in double, in the fixed order below
 *   norm_d = sqrt(total) * |(double)grad_scale|     the norm of the gradient the update sees
 *   coef_d = (double)max_norm / (norm_d + 1e-6)
 *   coef   = coef_d < 1 ? (float)coef_d : 1.0f      torch's rule; a NaN norm gives 1 (the gradient is NaN then anyway and the
 *                                                   parameters show it: nothing is hidden, no step is skipped)
 *   gs     = grad_scale * coef                      ONE fp32 multiply, rounded once
 * The update then uses g * gs where the other entries use g * grad_scale; at grad_scale = 1 that is torch's g.mul_(coef) exactly.
 * Every operation in double is rounded on its own (contraction off); grad_norm.clip_coef restates it on the host.
 *
 * The order of the sum.  It depends on n alone, never on the chip or the grid, and uses no atomics, so total is bit-reproducible.
 *   slots  G(n) = clamp(ceil(n / 16384), 1, 1024); slot length L(n) = ceil(ceil(n / G) / 1024) * 1024; slot s owns the elements
 *          [s L, min((s + 1) L, n)) -- possibly none, its sum is then +0.
 *   thread one workgroup of 256 threads per slot.  The slot is read as quads of 4 elements; thread t owns quads t, t + 256, ...
 *          (eight 16-byte loads requested together) and keeps FOUR accumulators, one per position in the quad, each advanced
 *          in quad order from +0.  The (slot length % 4) elements behind the last full quad -- only the last slot has any -- go
 *          one each to threads 0, 1, 2, into accumulator 0, 1, 2, after that thread's quads.  Thread sum = (a0 + a1) + (a2 + a3).
 *   group  the 256 thread sums are combined by the tree v[t] += v[t + h], h = 128, 64, ..., 1; v[0] is the slot's sum.
 *   total  the same workgroup shape over the slots: thread t adds slots t, t + 256, t + 512, t + 768 (those below G) in that order
 *          from +0, then the same tree.  Every workgroup of the clipped optimizer launch, and the probe, do exactly this.
 * ib_grad_sumsq only fills the slots; the kernel boundary behind it publishes them.  The reduction is not finished inside that
 * launch by a last-arriver hand-off: the per-XCD L2s are not coherent with each other within a launch. */
#ifndef IB_HIP_GRADNORM_H
#define IB_HIP_GRADNORM_H

#include "ib_hip_decay.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of the slot buffer for a gradient of n elements, 8 * G(n), never 0; n <= 0 -> 0 */
size_t ib_grad_sumsq_workspace(int64_t n);

/* slots[s] = the sum of squares of slot s of g[0, n), s < G(n): one streaming pass, one workgroup per slot.  g and slots 16-byte
 * aligned; slots holds ib_grad_sumsq_workspace(n) bytes.  A null or misaligned pointer, n <= 0 -> IB_E_ARG, nothing is launched. */
int ib_grad_sumsq(const float* g, int64_t n, double* slots, ib_stream_t stream);

/* The probe: one workgroup adds the G(n) slots as the clipped optimizer launch does and evaluates the arithmetic above by the
 * same device function.  *total_out = total, stats3[0..2] = {(float)norm_d, coef, gs}.  A null pointer or one that is not
 * 16-byte aligned, n <= 0, max_norm <= 0 or NaN -> IB_E_ARG, nothing is launched. */
int ib_grad_norm_eval(const double* slots, int64_t n, float grad_scale, float max_norm, double* total_out, float* stats3,
                      ib_stream_t stream);

/* ib_optim_step_decay (every argument as there, the plain form: no gradient sources) with the gradient clipped: every workgroup
 * adds the G(sumsq_n) slots that an ib_grad_sumsq launch over the WHOLE gradient left (sumsq_n is that launch's n; this launch may
 * cover a slice), puts gs in grad_scale's place and updates as ib_optim_step_decay does -- p, s1, s2, the shadow and ema are
 * bitwise those of ib_optim_step_decay called with grad_scale = gs.  Workgroup 0 writes stats3[0..2] = {(float)norm_d, coef, gs}.
 * slots or stats3 null or not 16-byte aligned, max_norm <= 0 or NaN, sumsq_n <= 0, and every argument error of
 * ib_optim_step_decay -> IB_E_ARG, nothing is launched. */
int ib_optim_step_gradnorm(int opt, float* p, const float* g, float* s1, float* s2, int64_t n, float lr,
                           float grad_scale, int32_t step, int32_t* step_dev, int32_t* ticket, void* shadow_bf16,
                           float* ema, float ema_decay, int ema_warmup, int sched_kind, int32_t sched_warmup,
                           int32_t sched_total, float sched_min_ratio, float weight_decay, const void* table_dev,
                           int table_n, int64_t origin, const double* slots, int64_t sumsq_n, float max_norm, float* stats3,
                           ib_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* IB_HIP_GRADNORM_H */
