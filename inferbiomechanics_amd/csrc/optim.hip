// Fused optimizer step over ONE flat fp32 parameter buffer (one launch per step instead of
// torch.optim's per-tensor foreach kernels): torch.optim.{SGD,Adam,RMSprop,Adagrad,Adadelta,Adamax}
// with only lr set, as src/cli/train.py:183-194 constructs them.  The DDP mean (1/world) is folded
// in as grad_scale; an optional bf16 shadow of the parameters is refreshed in the same pass so the
// bf16 GEMMs never need a separate cast kernel.  With EMA on (optim_kernel<SRC, true>, the *_ema entries) the same pass also
// advances an exponential moving average of the parameters from the new value it already holds in registers: one more fp32
// read and write per parameter, no launch of its own, and the decay follows the device step counter under graph replay.
// Decoupled weight decay (the *_decay entries, include/ib_hip_decay.h; AdamW with Adam) multiplies the quads a range table
// covers by 1 - lr_s * wd in the same pass, before the update: optim_kernel<SRC, EMA, ..., DecayArgs>.
#include "ib_common.h"
#include "../../include/ib_hip_gradnorm.h"
#include <type_traits>
#include <vector>

namespace {

struct OptArgs {
  float* p; const float* g; float* s1; float* s2; bf16_t* shadow;
  int64_t n; float lr; float gscale; int step; int32_t* step_dev; int32_t* ticket; int opt;
  float* ema; float ema_decay; int ema_warmup;     // read by optim_kernel<SRC, true> only
};

// Gradient SOURCES (ib_optim_step_sources): ranges of the flat buffer whose gradient is still a set of partial sums when
// the optimizer runs -- the split-M slabs of a weight-gradient GEMM, or per-workgroup partial rows (column sums).  The
// optimizer sums them itself, in the same fixed order as ib_step_reduce, so the reduction launch, its kernel boundary
// and the round trip of the reduced gradient through HBM disappear (single-GPU steps only: an all-reduce needs the
// reduced gradient in memory).
constexpr int OPT_TICKET_SUBS = 32, OPT_TICKET_LINE = 32;     // sub-counters, int32 words per 128-byte line
constexpr int OPT_MAXSRC = 64;   // 4 transformer layers x (4 slab sets + 4 bias sums + 4 LayerNorm sums) + the projections
struct GradSrc {
  int64_t start, len;          // flat element range (start % 4 == 0)
  const float* base;           // slabs: [nslab][len] ; column sums: part + col0
  int64_t stride;              // slabs: elements between slabs ; column sums: row pitch of part
  int count;                   // slabs: nslab ; column sums: rows
  int kind;                    // 1 = slabs, 2 = column sums, 3 = none: the range was updated by an earlier launch of this step
  float scale;
};
struct OptSources {
  GradSrc s[OPT_MAXSRC]; int n;
  const float* loss_col; int64_t loss_ld; int loss_rows; float loss_scale; float* loss_out;   // optional scalar
};

// Learning-rate schedule (include/ib_hip_sched.h states it): warmup s / w, then 1, a linear or a cosine decay to m over
// steps w .. T, clamped beyond T.  Double throughout, every operation rounded on its own (contraction off: the host's
// restatement, lr_schedule.LrSchedule.lr_at, is then bitwise this except for the last place of cos), the result rounded to
// fp32 once.  s is wave-uniform; the cosine is evaluated only on the decay of a cosine schedule (w < s < T).
struct SchedArgs { int kind; int32_t warmup, total; float min_ratio; };

__device__ __forceinline__ float lr_scheduled(float lr, const SchedArgs& sc, int s) {
#pragma clang fp contract(off)
  const double sd = (double)s, wd = (double)sc.warmup;
  double f = 1.0;
  if (s <= sc.warmup) {
    f = sd / wd;
  } else if (sc.kind != IB_SCHED_CONSTANT && s >= sc.total) {
    f = (double)sc.min_ratio;                    // u = 1: m + (1 - m) * 0, without asking cos(pi) for an exact -1
  } else if (sc.kind != IB_SCHED_CONSTANT) {
    const double u = (sd - wd) / ((double)sc.total - wd);
    const double m = (double)sc.min_ratio;
    const double shape = sc.kind == IB_SCHED_COSINE ? 0.5 * (1.0 + cos(3.14159265358979323846 * u)) : 1.0 - u;
    f = m + (1.0 - m) * shape;
  }
  return (float)((double)lr * f);
}

// Decoupled weight decay (include/ib_hip_decay.h states it): f = (float)(1 - lr_s * wd) in double (the product of two fp32 values
// is exact there, so f is rounded once), p' = p * f as a multiply of its own -- contraction is off in decay_mul, so the
// product carries no `contract` flag and cannot be fused into the update's subtraction -- then the update of (p', g).
// table: n pairs (start, end) of int64 in device memory, global flat-buffer coordinates, sorted and disjoint, every bound a
// multiple of 4 (ib_decay_table_build rounds the ends up); origin: the global offset of this launch's p[0].
struct DecayArgs { float wd; int n; const int64_t* table; int64_t origin; };

__device__ __forceinline__ float decay_factor(float lr, float wd) {
#pragma clang fp contract(off)
  return (float)(1.0 - (double)lr * (double)wd);
}

__device__ __forceinline__ float decay_mul(float p, float f) {
#pragma clang fp contract(off)
  return p * f;
}

// The quad as the update sees it: p * f where `dec` holds, p's own bits elsewhere, handed on through an empty asm that the
// compiler cannot look through.  Without it the multiply and the select in front of the update changed how the update
// itself was vectorised and contracted (Adam's s1 and p came out one rounding apart from the launch without decay, on
// undecayed elements too); behind it the update starts from four opaque registers, as it does behind the load of p.
__device__ __forceinline__ float4 decay4(float4 p, bool dec, float f) {
  typedef float f4v __attribute__((ext_vector_type(4)));
  f4v v;
  v.x = dec ? decay_mul(p.x, f) : p.x; v.y = dec ? decay_mul(p.y, f) : p.y;
  v.z = dec ? decay_mul(p.z, f) : p.z; v.w = dec ? decay_mul(p.w, f) : p.w;
  asm("" : "+v"(v));
  return make_float4(v.x, v.y, v.z, v.w);
}

// is the quad at local element idx decayed?  As source_grad4 finds a gradient source: the wave's first element picks the first
// range that ends beyond it by a UNIFORM binary search (the active lane with the lowest index holds the lowest element), each
// lane walks on from there.
__device__ __forceinline__ bool decayed4(const DecayArgs& D, int64_t idx) {
  const int64_t gi = D.origin + idx;
  const int64_t g0 = ((int64_t)__builtin_amdgcn_readfirstlane((int)(gi >> 32)) << 32) |
                     (uint32_t)__builtin_amdgcn_readfirstlane((int)(gi & 0xffffffff));
  int lo = 0, hi = D.n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (D.table[2 * mid + 1] <= g0) lo = mid + 1; else hi = mid;
  }
  for (int j = lo; j < D.n; ++j) {
    if (gi < D.table[2 * j]) break;
    if (gi < D.table[2 * j + 1]) return true;
  }
  return false;
}

// ---- clipping to a global gradient norm (include/ib_hip_gradnorm.h states the arithmetic and the order of every sum) --------
// The slot layout is a function of n alone: G slots of L elements, L a multiple of 1024 (every slot starts 16-byte aligned).
constexpr int64_t GN_SLOT_ELEMS = 16384, GN_SLOT_ALIGN = 1024;
constexpr int GN_MAX_SLOTS = 1024;
inline int gn_slots(int64_t n) {
  const int64_t G = n / GN_SLOT_ELEMS + (n % GN_SLOT_ELEMS != 0);
  return (int)(G < 1 ? 1 : G > GN_MAX_SLOTS ? GN_MAX_SLOTS : G);
}
inline int64_t gn_slot_len(int64_t n, int G) {
  const int64_t per = n / G + (n % G != 0);
  return (per / GN_SLOT_ALIGN + (per % GN_SLOT_ALIGN != 0)) * GN_SLOT_ALIGN;
}

// the product of two fp32 values is exact in double, so a0 += gn_sq(x) rounds once whether or not it becomes an fma
__device__ __forceinline__ double gn_sq(float x) { const double d = (double)x; return d * d; }

// the workgroup's 256 thread sums: v[t] += v[t + h], h = 128, 64, ..., 1; every thread returns v[0]
__device__ __forceinline__ double gn_tree256(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  return red[0];
}

// one workgroup per slot, one pass: 16-byte loads, eight in flight per lane, four accumulators per thread (one per position in
// the quad), the slot's ragged end (only the last slot has one) element by element on threads 0..2
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, int64_t n, int64_t L,
                                                         double* __restrict__ slots) {
  __shared__ double red[256];
  const int64_t b = (int64_t)blockIdx.x * L;
  const int64_t len = b < n ? (n - b < L ? n - b : L) : 0;
  const int64_t nq = len >> 2;
  const float4* q = reinterpret_cast<const float4*>(g + b);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (int64_t k = threadIdx.x; k < nq; k += 256 * 8) {
    float4 v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (k + e * 256 < nq) v[e] = q[k + e * 256];
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (k + e * 256 < nq) { a0 += gn_sq(v[e].x); a1 += gn_sq(v[e].y); a2 += gn_sq(v[e].z); a3 += gn_sq(v[e].w); }
  }
  if ((int64_t)threadIdx.x < (len & 3)) {
    const double s = gn_sq(g[b + 4 * nq + threadIdx.x]);
    if (threadIdx.x == 0) a0 += s; else if (threadIdx.x == 1) a1 += s; else a2 += s;
  }
  const double t = gn_tree256((a0 + a1) + (a2 + a3), red);
  if (threadIdx.x == 0) slots[blockIdx.x] = t;
}

// total of the G <= 1024 slots, by every workgroup that needs it: thread t adds slots t, t + 256, ... in order, then the tree
__device__ __forceinline__ double gn_total(const double* slots, int G, double* red) {
  double v = 0.0;
  for (int s = threadIdx.x; s < G; s += 256) v += slots[s];
  return gn_tree256(v, red);
}

// the header's arithmetic, every double operation rounded on its own; a NaN or infinite coef_d fails the comparison: coef = 1
struct ClipOut { float norm, coef, gs; };
__device__ __forceinline__ ClipOut grad_clip(double total, float gscale, float max_norm) {
#pragma clang fp contract(off)
  const double norm_d = sqrt(total) * fabs((double)gscale);
  const double coef_d = (double)max_norm / (norm_d + 1e-6);
  const float coef = coef_d < 1.0 ? (float)coef_d : 1.0f;
  return ClipOut{(float)norm_d, coef, gscale * coef};
}

// the probe: total and {norm, coef, gs} as the clipped launch below gets them
__global__ __launch_bounds__(256) void grad_norm_eval_kernel(const double* slots, int G, float gscale, float max_norm,
                                                             double* __restrict__ total_out, float* __restrict__ stats) {
  __shared__ double red[256];
  const double total = gn_total(slots, G, red);
  const ClipOut k = grad_clip(total, gscale, max_norm);
  if (threadIdx.x == 0) { *total_out = total; stats[0] = k.norm; stats[1] = k.coef; stats[2] = k.gs; }
}

// the clipped launch's own arguments: the slots ib_grad_sumsq left, their count, the bound, where {norm, coef, gs} go
struct ClipArgs { const double* slots; int G; float max_norm; float* stats; };

// the optional trailing arguments of optim_kernel: is T among them, and which one is it
template <typename T, typename... P> constexpr bool pack_has = (std::is_same<T, P>::value || ...);
template <typename T, typename F, typename... R>
__device__ __forceinline__ const T& pack_get(const F& f, const R&... r) {
  if constexpr (std::is_same<T, F>::value) return f; else return pack_get<T>(r...);
}

__device__ __forceinline__ float opt_update(const OptArgs& a, float p, float g, float& s1, float& s2, float bc1,
                                            float bc2s) {
  switch (a.opt) {
    case IB_OPT_SGD: return p - a.lr * g;
    case IB_OPT_ADAM: {
      s1 = 0.9f * s1 + 0.1f * g;                 // exp_avg
      s2 = 0.999f * s2 + 0.001f * g * g;         // exp_avg_sq
      const float denom = sqrtf(s2) / bc2s + 1e-8f;
      return p - (a.lr / bc1) * (s1 / denom);
    }
    case IB_OPT_RMSPROP: {
      s1 = 0.99f * s1 + 0.01f * g * g;           // square_avg
      return p - a.lr * (g / (sqrtf(s1) + 1e-8f));
    }
    case IB_OPT_ADAGRAD: {
      s1 = s1 + g * g;
      return p - a.lr * (g / (sqrtf(s1) + 1e-10f));
    }
    case IB_OPT_ADADELTA: {
      s1 = 0.9f * s1 + 0.1f * g * g;             // square_avg
      const float delta = sqrtf(s2 + 1e-6f) / sqrtf(s1 + 1e-6f) * g;
      s2 = 0.9f * s2 + 0.1f * delta * delta;     // acc_delta
      return p - a.lr * delta;
    }
    case IB_OPT_ADAMAX: {
      s1 = 0.9f * s1 + 0.1f * g;                 // exp_avg
      s2 = fmaxf(0.999f * s2, fabsf(g) + 1e-8f); // exp_inf
      return p - (a.lr / bc1) * (s1 / s2);
    }
    default: return p;
  }
}

// ema <- d * ema + (1 - d) * p_new as ONE fma over the rounded product: d = 0 gives p_new and d = 1 the old ema, bit for bit
__device__ __forceinline__ float ema_update(float d, float e, float p) { return __fmaf_rn(d, e, (1.f - d) * p); }

// The EMA reads the new parameters back through a volatile load of what this thread has just stored (an L2 hit), not
// from the registers of the update: used there, they changed how the compiler vectorised and contracted the update
// itself (p and s1 of Adam's column-sum ranges came out one rounding apart from the launch without the EMA).  This way
// the update is the same code in both instantiations, bit for bit.
__device__ __forceinline__ void ema4(const OptArgs& a, float d, int64_t i, int nvalid) {
  typedef float f4v __attribute__((ext_vector_type(4)));
  const f4v p = *reinterpret_cast<const volatile f4v*>(a.p + 4 * i);
  float4 e = reinterpret_cast<float4*>(a.ema)[i];
  e.x = ema_update(d, e.x, p.x);
  if (nvalid >= 2) e.y = ema_update(d, e.y, p.y);
  if (nvalid >= 3) e.z = ema_update(d, e.z, p.z);
  if (nvalid >= 4) e.w = ema_update(d, e.w, p.w);
  reinterpret_cast<float4*>(a.ema)[i] = e;
}

// slab-backed ranges are summed by whichever thread owns the element; column-sum ranges are left to the dedicated
// cooperative blocks below (a single thread summing 256 strided rows was a 100-us tail)
// (the host passes the sources sorted by start).  Two things made this path 40 us of the transformer's 111-us launch
// beyond its bytes (48 sources, 126 MB of slabs): every thread walked the source list from its head -- up to 48 dependent
// scalar loads before its first vector load -- and a slab count below 8 (2 for most transformer weights) fell into a
// rolled one-load-per-trip loop, i.e. `count` HBM round trips in sequence.  Now the wave finds its first candidate by a
// UNIFORM binary search (6 scalar steps) and every batch of up to 8 slabs is requested at once (predicated on the count), the sum still runs strictly in slab order
// (= ib_step_reduce / slab_reduce_multi, bitwise).
__device__ __forceinline__ bool source_grad4(const OptSources& S, const float* g, int64_t idx, float4& t) {
  const int64_t idx0 = ((int64_t)__builtin_amdgcn_readfirstlane((int)(idx >> 32)) << 32) |
                       (uint32_t)__builtin_amdgcn_readfirstlane((int)(idx & 0xffffffff));
  int lo = 0, hi = S.n;                        // first source whose end lies beyond the wave's first element
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (S.s[mid].start + S.s[mid].len <= idx0) lo = mid + 1; else hi = mid;
  }
  for (int j = lo; j < S.n; ++j) {
    const GradSrc& r = S.s[j];
    if (idx < r.start) break;
    if (idx < r.start + r.len) {
      if (r.kind != 1) return false;
      const int64_t o = idx - r.start;
      t = make_float4(0.f, 0.f, 0.f, 0.f);
      const float4* q = reinterpret_cast<const float4*>(r.base + o);
      const int64_t st4 = r.stride >> 2;
      for (int k = 0; k < r.count; k += 8) {  // up to 8 slabs in flight, added strictly in sequence
        float4 v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (k + e < r.count) v[e] = q[(int64_t)(k + e) * st4];
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (k + e < r.count) { t.x += v[e].x; t.y += v[e].y; t.z += v[e].z; t.w += v[e].w; }
      }
      return true;
    }
  }
  t = *reinterpret_cast<const float4*>(g + idx);
  return true;
}

template <bool EMA, bool DECAY = false>
__device__ __forceinline__ void apply4(const OptArgs& a, int64_t i, float4 g, float bc1, float bc2s, float d, int nvalid,
                                       bool dec = false, float f = 1.f) {
  // nvalid < 4 only at the ragged end of a column-sum range (the remaining lanes belong to alignment padding: they get back
  // the bits they had, p0, from before the decay)
  const bool has1 = a.s1 != nullptr, has2 = a.s2 != nullptr;
  float4 p = reinterpret_cast<float4*>(a.p)[i];
  float4 s1 = has1 ? reinterpret_cast<float4*>(a.s1)[i] : make_float4(0, 0, 0, 0);
  float4 s2 = has2 ? reinterpret_cast<float4*>(a.s2)[i] : make_float4(0, 0, 0, 0);
  const float4 p0 = p, s10 = s1, s20 = s2;
  if constexpr (DECAY) p = decay4(p, dec, f);
  p.x = opt_update(a, p.x, g.x * a.gscale, s1.x, s2.x, bc1, bc2s);
  p.y = opt_update(a, p.y, g.y * a.gscale, s1.y, s2.y, bc1, bc2s);
  p.z = opt_update(a, p.z, g.z * a.gscale, s1.z, s2.z, bc1, bc2s);
  p.w = opt_update(a, p.w, g.w * a.gscale, s1.w, s2.w, bc1, bc2s);
  if (nvalid < 4) { p.w = p0.w; s1.w = s10.w; s2.w = s20.w; }
  if (nvalid < 3) { p.z = p0.z; s1.z = s10.z; s2.z = s20.z; }
  if (nvalid < 2) { p.y = p0.y; s1.y = s10.y; s2.y = s20.y; }
  reinterpret_cast<float4*>(a.p)[i] = p;
  if (has1) reinterpret_cast<float4*>(a.s1)[i] = s1;
  if (has2) reinterpret_cast<float4*>(a.s2)[i] = s2;
  if (a.shadow) {
    bf16x4_t o;
    o[0] = (bf16_t)p.x; o[1] = (bf16_t)p.y; o[2] = (bf16_t)p.z; o[3] = (bf16_t)p.w;
    reinterpret_cast<bf16x4_t*>(a.shadow)[i] = o;
  }
  if constexpr (EMA) ema4(a, d, i, nvalid);
}

// SRC: blocks [0, main_blocks) walk the flat buffer (skipping column-sum ranges); block main_blocks + b owns 64 columns of
// a column-sum range: 16 float4 columns x 16 row groups, LDS combine in the order of colsum_segments_kernel, update.
// EMA: every element this launch updates also updates a.ema (kind-3 ranges leave both untouched); EMA = false is the
// kernel without it, instruction for instruction.
// Sched: empty for the kernel as it always was -- optim_kernel<SRC, EMA> has the argument list (a, S, main_blocks) and the
// instructions it had -- or one SchedArgs behind main_blocks: the rate of this launch is then the schedule's (lr_scheduled
// above, from the step number of the bias corrections), put in a.lr's place once at the head.  One kernel template and not a
// body shared by two kernels: inlined from a device function the same statements compiled to other code (blockDim.x is
// lowered there without the kernel's uniform-work-group-size attribute, and the sources form came out scheduled differently).
// The pack's second optional element, behind SchedArgs where there is one, is a DecayArgs: every quad this launch updates
// whose global position lies in a range of D.table is multiplied by f = decay_factor(lr_s, wd) before its update (kind-3
// ranges are skipped before that, as before any other work).  Without it: the functions above, instruction for instruction.
// The pack's third optional element, only behind both others and only with SRC = false (the clip needs the materialised
// gradient), is a ClipArgs: a head in front of everything else puts gs = grad_scale * coef in grad_scale's place.  Every
// workgroup adds the slots itself (8 KB of L2 hits at most) and evaluates grad_clip, so the coefficient needs no launch and
// no host read of its own; block 0 writes {norm, coef, gs}; gs is handed on as a wave-uniform value (readfirstlane), as the
// kernel argument it replaces is.  This form always carries a SchedArgs, so it tests at run time for the constant schedule
// without warmup, where the rate is the host's lr as in the forms without a SchedArgs; an empty table decays nothing.
template <bool SRC, bool EMA, typename... Sched>
__global__ __launch_bounds__(256) void optim_kernel(OptArgs a, OptSources S, int main_blocks, Sched... sc) {
  static_assert(std::is_same<void(Sched...), void()>::value || std::is_same<void(Sched...), void(SchedArgs)>::value ||
                std::is_same<void(Sched...), void(DecayArgs)>::value ||
                std::is_same<void(Sched...), void(SchedArgs, DecayArgs)>::value ||
                (!SRC && std::is_same<void(Sched...), void(SchedArgs, DecayArgs, ClipArgs)>::value),
                "(), (SchedArgs), (DecayArgs), both in this order, or both and a ClipArgs without sources");
  constexpr bool SCHED = pack_has<SchedArgs, Sched...>, DECAY = pack_has<DecayArgs, Sched...>;
  constexpr bool CLIP = pack_has<ClipArgs, Sched...>;
  if constexpr (CLIP) {
    __shared__ double red[256];
    const ClipArgs& c = pack_get<ClipArgs>(sc...);
    const ClipOut k = grad_clip(gn_total(c.slots, c.G, red), a.gscale, c.max_norm);
    if (blockIdx.x == 0 && threadIdx.x == 0) { c.stats[0] = k.norm; c.stats[1] = k.coef; c.stats[2] = k.gs; }
    a.gscale = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, k.gs)));
  }
  // self-counting mode (ticket != NULL): *step_dev holds the number of COMPLETED steps; every block reads it on
  // entry, and the block that draws the last exit ticket publishes step and resets the ticket -- it exits after
  // every other block has entered (and therefore read the old value), so no block can see the new count.
  // step_dev without a ticket: step = *step_dev + a.step, nothing published -- a.step = 1 is how a launch over PART of
  // the buffer (a layer's range, issued as soon as its gradient is complete) takes part in a self-counting step whose
  // last launch publishes.
  const int step = a.step_dev ? *(volatile int32_t*)a.step_dev + (a.ticket ? 1 : a.step) : a.step;
  if constexpr (SCHED) {
    const SchedArgs& q = pack_get<SchedArgs>(sc...);
    if (!CLIP || !(q.kind == IB_SCHED_CONSTANT && q.warmup == 0)) a.lr = lr_scheduled(a.lr, q, step);
  }
  DecayArgs D{};
  float f = 1.f;                                 // the decay's factor, from the rate this launch uses
  if constexpr (DECAY) { D = pack_get<DecayArgs>(sc...); f = decay_factor(a.lr, D.wd); }
  // bias corrections in double (torch computes them as Python floats) -- Adam / Adamax only: two double-precision pow()
  // are several hundred instructions at the head of every thread, ahead of its first load
  float bc1 = 1.f, bc2s = 1.f;
  if (a.opt == IB_OPT_ADAM || a.opt == IB_OPT_ADAMAX) {
    bc1 = (float)(1.0 - pow(0.9, (double)step));
    bc2s = (float)sqrt(1.0 - pow(0.999, (double)step));
  }
  // EMA decay from the same step number (warmup: min(D, (1 + step) / (10 + step))), in double, rounded once
  float d = 0.f;
  if constexpr (EMA)
    d = (float)(a.ema_warmup ? fmin((double)a.ema_decay, (1.0 + step) / (10.0 + step)) : (double)a.ema_decay);
  const int64_t n4 = a.n / 4;
  const bool has1 = a.s1 != nullptr, has2 = a.s2 != nullptr;
  // the column-sum blocks are long dependent chains (256 strided rows each): they take the FIRST physical block ids so
  // they start at once and overlap the streaming blocks instead of forming the launch's tail
  const int ncs = SRC ? (int)gridDim.x - main_blocks : 0;
  const int lb = SRC ? ((int)blockIdx.x < ncs ? main_blocks + (int)blockIdx.x : (int)blockIdx.x - ncs) : (int)blockIdx.x;
  if (SRC && lb >= main_blocks) {
    __shared__ float4 red[16][16];
    int rb = lb - main_blocks, j = 0;
    for (; j < S.n; ++j) {                      // which column-sum range, which 64-column chunk of it
      if (S.s[j].kind != 2) continue;
      const int nb = (int)((S.s[j].len + 63) / 64);
      if (rb < nb) break;
      rb -= nb;
    }
    if (j < S.n) {
      const GradSrc& r = S.s[j];
      const int c4 = threadIdx.x & 15, rg = threadIdx.x >> 4;
      const int64_t o = (int64_t)rb * 64 + 4 * c4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (o < r.len) {
        const float* q = r.base + o;
        if (o + 4 <= r.len) {
          // rows rg, rg + 16, ...: batches of 8 requested together, added strictly in row order (= colsum_segments_kernel)
          v = ib_rows_sum4(q, r.stride, rg, 16, r.count);
        } else {
          for (int row = rg; row < r.count; row += 16) {
            const float* w = q + (int64_t)row * r.stride;
            v.x += w[0];
            if (o + 1 < r.len) v.y += w[1];
            if (o + 2 < r.len) v.z += w[2];
          }
        }
      }
      red[rg][c4] = v;
      __syncthreads();
      if (rg == 0 && o < r.len) {
        float4 t = red[0][c4];
#pragma unroll
        for (int k = 1; k < 16; ++k) { const float4 w = red[k][c4]; t.x += w.x; t.y += w.y; t.z += w.z; t.w += w.w; }
        t.x *= r.scale; t.y *= r.scale; t.z *= r.scale; t.w *= r.scale;
        if constexpr (DECAY)
          apply4<EMA, true>(a, (r.start + o) >> 2, t, bc1, bc2s, d, (int)min((int64_t)4, r.len - o),
                            decayed4(D, r.start + o), f);
        else
          apply4<EMA>(a, (r.start + o) >> 2, t, bc1, bc2s, d, (int)min((int64_t)4, r.len - o));
      }
    }
  } else {
  const int64_t gstride = (int64_t)(SRC ? main_blocks : (int)gridDim.x) * blockDim.x;
  for (int64_t i = (int64_t)lb * blockDim.x + threadIdx.x; i < n4; i += gstride) {
    float4 p = reinterpret_cast<float4*>(a.p)[i];
    float4 g;
    if constexpr (SRC) {
      if (!source_grad4(S, a.g, i * 4, g)) continue;
    } else {
      g = reinterpret_cast<const float4*>(a.g)[i];
    }
    float4 s1 = has1 ? reinterpret_cast<float4*>(a.s1)[i] : make_float4(0, 0, 0, 0);
    float4 s2 = has2 ? reinterpret_cast<float4*>(a.s2)[i] : make_float4(0, 0, 0, 0);
    if constexpr (DECAY) p = decay4(p, decayed4(D, i * 4), f);
    p.x = opt_update(a, p.x, g.x * a.gscale, s1.x, s2.x, bc1, bc2s);
    p.y = opt_update(a, p.y, g.y * a.gscale, s1.y, s2.y, bc1, bc2s);
    p.z = opt_update(a, p.z, g.z * a.gscale, s1.z, s2.z, bc1, bc2s);
    p.w = opt_update(a, p.w, g.w * a.gscale, s1.w, s2.w, bc1, bc2s);
    reinterpret_cast<float4*>(a.p)[i] = p;
    if (has1) reinterpret_cast<float4*>(a.s1)[i] = s1;
    if (has2) reinterpret_cast<float4*>(a.s2)[i] = s2;
    if (a.shadow) {
      bf16x4_t o;
      o[0] = (bf16_t)p.x; o[1] = (bf16_t)p.y; o[2] = (bf16_t)p.z; o[3] = (bf16_t)p.w;
      reinterpret_cast<bf16x4_t*>(a.shadow)[i] = o;
    }
    if constexpr (EMA) ema4(a, d, i, 4);
  }
  // tail (n % 4)
  const int64_t t0 = n4 * 4;
  for (int64_t i = t0 + (int64_t)lb * blockDim.x + threadIdx.x; i < a.n; i += gstride) {
    float s1 = has1 ? a.s1[i] : 0.f, s2 = has2 ? a.s2[i] : 0.f;
    float pi = a.p[i];
    if constexpr (DECAY) {
      if (decayed4(D, t0)) pi = decay_mul(pi, f);              // the tail belongs to quad n / 4
      asm("" : "+v"(pi));
    }
    const float p = opt_update(a, pi, a.g[i] * a.gscale, s1, s2, bc1, bc2s);
    a.p[i] = p;
    if (has1) a.s1[i] = s1;
    if (has2) a.s2[i] = s2;
    if (a.shadow) a.shadow[i] = (bf16_t)p;
    if constexpr (EMA) a.ema[i] = ema_update(d, a.ema[i], *(const volatile float*)(a.p + i));
  }
  }   // main blocks
  if constexpr (SRC) {
    if (S.loss_out && lb == 0) {       // the step's loss scalar: one column of the partial rows, fixed order
      __shared__ float lred[16];
      float v = 0.f;
      const int rg = threadIdx.x >> 4;
      if ((threadIdx.x & 15) == 0)
        for (int r = rg; r < S.loss_rows; r += 16) v += S.loss_col[(int64_t)r * S.loss_ld];
      if ((threadIdx.x & 15) == 0) lred[rg] = v;
      __syncthreads();
      if (threadIdx.x == 0) {
        float t = lred[0];
#pragma unroll
        for (int k = 1; k < 16; ++k) t += lred[k];
        *S.loss_out = t * S.loss_scale;
      }
    }
  }
  if (a.ticket) {
    // Exit tickets, two levels: 1137 blocks (the MLP denoiser's flat buffer) drawing from ONE word were 1137 returning
    // atomics on one address, serialised in L2 at ~11 ns each -- 12 of the launch's 17 us.  Block b draws from sub-counter
    // b % 32 (its own 128-byte line: different lines pipeline); the last arriver of a sub-counter resets it and draws from
    // the top word; the last of those publishes.  The longest same-address chain is grid / 32 + 32 draws.
    __syncthreads();
    if (threadIdx.x == 0) {
      const int G = (int)gridDim.x;
      const int nsub = G < OPT_TICKET_SUBS ? G : OPT_TICKET_SUBS;
      const int sub = (int)blockIdx.x % OPT_TICKET_SUBS;
      const int quota = (G - sub + OPT_TICKET_SUBS - 1) / OPT_TICKET_SUBS;
      int32_t* sc = a.ticket + OPT_TICKET_LINE * (1 + sub);
      if (atomicAdd(sc, 1) == quota - 1) {
        *sc = 0;
        if (atomicAdd(a.ticket, 1) == nsub - 1) {
          *a.step_dev = step;
          *a.ticket = 0;
        }
      }
    }
  }
}

// the probe: out[i] = the rate of step steps[i], by the function the kernel above calls
__global__ __launch_bounds__(256) void lr_schedule_eval_kernel(float lr, SchedArgs sc, const int32_t* __restrict__ steps,
                                                               float* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = lr_scheduled(lr, sc, steps[i]);
}

// the *_ema entries: a 16-byte aligned EMA buffer (like p) and a decay in [0, 1] (NaN fails the comparisons too)
bool ema_args_ok(const float* ema, float ema_decay) {
  return ema && ib_aligned(ema, 16) && ema_decay >= 0.f && ema_decay <= 1.f;
}

// the *_sched entries and the probe: kind 0..2, warmup >= 0, a decay needs total > warmup, min_ratio in [0, 1] (NaN fails too)
bool sched_args_ok(int kind, int32_t warmup, int32_t total, float min_ratio) {
  if (kind < IB_SCHED_CONSTANT || kind > IB_SCHED_COSINE || warmup < 0) return false;
  if (kind != IB_SCHED_CONSTANT && total <= warmup) return false;
  return min_ratio >= 0.f && min_ratio <= 1.f;
}

// the *_decay entries: weight_decay >= 0 (NaN fails the comparison), a table of table_n >= 0 ranges (8-byte aligned int64
// pairs; may be null only when empty), the launch's origin a quad boundary of the flat buffer
bool decay_args_ok(float wd, const void* table, int table_n, int64_t origin) {
  if (!(wd >= 0.f) || table_n < 0 || (table_n > 0 && !table) || !ib_aligned(table, 8)) return false;
  return origin >= 0 && origin % 4 == 0;
}

// The optional features of one launch, checked: what the entries hand to optim_launch.  The *_sched entries always pass their
// SchedArgs.  The *_decay entries drop what does nothing: no SchedArgs for a constant schedule without warmup (the rate is the
// host's lr, as in the entries without a schedule), no DecayArgs where nothing can be decayed (the kernels without decay, bit
// for bit).  The gradnorm entry passes both, with an empty table at weight_decay = 0 (decay_factor(lr, 0) = 1 would be a
// multiply by one all the same).  ok: the arguments passed their checks (an EMA buffer may be absent here).
enum class OptEntry { sched, decay, gradnorm };
struct OptFeatures {
  SchedArgs sc; DecayArgs dk;
  bool ok, has_sc, has_dk;
  OptFeatures(OptEntry e, const float* ema, float ema_decay, int kind, int32_t warmup, int32_t total, float min_ratio,
              float wd = 0.f, const void* table = nullptr, int table_n = 0, int64_t origin = 0)
      : sc{kind, warmup, total, min_ratio},
        dk{wd, e == OptEntry::gradnorm && !(wd > 0.f) ? 0 : table_n, reinterpret_cast<const int64_t*>(table), origin},
        ok(sched_args_ok(kind, warmup, total, min_ratio) && (!ema || ema_args_ok(ema, ema_decay)) &&
           decay_args_ok(wd, table, table_n, origin)),
        has_sc(e != OptEntry::decay || !(kind == IB_SCHED_CONSTANT && warmup == 0)),
        has_dk(e == OptEntry::gradnorm || (e == OptEntry::decay && wd > 0.f && table_n > 0)) {}
  const SchedArgs* sched() const { return has_sc ? &sc : nullptr; }
  const DecayArgs* decay() const { return has_dk ? &dk : nullptr; }
};

// The one place that names kernel instantiations: optim_kernel<SRC, EMA> with the pack (sc, dk, clip) that is present, the EMA
// form where a.ema is.  A clip comes with both others and without sources.
template <bool SRC, typename... F>
void optim_launch_pack(dim3 grid, ib_stream_t stream, const OptArgs& a, const OptSources& S, int main_blocks, const F&... f) {
  if (a.ema)
    hipLaunchKernelGGL((optim_kernel<SRC, true, F...>), grid, dim3(256), 0, ib_s(stream), a, S, main_blocks, f...);
  else
    hipLaunchKernelGGL((optim_kernel<SRC, false, F...>), grid, dim3(256), 0, ib_s(stream), a, S, main_blocks, f...);
}

template <bool SRC>
void optim_launch(dim3 grid, ib_stream_t stream, const OptArgs& a, const OptSources& S, int main_blocks, const SchedArgs* sc,
                  const DecayArgs* dk, const ClipArgs* clip) {
  if constexpr (!SRC)
    if (clip) return optim_launch_pack<SRC>(grid, stream, a, S, main_blocks, *sc, *dk, *clip);
  if (sc && dk) optim_launch_pack<SRC>(grid, stream, a, S, main_blocks, *sc, *dk);
  else if (sc) optim_launch_pack<SRC>(grid, stream, a, S, main_blocks, *sc);
  else if (dk) optim_launch_pack<SRC>(grid, stream, a, S, main_blocks, *dk);
  else optim_launch_pack<SRC>(grid, stream, a, S, main_blocks);
}

// the arguments every entry starts with, in the entries' order, as the kernel's OptArgs (unchecked: optim_check)
OptArgs opt_args(int opt, float* p, const float* g, float* s1, float* s2, int64_t n, float lr, float grad_scale, int32_t step,
                 int32_t* step_dev, int32_t* ticket, void* shadow_bf16, float* ema = nullptr, float ema_decay = 0.f,
                 int ema_warmup = 0) {
  return OptArgs{p, g, s1, s2, reinterpret_cast<bf16_t*>(shadow_bf16), n, lr, grad_scale, step, step_dev, ticket, opt,
                 ema, ema_decay, ema_warmup};
}

// The checks every optimizer entry shares, on the arguments as the entry got them; s1 / s2 the optimizer does not use are
// dropped.  quads_only (the sources form): n % 4 != 0 is IB_E_UNSUPPORTED, behind the checks on p, g, n, opt and the ticket
// and in front of those on the states and the alignment.
int optim_check(OptArgs& a, bool quads_only) {
  if (!a.p || !a.g || a.n <= 0 || a.opt < IB_OPT_SGD || a.opt > IB_OPT_ADAMAX) return IB_E_ARG;
  if (a.ticket && !a.step_dev) return IB_E_ARG;
  if (quads_only && a.n % 4 != 0) return IB_E_UNSUPPORTED;
  const bool need1 = a.opt != IB_OPT_SGD;
  const bool need2 = (a.opt == IB_OPT_ADAM || a.opt == IB_OPT_ADADELTA || a.opt == IB_OPT_ADAMAX);
  if ((need1 && !a.s1) || (need2 && !a.s2)) return IB_E_ARG;
  if (!ib_al16({a.p, a.g, a.s1, a.s2, a.ema}) || !ib_aligned(a.shadow, 8)) return IB_E_ARG;
  if (!need1) a.s1 = nullptr;
  if (!need2) a.s2 = nullptr;
  return IB_OK;
}

// the two launchers behind the C entries: ema == NULL launches optim_kernel<SRC, false>, the kernel without the EMA
int optim_plain(OptArgs a, const SchedArgs* sc, const DecayArgs* dk, const ClipArgs* clip, ib_stream_t stream) {
  if (const int rc = optim_check(a, false)) return rc;
  optim_launch<false>(dim3(ib_grid_1d(a.n / 4 + 1, 256)), stream, a, OptSources{}, 0, sc, dk, clip);
  IB_CHECK_LAUNCH();
  return IB_OK;
}

int optim_sources(OptArgs a, int nsrc, const int64_t* start, const int64_t* len, const int32_t* kind, const void* const* base,
                  const int64_t* stride, const int32_t* count, const float* scale, const float* loss_col, int64_t loss_ld,
                  int64_t loss_rows, float loss_scale, float* loss_out, const SchedArgs* sc, const DecayArgs* dk,
                  ib_stream_t stream) {
  // a bad source list is IB_E_ARG whatever n % 4 is: in front of optim_check's IB_E_UNSUPPORTED
  if (nsrc < 0 || nsrc > OPT_MAXSRC || (nsrc > 0 && (!start || !len || !kind || !base || !stride || !count))) return IB_E_ARG;
  if (const int rc = optim_check(a, true)) return rc;
  const int64_t n = a.n;
  OptSources S{};
  S.n = nsrc;
  for (int j = 0; j < nsrc; ++j) {
    if (start[j] < 0 || len[j] <= 0 || start[j] % 4 != 0 || start[j] + len[j] > n) return IB_E_ARG;
    if (kind[j] == 3) {                                     // skipped by every block
      if (len[j] % 4 != 0) return IB_E_ARG;
      S.s[j] = GradSrc{start[j], len[j], nullptr, 0, 0, 3, 1.f};
      continue;
    }
    if (!base[j] || count[j] <= 0) return IB_E_ARG;
    if (kind[j] == 1) {
      if (len[j] % 4 != 0 || stride[j] % 4 != 0 || !ib_aligned(base[j], 16)) return IB_E_ARG;
    } else if (kind[j] == 2) {
      if (stride[j] % 4 != 0 || !ib_aligned(base[j], 16)) return IB_E_ARG;
    } else return IB_E_ARG;
    S.s[j] = GradSrc{start[j], len[j], reinterpret_cast<const float*>(base[j]), stride[j], count[j], kind[j],
                     scale ? scale[j] : 1.f};
  }
  if (loss_out) {
    if (!loss_col || loss_rows <= 0) return IB_E_ARG;
    S.loss_col = loss_col; S.loss_ld = loss_ld; S.loss_rows = (int)loss_rows; S.loss_scale = loss_scale; S.loss_out = loss_out;
  }
  const int main_blocks = ib_grid_1d(n / 4 + 1, 256);
  int cs_blocks = 0;
  for (int j = 0; j < nsrc; ++j)
    if (kind[j] == 2) cs_blocks += (int)((len[j] + 63) / 64);
  optim_launch<true>(dim3(main_blocks + cs_blocks), stream, a, S, main_blocks, sc, dk, nullptr);
  IB_CHECK_LAUNCH();
  return IB_OK;
}

// the entries of ib_hip_gradnorm.h: every pointer present and 16-byte aligned, max_norm > 0 (NaN fails the comparison)
bool gradnorm_args_ok(std::initializer_list<const void*> ptrs, int64_t n, float max_norm) {
  for (const void* q : ptrs)
    if (!q) return false;
  return ib_al16(ptrs) && n > 0 && max_norm > 0.f;
}

}  // namespace

extern "C" size_t ib_grad_sumsq_workspace(int64_t n) { return n <= 0 ? 0 : (size_t)gn_slots(n) * sizeof(double); }

extern "C" int ib_grad_sumsq(const float* g, int64_t n, double* slots, ib_stream_t stream) {
  if (!gradnorm_args_ok({g, slots}, n, 1.f)) return IB_E_ARG;
  const int G = gn_slots(n);
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(G), dim3(256), 0, ib_s(stream), g, n, gn_slot_len(n, G), slots);
  IB_CHECK_LAUNCH();
  return IB_OK;
}

extern "C" int ib_grad_norm_eval(const double* slots, int64_t n, float grad_scale, float max_norm, double* total_out,
                                 float* stats3, ib_stream_t stream) {
  if (!gradnorm_args_ok({slots, total_out, stats3}, n, max_norm)) return IB_E_ARG;
  hipLaunchKernelGGL(grad_norm_eval_kernel, dim3(1), dim3(256), 0, ib_s(stream), slots, gn_slots(n), grad_scale, max_norm,
                     total_out, stats3);
  IB_CHECK_LAUNCH();
  return IB_OK;
}

extern "C" int ib_optim_step_gradnorm(int opt, float* p, const float* g, float* s1, float* s2, int64_t n, float lr,
                                      float grad_scale, int32_t step, int32_t* step_dev, int32_t* ticket, void* shadow_bf16,
                                      float* ema, float ema_decay, int ema_warmup, int sched_kind, int32_t sched_warmup,
                                      int32_t sched_total, float sched_min_ratio, float weight_decay, const void* table_dev,
                                      int table_n, int64_t origin, const double* slots, int64_t sumsq_n, float max_norm,
                                      float* stats3, ib_stream_t stream) {
  const OptFeatures F(OptEntry::gradnorm, ema, ema_decay, sched_kind, sched_warmup, sched_total, sched_min_ratio, weight_decay,
                      table_dev, table_n, origin);
  if (!F.ok || !gradnorm_args_ok({slots, stats3}, sumsq_n, max_norm)) return IB_E_ARG;
  const ClipArgs c{slots, gn_slots(sumsq_n), max_norm, stats3};
  return optim_plain(opt_args(opt, p, g, s1, s2, n, lr, grad_scale, step, step_dev, ticket, shadow_bf16, ema, ema_decay, ema_warmup),
                     F.sched(), F.decay(), &c, stream);
}

extern "C" int ib_optim_ticket_words(void) { return OPT_TICKET_LINE * (1 + OPT_TICKET_SUBS); }

extern "C" int ib_optim_step(int opt, float* p, const float* g, float* s1, float* s2, int64_t n, float lr,
                             float grad_scale, int32_t step, int32_t* step_dev, int32_t* ticket, void* shadow_bf16,
                             ib_stream_t stream) {
  return optim_plain(opt_args(opt, p, g, s1, s2, n, lr, grad_scale, step, step_dev, ticket, shadow_bf16), nullptr, nullptr,
                     nullptr, stream);
}

extern "C" int ib_optim_step_ema(int opt, float* p, const float* g, float* s1, float* s2, int64_t n, float lr,
                                 float grad_scale, int32_t step, int32_t* step_dev, int32_t* ticket, void* shadow_bf16,
                                 float* ema, float ema_decay, int ema_warmup, ib_stream_t stream) {
  if (!ema_args_ok(ema, ema_decay)) return IB_E_ARG;
  return optim_plain(opt_args(opt, p, g, s1, s2, n, lr, grad_scale, step, step_dev, ticket, shadow_bf16, ema, ema_decay, ema_warmup),
                     nullptr, nullptr, nullptr, stream);
}

extern "C" int ib_optim_step_sources(int opt, float* p, const float* g, float* s1, float* s2, int64_t n, float lr,
                                     float grad_scale, int32_t step, int32_t* step_dev, int32_t* ticket,
                                     void* shadow_bf16, int nsrc, const int64_t* start, const int64_t* len,
                                     const int32_t* kind, const void* const* base, const int64_t* stride,
                                     const int32_t* count, const float* scale, const float* loss_col, int64_t loss_ld,
                                     int64_t loss_rows, float loss_scale, float* loss_out, ib_stream_t stream) {
  return optim_sources(opt_args(opt, p, g, s1, s2, n, lr, grad_scale, step, step_dev, ticket, shadow_bf16), nsrc, start, len, kind,
                       base, stride, count, scale, loss_col, loss_ld, loss_rows, loss_scale, loss_out, nullptr, nullptr, stream);
}

extern "C" int ib_optim_step_sources_ema(int opt, float* p, const float* g, float* s1, float* s2, int64_t n, float lr,
                                         float grad_scale, int32_t step, int32_t* step_dev, int32_t* ticket,
                                         void* shadow_bf16, int nsrc, const int64_t* start, const int64_t* len,
                                         const int32_t* kind, const void* const* base, const int64_t* stride,
                                         const int32_t* count, const float* scale, const float* loss_col,
                                         int64_t loss_ld, int64_t loss_rows, float loss_scale, float* loss_out,
                                         float* ema, float ema_decay, int ema_warmup, ib_stream_t stream) {
  if (!ema_args_ok(ema, ema_decay)) return IB_E_ARG;
  return optim_sources(opt_args(opt, p, g, s1, s2, n, lr, grad_scale, step, step_dev, ticket, shadow_bf16, ema, ema_decay, ema_warmup),
                       nsrc, start, len, kind, base, stride, count, scale, loss_col, loss_ld, loss_rows, loss_scale, loss_out,
                       nullptr, nullptr, stream);
}

extern "C" int ib_optim_step_sched(int opt, float* p, const float* g, float* s1, float* s2, int64_t n, float lr,
                                   float grad_scale, int32_t step, int32_t* step_dev, int32_t* ticket, void* shadow_bf16,
                                   float* ema, float ema_decay, int ema_warmup, int sched_kind, int32_t sched_warmup,
                                   int32_t sched_total, float sched_min_ratio, ib_stream_t stream) {
  const OptFeatures F(OptEntry::sched, ema, ema_decay, sched_kind, sched_warmup, sched_total, sched_min_ratio);
  if (!F.ok) return IB_E_ARG;
  return optim_plain(opt_args(opt, p, g, s1, s2, n, lr, grad_scale, step, step_dev, ticket, shadow_bf16, ema, ema_decay, ema_warmup),
                     F.sched(), F.decay(), nullptr, stream);
}

extern "C" int ib_optim_step_sources_sched(int opt, float* p, const float* g, float* s1, float* s2, int64_t n, float lr,
                                           float grad_scale, int32_t step, int32_t* step_dev, int32_t* ticket,
                                           void* shadow_bf16, int nsrc, const int64_t* start, const int64_t* len,
                                           const int32_t* kind, const void* const* base, const int64_t* stride,
                                           const int32_t* count, const float* scale, const float* loss_col,
                                           int64_t loss_ld, int64_t loss_rows, float loss_scale, float* loss_out,
                                           float* ema, float ema_decay, int ema_warmup, int sched_kind,
                                           int32_t sched_warmup, int32_t sched_total, float sched_min_ratio,
                                           ib_stream_t stream) {
  const OptFeatures F(OptEntry::sched, ema, ema_decay, sched_kind, sched_warmup, sched_total, sched_min_ratio);
  if (!F.ok) return IB_E_ARG;
  return optim_sources(opt_args(opt, p, g, s1, s2, n, lr, grad_scale, step, step_dev, ticket, shadow_bf16, ema, ema_decay, ema_warmup),
                       nsrc, start, len, kind, base, stride, count, scale, loss_col, loss_ld, loss_rows, loss_scale, loss_out,
                       F.sched(), F.decay(), stream);
}

extern "C" int ib_lr_schedule_eval(float lr, int kind, int32_t warmup, int32_t total, float min_ratio, const int32_t* steps,
                                   float* out, int64_t n, ib_stream_t stream) {
  if (!sched_args_ok(kind, warmup, total, min_ratio) || !steps || !out || n <= 0) return IB_E_ARG;
  const SchedArgs sc{kind, warmup, total, min_ratio};
  hipLaunchKernelGGL(lr_schedule_eval_kernel, dim3(ib_grid_1d(n, 256)), dim3(256), 0, ib_s(stream), lr, sc, steps, out, n);
  IB_CHECK_LAUNCH();
  return IB_OK;
}

extern "C" size_t ib_decay_table_bytes(int n) { return n < 0 ? 0 : (size_t)(n > 0 ? n : 1) * 2 * sizeof(int64_t); }

extern "C" int ib_decay_table_build(const int64_t* start, const int64_t* len, int n, void* table_dev, ib_stream_t stream) {
  if (n < 0 || !table_dev || !ib_aligned(table_dev, 16) || (n > 0 && (!start || !len))) return IB_E_ARG;
  std::vector<int64_t> t(2 * (size_t)n);
  int64_t prev_end = 0;
  for (int j = 0; j < n; ++j) {
    if (start[j] < 0 || start[j] % 4 != 0 || len[j] <= 0 || len[j] > INT64_MAX - 3 - start[j]) return IB_E_ARG;
    if (start[j] < prev_end) return IB_E_ARG;                 // unsorted, or inside the range before it
    prev_end = start[j] + (len[j] + 3) / 4 * 4;               // a range covers whole quads
    t[2 * j] = start[j];
    t[2 * j + 1] = prev_end;
  }
  if (n == 0) return IB_OK;
  // the host arrays may go on return: the copy out of this vector is complete before it is destroyed
  if (hipMemcpyAsync(table_dev, t.data(), t.size() * sizeof(int64_t), hipMemcpyHostToDevice, ib_s(stream)) != hipSuccess)
    return IB_E_LAUNCH;
  if (hipStreamSynchronize(ib_s(stream)) != hipSuccess) return IB_E_LAUNCH;
  return IB_OK;
}

extern "C" int ib_optim_step_decay(int opt, float* p, const float* g, float* s1, float* s2, int64_t n, float lr,
                                   float grad_scale, int32_t step, int32_t* step_dev, int32_t* ticket, void* shadow_bf16,
                                   float* ema, float ema_decay, int ema_warmup, int sched_kind, int32_t sched_warmup,
                                   int32_t sched_total, float sched_min_ratio, float weight_decay, const void* table_dev,
                                   int table_n, int64_t origin, ib_stream_t stream) {
  const OptFeatures F(OptEntry::decay, ema, ema_decay, sched_kind, sched_warmup, sched_total, sched_min_ratio, weight_decay,
                      table_dev, table_n, origin);
  if (!F.ok) return IB_E_ARG;
  return optim_plain(opt_args(opt, p, g, s1, s2, n, lr, grad_scale, step, step_dev, ticket, shadow_bf16, ema, ema_decay, ema_warmup),
                     F.sched(), F.decay(), nullptr, stream);
}

extern "C" int ib_optim_step_sources_decay(int opt, float* p, const float* g, float* s1, float* s2, int64_t n, float lr,
                                           float grad_scale, int32_t step, int32_t* step_dev, int32_t* ticket,
                                           void* shadow_bf16, int nsrc, const int64_t* start, const int64_t* len,
                                           const int32_t* kind, const void* const* base, const int64_t* stride,
                                           const int32_t* count, const float* scale, const float* loss_col,
                                           int64_t loss_ld, int64_t loss_rows, float loss_scale, float* loss_out,
                                           float* ema, float ema_decay, int ema_warmup, int sched_kind,
                                           int32_t sched_warmup, int32_t sched_total, float sched_min_ratio,
                                           float weight_decay, const void* table_dev, int table_n, int64_t origin,
                                           ib_stream_t stream) {
  const OptFeatures F(OptEntry::decay, ema, ema_decay, sched_kind, sched_warmup, sched_total, sched_min_ratio, weight_decay,
                      table_dev, table_n, origin);
  if (!F.ok) return IB_E_ARG;
  return optim_sources(opt_args(opt, p, g, s1, s2, n, lr, grad_scale, step, step_dev, ticket, shadow_bf16, ema, ema_decay, ema_warmup),
                       nsrc, start, len, kind, base, stride, count, scale, loss_col, loss_ld, loss_rows, loss_scale, loss_out,
                       F.sched(), F.decay(), stream);
}
