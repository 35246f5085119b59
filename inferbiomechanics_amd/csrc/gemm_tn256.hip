// Weight-gradient GEMM with a 256 (n) x 256 (k) output tile, bf16, gfx950: dW[N,K] = sum_m dz[m][n] * x[m][k] as fp32
// split slabs, for groups of problems whose N and K are multiples of 256 (the transformer denoiser's layers: [1536,512],
// [512,512], [2048,512], [512,2048] at M = 12800 token rows).
//
// Why beside gemm_tn.hip: that kernel's K step is bound by what one CU takes in from L2 (48 KB per 64-deep step = 0.82 us
// at ~60 GB/s per CU, against 0.49 us of MFMA issue).  A 256 x 256 tile takes in 64 KB per 64 reduction rows for TWICE the
// flops: ingest and MFMA time meet (~1.0 us per 64 rows), i.e. ~1.5x the rate per CU.  The second thing it fixes is the
// grouped launch's balance: gemm_tn.hip gives every problem its own split count (2, 8, 2, 2 for a transformer layer), so
// the out-projection's items are 25 K steps long and the others 100, one item per CU -- the launch lasts 100 steps for 75
// steps of work per CU.  Here every problem of the group takes the SAME split count, so all items are equally long.
//
// Layout of a stage (32 reduction rows): A image [32][256 n] and B image [32][256 k], 512-byte rows, filled by
// global_load_lds_dwordx4 (two rows per 1-KiB wave instruction); the sixteen 32-byte column chunks of a row are
// XOR-swizzled with s(m) = (m & 3) | ((m >> 3) & 1) << 2 on the per-lane SOURCE address (LDS-DMA writes lane-linearly), so
// the ds_read_b64_tr_b16 fragment reads are conflict-free (same scheme as gemm_tn.hip).  A ring of four stages of 32 KiB.
// Four waves as 2 (n) x 2 (k): a wave owns 128 n x 128 k = 8 x 8 MFMA 16x16x32 tiles (256 accumulator registers per lane:
// one wave per SIMD, the 512-register budget) and issues eight LDS-DMA instructions per stage (four per operand).
// A step = one stage = 64 MFMAs per wave.  A stage's sixteen fragments are held whole (64 registers); under the step's
// MFMAs the NEXT stage's sixteen are read and the stage four ahead is requested into the slot the current one came from,
// which is free from the step's one barrier on: every wave then holds the stage in registers.  Workgroups are persistent
// (XCD-aware walk over the work items); each item runs its own prologue, steady steps and four draining steps.
// No ragged tiles (the host refuses them): every address is in range by construction.
#include <type_traits>

#include "wave_prims.h"
#include "gemm_families.h"

namespace {

constexpr int TM = 256, TK = 256, BK = 32, THREADS4 = 256;
constexpr int ROW = 512;                              // bytes per image row (256 bf16), both operands
constexpr int OP_BYTES = BK * ROW, STAGE = 2 * OP_BYTES;                              // 16 KiB, 32 KiB
constexpr int MAXP = 6;
#ifndef TN256_ABL
#define TN256_ABL 0      // TIMING-ONLY build variants (tools/build_variant.sh): 1 no MFMA, 2 no LDS-DMA after the prologue, 3 no fragment reads, 4 neither of the last two
#endif

struct Prob {
  const bf16_t* A; const bf16_t* B; int lda, ldb;        // dz [M, N], x [M, K]
  int N, K;
  float* C;                                               // slabs [splits][N][K]
  float* dbias;                                           // optional [splits][N]
  int tiles_k, per_split, item0;                          // K / 256 ; tiles per split ; first work item
};
struct Params {
  Prob pr[MAXP]; int n, items;
  int splits, chunk, nk;             // common to the group: reduction rows per split, stages (of 32 rows) per item
};

// ---------------------------------------------------------------------------------------------------------------------
// Why four waves, not eight (round 5; the eight-wave form, 4 (n) x 2 (k) waves of 64 x 128, is retired: docs/EXPERIMENTS.md):
// eight waves read (64 + 128) x 32 x 2 B = 12 KiB of fragments per wave and stage = 96 KiB per workgroup against 32 KiB
// that the LDS-DMA writes -- 1024 LDS cycles (128 B / clk) per stage next to 1024 MFMA cycles: the two pipes could only
// lose to each other (timing-only ablations: no fragment reads 84 us, no LDS-DMA 86 us, both 102 us).  A 128 x 128 wave
// tile reads 16 KiB per wave = 64 KiB per workgroup and stage: 768 LDS cycles under the same 1024 MFMA cycles.
// A stage's sixteen fragments are held whole (64 registers) and the NEXT stage's sixteen are read under the 64 MFMAs, so
// the stage's slot is free from the barrier at the head of its own step: one barrier per step, at the step boundary.
struct Frags { bf16x8_t a[8], b[8]; };
#ifndef TN256_NS4
#define TN256_NS4 4
#endif
constexpr int NS4 = TN256_NS4;          // ring depth of the four-wave form (5 x 32 KiB = the whole LDS measured the same: 104.9-108.5 vs 106.1-107.9 us)
// accumulators pinned to the AccVGPR half of the wave's 512 registers (left to itself the allocator spreads them over both
// halves and copies: 179 v_accvgpr moves per 128 MFMAs); volatile: issue order = program order
__device__ __forceinline__ void mfma_acc(f32x4_t& acc, const bf16x8_t& a, const bf16x8_t& b) {
  asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b));
}

template <bool BIAS>
__global__ __launch_bounds__(THREADS4, 1) void gemm_tn256w4_kernel(Params P) {
  __shared__ __attribute__((aligned(1024))) unsigned char smem[NS4 * STAGE];
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int wm = wave & 1, wn = wave >> 1;
  const int nwg = (int)gridDim.x;
  const int first = ib_xcd_remap((int)blockIdx.x, nwg);
  if (first >= P.items) return;
  const unsigned smem0 = lds_off(smem);
  const int nk = P.nk;

  unsigned ab0, bb0;
  {
    const int lane = lane_now();
    const int g = lane >> 4, q = (lane & 15) >> 2, pq = lane & 3;
    const unsigned ro = (unsigned)((8 * g + q) * ROW + 8 * pq);
    ab0 = smem0 + ro + (unsigned)(32 * ((wm << 3) | ((g & 1) << 2) | q));
    bb0 = smem0 + OP_BYTES + ro + (unsigned)(32 * ((wn << 3) | ((g & 1) << 2) | q));
  }
  [[maybe_unused]] bf16x8_t ones;
#pragma unroll
  for (int e = 0; e < 8; ++e) ones[e] = (bf16_t)1.0f;

  for (int item = first; item < P.items; item += nwg) {
    int e = 0;
    for (int j = 1; j < P.n; ++j)
      if (item >= P.pr[j].item0) e = j;
    const Prob& q = P.pr[e];
    const int local = item - q.item0;
    const int split = local / q.per_split, tl = local % q.per_split;
    const int i0 = (tl / q.tiles_k) * TM, j0 = (tl % q.tiles_k) * TK;

    // LDS-DMA sources.  A wave's piece j (0..3) of an operand = stage rows r0 + 8 j, r0 = 2 wave + (lane >> 5): the row's
    // swizzle s(m) = (m & 3) | ((m >> 3) & 1) << 2 has its high bit from j's parity, so two per-lane column offsets
    const bf16_t* pa[2];
    const bf16_t* pb[2];
    const unsigned sa = (unsigned)q.lda, sb = (unsigned)q.ldb;
    {
      const int lane = lane_now();
      const int r0 = 2 * wave + (lane >> 5);
#pragma unroll
      for (int par = 0; par < 2; ++par) {
        const int src = (lane & 31) ^ (((r0 & 3) | (par << 2)) << 1);
        pa[par] = q.A + (size_t)(split * P.chunk + r0) * sa + (size_t)(i0 + 8 * src);
        pb[par] = q.B + (size_t)(split * P.chunk + r0) * sb + (size_t)(j0 + 8 * src);
      }
    }
    // piece j (0..3: operand A, 4..7: operand B) of stage kt into the slot at `st`
    auto piece = [&](int j, int kt, unsigned char* st) {
      if (j < 4)
        __builtin_amdgcn_global_load_lds((glb_void_t*)(pa[j & 1] + (size_t)((unsigned)(kt * BK + 8 * j) * sa)),
                                         (lds_void_t*)(st + (wave + 4 * j) * 1024), 16, 0, 0);
      else
        __builtin_amdgcn_global_load_lds((glb_void_t*)(pb[j & 1] + (size_t)((unsigned)(kt * BK + 8 * (j - 4)) * sb)),
                                         (lds_void_t*)(st + OP_BYTES + (wave + 4 * (j - 4)) * 1024), 16, 0, 0);
    };

    [[maybe_unused]] const bool want_bias = BIAS && q.dbias != nullptr && j0 == 0;
    f32x4_t acc[8][8];
    [[maybe_unused]] f32x4_t accb[4];
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[t][u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    if constexpr (BIAS) {
#pragma unroll
      for (int t = 0; t < 4; ++t) accb[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }

    // prologue: NS stages in flight (nk >= 8 by the host's choice of the split), the first one's fragments
#pragma unroll
    for (int s = 0; s < NS4; ++s)
#pragma unroll
      for (int j = 0; j < 8; ++j) piece(j, s, smem + s * STAGE);
    wait_vm<8 * (NS4 - 1)>();
    __builtin_amdgcn_s_barrier();
    Frags f0, f1;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      f0.a[t] = lds_read_tr<0, 4 * ROW>(ab0 ^ (unsigned)(t << 5));
      f0.b[t] = lds_read_tr<0, 4 * ROW>(bb0 ^ (unsigned)(t << 5));
    }
    frags_ready(f0.a, f0.b);

    // step kt: the 64 MFMAs of stage kt (fragments in `cur`); under them the fragments of stage kt + 1 are read into `nxt`
    // (NEXT) and stage kt + NS is requested into the slot stage kt came from (ISSUE).  VM = LDS-DMA instructions that may
    // still be in flight when stage kt + 1 must have landed (the stages issued behind it, 8 per stage; loads retire in order).
    // The order below IS the issue order (MFMAs and fragment reads are volatile asm, scheduling barriers pin the rest): the
    // first row of MFMAs runs ahead of the barrier (it needs neither the freed slot nor the next stage), the sixteen
    // fragment reads and eight requests are spread over the other seven rows.
    int slot = 0;                          // the slot stage kt lies in (kt mod NS4)
    auto step = [&](auto next_c, auto issue_c, auto vm_c, int kt, Frags& cur, Frags& nxt) {
      constexpr bool NEXT = decltype(next_c)::value, ISSUE = decltype(issue_c)::value;
      constexpr int VM = decltype(vm_c)::value;
      const int slot1 = slot == NS4 - 1 ? 0 : slot + 1;
      const unsigned so1 = (unsigned)(slot1 * STAGE);
      unsigned char* st = smem + slot * STAGE;
      auto read_pair = [&](int t) {
        nxt.a[t] = lds_read_tr<0, 4 * ROW>((ab0 + so1) ^ (unsigned)(t << 5));
        nxt.b[t] = lds_read_tr<0, 4 * ROW>((bb0 + so1) ^ (unsigned)(t << 5));
      };
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        if (t == 1 && NEXT) {
          wait_vm<VM>();
          __builtin_amdgcn_s_barrier();    // every wave holds stage kt in registers (slot free) and stage kt + 1 is visible
        }
        if (t >= 1 && NEXT && TN256_ABL != 3 && TN256_ABL != 4) {
          read_pair(t);
          if (t == 1) read_pair(0);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (TN256_ABL != 1) mfma_acc(acc[t][u], cur.b[u], cur.a[t]);
        __builtin_amdgcn_sched_barrier(0);
        if (t >= 1 && ISSUE && TN256_ABL != 2 && TN256_ABL != 4) {
          piece(t, kt + NS4, st);
          if (t == 1) piece(0, kt + NS4, st);
        }
      }
      if constexpr (BIAS) {
        if (want_bias) {                   // item-uniform; the two k-half waves of an n half take four row tiles each
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const bf16x8_t fsel = wn ? cur.a[4 + i] : cur.a[i];
            // (the builtin would take the AccVGPR form and shuttle these four through a[16:19] every step)
            asm volatile("s_nop 1\n\tv_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(accb[i]) : "v"(ones), "v"(fsel));
          }
        }
      }
      if constexpr (NEXT) frags_ready(nxt.a, nxt.b);
      slot = slot1;
    };
    using T_ = std::true_type;
    using F_ = std::false_type;
    auto vm = [](auto c) { return std::integral_constant<int, 8 * decltype(c)::value>{}; };   // stages -> instructions
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    using I3 = std::integral_constant<int, 3>;
    // main steps (a request each) in pairs, then the NS4 steps that only drain the ring; nk is even (host), so with an odd
    // ring the first step stands alone and the fragment buffers swap roles
    auto run = [&](int kt, Frags& x, Frags& y) {
      for (; kt < nk - NS4; kt += 2) {
        step(T_{}, T_{}, vm(std::integral_constant<int, NS4 - 2>{}), kt, x, y);
        step(T_{}, T_{}, vm(std::integral_constant<int, NS4 - 2>{}), kt + 1, y, x);
      }
      if constexpr (NS4 == 4) {
        step(T_{}, F_{}, vm(I2{}), kt, x, y);
        step(T_{}, F_{}, vm(I1{}), kt + 1, y, x);
        step(T_{}, F_{}, vm(I0{}), kt + 2, x, y);
        step(F_{}, F_{}, vm(I0{}), kt + 3, y, x);
      } else {
        static_assert(NS4 == 4 || NS4 == 5, "ring depth");
        step(T_{}, F_{}, vm(I3{}), kt, x, y);
        step(T_{}, F_{}, vm(I2{}), kt + 1, y, x);
        step(T_{}, F_{}, vm(I1{}), kt + 2, x, y);
        step(T_{}, F_{}, vm(I0{}), kt + 3, y, x);
        step(F_{}, F_{}, vm(I0{}), kt + 4, x, y);
      }
    };
    if constexpr (NS4 & 1) {
      step(T_{}, T_{}, vm(std::integral_constant<int, NS4 - 2>{}), 0, f0, f1);
      run(1, f1, f0);
    } else {
      run(0, f0, f1);
    }

    // ---- epilogue: fp32 accumulators straight to the slab of this split
    // (the asm MFMAs are opaque to the compiler's hazard recognizer: the last results need 2 + 4 x 2 passes to land)
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    if constexpr (BIAS) {
      // ALL four registers of each bias accumulator stay live up to here.  Only element 0 is stored, so after the last
      // step's MFMAs the allocator took elements 2-3 of accb[0] as temporaries for the next MFMA's operand while the
      // (opaque) MFMA was still writing them: one or two non-finite bias gradients per ~100 training steps.
      asm volatile("" : "+v"(accb[0]), "+v"(accb[1]), "+v"(accb[2]), "+v"(accb[3]));
    }
    {
      const int lane = lane_now();
      float* slab = q.C + (size_t)split * (size_t)q.N * (size_t)q.K;
      const int n0 = i0 + wm * 128 + (lane & 15), k0 = j0 + wn * 128 + 4 * (lane >> 4);
#pragma unroll
      for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int u = 0; u < 8; ++u)
          *reinterpret_cast<f32x4_t*>(slab + (size_t)(n0 + 16 * t) * q.K + k0 + 16 * u) = acc[t][u];
      if constexpr (BIAS) {
        if (want_bias && (lane >> 4) == 0) {
#pragma unroll
          for (int i = 0; i < 4; ++i) q.dbias[(size_t)split * q.N + n0 + 16 * (4 * wn + i)] = accb[i][0];
        }
      }
    }
    // the next item's prologue reuses all four slots: every read of them is behind the last step's barrier; its 32 requests
    // and these 64 stores do not fit the 6-bit counter together, so the stores drain first (one item per workgroup at the
    // transformer's shapes: this is the kernel's end there)
    wait_vm<0>();
  }
}


}  // namespace

// Common split count of a group of qualifying problems (0: the group does not qualify): the largest divisor s of M / 32
// with s x (total tiles) <= 224 work items (at most one per CU), items at least 8 stages long and an even stage count, s <= 32
// (the bias partial sums have 32 rows).
int ib_gemm_tn256_splits(int n, const int64_t* M, const int64_t* N, const int64_t* K) {
  static const bool off = ib_ab_set("IB_NO_TN256");
  if (off || n <= 0 || n > MAXP) return 0;
  int64_t tiles = 0;
  for (int j = 0; j < n; ++j) {
    if (M[j] != M[0] || M[j] % (2 * BK) != 0 || M[j] < 4096 || N[j] <= 0 || K[j] <= 0 || N[j] % TM != 0 || K[j] % TK != 0) return 0;
    tiles += (N[j] / TM) * (K[j] / TK);
  }
  const int64_t stages = M[0] / BK;
  static const int forced = ib_ab_int("IB_TN256_SPLITS", 0);   // tuning override
  if (forced > 0 && forced <= 32 && stages % forced == 0 && stages / forced >= 8 && !((stages / forced) & 1)) return forced;
  int best = 0;
  for (int64_t s = 1; s <= 32; ++s) {
    if (stages % s != 0) continue;
    const int64_t nk = stages / s;
    if (nk < 8 || (nk & 1)) continue;
    // 224, not 256: the launch runs on a side stream beside the backward's main-stream GEMMs, and every split is one more
    // fp32 slab for the optimizer to read (transformer layer, 48 tiles, same box: 4 splits 2.110-2.116 ms per step, 5 splits
    // 2.126-2.159)
    if (s * tiles <= 224 || best == 0) best = (int)s;      // s = 1 when even that exceeds the chip (several rounds)
  }
  return best;
}

int ib_gemm_tn256_multi(int n, const void* const* dz, const int64_t* lddz, const void* const* x, const int64_t* ldx,
                        void* const* workspace, const size_t* workspace_bytes, float* const* dbias_part, int32_t* nslab_out,
                        const int64_t* M, const int64_t* N, const int64_t* K, hipStream_t s) {
  const int sp = ib_gemm_tn256_splits(n, M, N, K);
  if (sp <= 0) return IB_E_UNSUPPORTED;
  Params P{};
  P.n = n; P.splits = sp; P.chunk = (int)(M[0] / sp); P.nk = P.chunk / BK;
  int items = 0;
  bool any_bias = false;
  for (int j = 0; j < n; ++j) {
    if (!dz[j] || !x[j] || !workspace[j]) return IB_E_ARG;
    if (!ib_al16({dz[j], x[j], workspace[j]}) || lddz[j] % 8 || ldx[j] % 8) return IB_E_UNSUPPORTED;
    if (lddz[j] < N[j] || ldx[j] < K[j]) return IB_E_UNSUPPORTED;
    if (M[j] * lddz[j] >= (int64_t(1) << 31) || M[j] * ldx[j] >= (int64_t(1) << 31)) return IB_E_UNSUPPORTED;
    if ((size_t)sp * (size_t)N[j] * (size_t)K[j] * sizeof(float) > workspace_bytes[j]) return IB_E_UNSUPPORTED;
    Prob& q = P.pr[j];
    q.A = (const bf16_t*)dz[j]; q.B = (const bf16_t*)x[j]; q.lda = (int)lddz[j]; q.ldb = (int)ldx[j];
    q.N = (int)N[j]; q.K = (int)K[j];
    q.C = (float*)workspace[j]; q.dbias = dbias_part ? dbias_part[j] : nullptr;
    any_bias = any_bias || q.dbias != nullptr;
    q.tiles_k = (int)(K[j] / TK); q.per_split = (int)(N[j] / TM) * q.tiles_k;
    q.item0 = items;
    items += q.per_split * sp;
    nslab_out[j] = sp;
  }
  P.items = items;
  const int grid = items < 256 ? items : 256;
  IB_PATH(IB_PATH_TN256);
  if (any_bias) hipLaunchKernelGGL(gemm_tn256w4_kernel<true>, dim3(grid), dim3(THREADS4), 0, s, P);
  else hipLaunchKernelGGL(gemm_tn256w4_kernel<false>, dim3(grid), dim3(THREADS4), 0, s, P);
  IB_CHECK_LAUNCH();
  return IB_OK;
}
