/* The merged launches at the head of the transformer denoiser's training step: the third header of the C-ABI of
 * libib_hip.so (csrc/chain.hip, csrc/ffn_chain.hip; device bodies shared with the stand-alone kernels in csrc/head_jobs.h).
 * Conventions as in ib_hip.h (device pointers, a negative IB_E_* code on error, the stream last); like ib_hip_stitch.h it is
 * a header of its own so that ib_hip.h and what is pinned to it stay as they are.  The binding parses it with the parser of
 * ib_hip.h.
 *
 * Every job of a merged launch runs the code of its stand-alone entry point as a block range of one grid, so the results
 * are bit-identical to the separate launches; what is saved is kernel boundaries, first-touch latencies and a stream fork. */
#ifndef IB_HIP_HEAD_H
#define IB_HIP_HEAD_H

#include "ib_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Launch A: ib_time_mlp_fwd (arguments and results unchanged) and, each optional (a NULL first pointer = absent), three jobs
 * that depend neither on it nor on each other:
 *   x0 != NULL        ib_q_sample in bf16 with the same t: x_t [B*T, D] at pitch ld_xt, sched_rows = rows of the two tables;
 *   pos != NULL       posproj [pm, pn] (pitch ldc) = A . B, A(m, k) = pos[m sam + k sak], B(k, n) = wp[k sbk + n sbn], all
 *                     bf16, pk < 64 (ib_tiny_matmul's one-thread-per-element form, same batches of 8 and k order);
 *   cast_src != NULL  cast_dst[r][c] = cast_src[r][c] over cast_rows x cast_cols, bf16 (ib_cast2d).
 * With all three absent the call equals ib_time_mlp_fwd.  ib_tr_head_prep_supported: 1 when the time-MLP shape is supported
 * and B is in the range where the merged form pays (the 16-window time kernel, whose 21 KB of LDS lets four blocks of the
 * element-wise jobs share a CU); the entry point itself runs for any B. */
int ib_tr_head_prep_supported(int64_t temb, int64_t hidden, int64_t out, int64_t B);
int ib_tr_head_prep(const float* table, int64_t table_rows, const int64_t* t, const void* w1, int64_t ldw1,
                    const float* b1, const void* w2, int64_t ldw2, const float* b2, void* s, void* zu, void* u,
                    void* e, int64_t ld_e, int64_t B, int64_t temb, int64_t hidden, int64_t out,
                    const void* x0, const void* eps, const float* sqrt_ab, const float* sqrt_1mab, void* x_t,
                    int64_t ld_xt, int64_t T, int64_t D, int64_t sched_rows,
                    const void* pos, int64_t sam, int64_t sak, const void* wp, int64_t sbk, int64_t sbn,
                    void* posproj, int64_t ldc, int64_t pm, int64_t pn, int64_t pk,
                    const void* cast_src, int64_t cast_lds, void* cast_dst, int64_t cast_ldd, int64_t cast_rows,
                    int64_t cast_cols, ib_stream_t stream);

/* Launch B: ib_ffn_chain_pack (first twelve arguments as there) + ib_transpose_multi (ntr <= 16 bf16 pairs, arguments as
 * there) + ncast <= 2 pitched copies (each as ib_cast2d: c_dst[r][c] = c_src[r][c] over c_rows x c_cols, IB_F32 / IB_BF16
 * codes per side) as ONE launch: everything a training step refreshes from the weights the optimizer just moved.  The
 * packing blocks come first (layer 0's images are the first to be read).  More pairs or copies: IB_E_UNSUPPORTED, nothing
 * launched. */
int ib_ffn_chain_pack_ex(const void* const* w1, const int64_t* ld1, const void* const* w2, const int64_t* ld2,
                         const void* const* wo, const int64_t* ldo, const void* const* wqkv, const int64_t* ldq,
                         void* const* packed, int layers, int64_t d, int64_t ffn,
                         int ntr, const void* const* tr_src, const int64_t* tr_lds, void* const* tr_dst,
                         const int64_t* tr_ldd, const int64_t* tr_rows, const int64_t* tr_cols,
                         int ncast, const void* const* c_src, const int64_t* c_lds, const int32_t* c_sdtype,
                         void* const* c_dst, const int64_t* c_ldd, const int32_t* c_ddtype, const int64_t* c_rows,
                         const int64_t* c_cols, ib_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
