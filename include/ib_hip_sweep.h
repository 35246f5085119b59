/* The image sweep of the whole-layer training launches (csrc/ffn_chain.hip, csrc/ffn_chain_bwd.hip; the rule itself in
 * csrc/image_sweep.h): at kernel start every workgroup requests its own 1 / grid slice of the packed weight parts its form will
 * stream, with 16-byte loads whose values are dropped, so that the layer's image -- read once per step, in HBM at every launch --
 * is on its way on chip before the GEMM phases walk it k-block by k-block.  The sweep only loads: every output is bitwise what it
 * is without it, and no entry of the step's C-ABI has another argument for it.
 * The twelfth header of the C-ABI of libib_hip.so.  Conventions as in ib_hip.h (a negative IB_E_* code on error).  It is a header
 * of its own so that the other eleven and what is pinned to them stay as they are.  The binding parses it with the parser of
 * ib_hip.h.  Its one entry is a pure host query: the slice rule exactly as the kernels apply it, for the test that checks every
 * slice against its part's bounds without a launch. */
#ifndef IB_HIP_SWEEP_H
#define IB_HIP_SWEEP_H

#include "ib_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The slices workgroup `wg` of a launch of `grid` workgroups sweeps, for one form of the kernels:
 *   backward == 0: ffn_chain_fwd_kernel<out, qkv, att>, parts in the order wop, w1p, w2p, wqkvp, (none)
 *   backward != 0: ffn_chain_bwd_kernel<out, qkv (the QKV head), att>, parts in the order wqkvtp, w2tp, w1tp, wotp, wqkvtp_own
 * at model width d and hidden width ffn (ib_ffn_chain_supported).  Three arrays of FIVE int64 come back, in that order:
 * part_bytes[k] = the size of part k (0: the form does not stream it), off[k] / len[k] = the workgroup's slice of it in bytes
 * from the part's start (len 0: none).  The parts laid end to end, workgroup wg takes bytes [wg q, (wg + 1) q) of the line,
 * q = min(24576, total / grid rounded up to 16): three 16-byte loads per thread of 512 at the most, so a small grid sweeps a
 * prefix of the image and a grid of 256 or more all 6 MB of a layer of ffn = 2048.
 * Returns the workgroup's byte count (the sum of len, >= 0).  A width the kernels do not take -> IB_E_UNSUPPORTED; a form that
 * does not exist (forward: att without qkv, qkv without out; backward: qkv or att without out, both), a null array, grid < 1,
 * wg outside [0, grid) -> IB_E_ARG. */
int ib_image_sweep_slices(int backward, int out, int qkv, int att, int64_t d, int64_t ffn, int grid, int wg,
                          int64_t* part_bytes, int64_t* off, int64_t* len);

#ifdef __cplusplus
}
#endif
#endif /* IB_HIP_SWEEP_H */
