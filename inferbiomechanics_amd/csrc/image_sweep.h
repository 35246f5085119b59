// The image sweep of the whole-layer training kernels (ffn_chain.hip, ffn_chain_bwd.hip): at kernel start every workgroup
// requests its own 1 / gridDim slice of the packed weight parts its form will stream, with 16-byte loads whose values are
// dropped.  A layer's image is read once per step and meets every launch in HBM; without the sweep the 32 workgroups of an
// XCD walk it in lockstep and pay one HBM miss per k-block in sequence.  The sweep only loads: no result depends on it.
//
// The slice rule below is the ONE place that maps (part sizes, grid, workgroup) to (offset, length) per part; the kernels
// call it on the device and include/ib_hip_sweep.h exposes it on the host (ib_image_sweep_slices), where
// tests/test_image_sweep_cpu.py checks alignment, bounds and disjointness exhaustively.
#pragma once
#include <stdint.h>

constexpr int IB_SWEEP_PARTS = 5;                         // most parts a form streams (backward: five pointers)
constexpr int IB_SWEEP_LOADS = 3;                         // 16-byte loads per thread ...
constexpr int IB_SWEEP_CAP = IB_SWEEP_LOADS * 512 * 16;   // ... of 512 threads: bytes per workgroup (6 MB over 256 workgroups)

// The parts are laid end to end in the order the kernel consumes them (part[k] bytes each, a multiple of 16; 0 = absent).
// Workgroup wg of `grid` takes bytes [wg q, (wg + 1) q) of that line, q = min(IB_SWEEP_CAP, total / grid rounded up to 16):
// slices are 16-byte aligned, inside their part, disjoint between workgroups, and their union is a prefix of the line -- all of
// it once grid * IB_SWEEP_CAP >= total.  off[k] / len[k] = the piece of part k (len 0: none, off 0); returns the sum of len.
__host__ __device__ inline int ib_sweep_slices(const int (&part)[IB_SWEEP_PARTS], int grid, int wg, int (&off)[IB_SWEEP_PARTS],
                                               int (&len)[IB_SWEEP_PARTS]) {
  int total = 0;
#pragma unroll
  for (int k = 0; k < IB_SWEEP_PARTS; ++k) total += part[k];
  int q = ((total + grid - 1) / grid + 15) & ~15;
  if (q > IB_SWEEP_CAP) q = IB_SWEEP_CAP;
  const int64_t lo64 = (int64_t)wg * q;
  const int lo = lo64 < total ? (int)lo64 : total;
  const int hi = lo64 + q < total ? (int)(lo64 + q) : total;
  int base = 0, bytes = 0;
#pragma unroll
  for (int k = 0; k < IB_SWEEP_PARTS; ++k) {
    const int a = lo > base ? lo : base;
    const int b = hi < base + part[k] ? hi : base + part[k];
    len[k] = b > a ? b - a : 0;
    off[k] = b > a ? a - base : 0;
    bytes += len[k];
    base += part[k];
  }
  return bytes;
}
