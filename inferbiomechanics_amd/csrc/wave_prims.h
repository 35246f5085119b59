// Wave-level and LDS primitives of the hand-scheduled gfx950 kernels: the address-space types, the inline-asm LDS accesses
// and the counted waits around them.  One definition each; a kernel file includes this header instead of copying from its
// neighbour.  A slip in one of these is not a compile error but a spill or a race: an operand missing from
// frags_ready's list lets a consumer be scheduled above the wait.
//
// Why the LDS accesses are inline asm: hipcc orders every LDS access it can see behind ALL outstanding LDS-DMA writes
// (s_waitcnt vmcnt(0) before the first ds_read of a K step), which would drain the stages in flight.  Accesses it cannot
// see are ordered by hand: a counted wait_vm + barrier above them, one frags_ready below them.
#pragma once
#include "ib_common.h"

namespace {

typedef __attribute__((address_space(3))) void lds_void_t;             // operands of __builtin_amdgcn_global_load_lds
typedef __attribute__((address_space(1))) const void glb_void_t;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2_t;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;
typedef __attribute__((address_space(3))) s16x4_t lds_s16x4_t;         // operand of the ds_read_tr16_b64 builtin
typedef __attribute__((ext_vector_type(8))) short s16x8_t;

// byte offset of an LDS object inside the workgroup's allocation (what the ds_* instructions address)
__device__ __forceinline__ unsigned lds_off(const void* p) {
  return (unsigned)(size_t)(__attribute__((address_space(3))) const void*)p;
}

// lane id recomputed where it is needed (2 VALU): values derived from a cached threadIdx.x were spilled, and a spill
// reload is a VMEM operation -- retired in order, it stalls on the weight prefetch issued just before it, and its
// s_waitcnt vmcnt(0) drains the LDS-DMA stages in flight
__device__ __forceinline__ int lane_now() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}

// all LDS reads issued so far have landed.  The fragments are the asm's in/out operands, so no consumer can be scheduled
// above the wait: one fragment quad, or a pair of sets of N = 2, 4 or 8 fragments (ONE wait whatever the count)
__device__ __forceinline__ void frags_ready(bf16x8_t (&f)[4]) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]));
}
template <int N>
__device__ __forceinline__ void frags_ready(bf16x8_t (&a)[N], bf16x8_t (&b)[N]) {
  static_assert(N == 2 || N == 4 || N == 8, "one asm statement per operand count");
  if constexpr (N == 2)
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a[0]), "+v"(a[1]), "+v"(b[0]), "+v"(b[1]));
  else if constexpr (N == 4)
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]));
  else
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]),
                   "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]), "+v"(b[4]), "+v"(b[5]), "+v"(b[6]), "+v"(b[7]));
}
// at most N of this wave's vector-memory operations (LDS-DMA pieces, loads, stores) are still in flight
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// this wave's LDS writes are done (before the barrier that publishes them)
__device__ __forceinline__ void lds_drain() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

template <int OFF>
__device__ __forceinline__ bf16x8_t lds_read16(unsigned addr) {
  u32x4_t v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
  return __builtin_bit_cast(bf16x8_t, v);
}
template <int OFF>
__device__ __forceinline__ void lds_write8(unsigned addr, u32x2_t v) {
  asm volatile("ds_write_b64 %0, %1 offset:%2" ::"v"(addr), "v"(v), "n"(OFF) : "memory");
}

// One MFMA fragment of a [k][row] image, transposed by the LDS: lane 4q + p of a 16-lane group addresses image row q,
// columns 4p .. 4p+3, and receives column (lane % 16) of the group's 4 rows.  Two reads: rows m .. m+3 (lo) and
// m+4 .. m+7 (hi).  The asm form takes the lane's byte address and the two halves' constant offsets ...
template <int OFF_LO, int OFF_HI>
__device__ __forceinline__ bf16x8_t lds_read_tr(unsigned addr) {
  u32x2_t lo, hi;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(lo) : "v"(addr), "n"(OFF_LO));
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(hi) : "v"(addr), "n"(OFF_HI));
  u32x4_t v;
  v[0] = lo[0]; v[1] = lo[1]; v[2] = hi[0]; v[3] = hi[1];
  return __builtin_bit_cast(bf16x8_t, v);
}
// ... the builtin form (kernels without LDS-DMA in flight: the compiler may see and schedule the reads) the two halves'
// addresses
__device__ __forceinline__ bf16x8_t lds_read_tr16(const void* a0, const void* a1) {
  s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(a0));
  s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(a1));
  s16x8_t v;
  v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3];
  v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
  return __builtin_bit_cast(bf16x8_t, v);
}

}  // namespace
