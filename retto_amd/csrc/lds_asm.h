// Inline-asm memory primitives of the LDS-DMA kernels (nn_gemm_dma.hip, nn_gemm_split.hip, nn_f16_dma.hip): the one copy of
// each.  Device code only: include it from a .hip file.
//
// The LDS-DMA request is written as inline asm: with the builtin (__builtin_amdgcn_global_load_lds) in a loop hipcc's
// wait-count pass treats the LDS counter as out of order and emits lgkmcnt(0) before every MFMA group -- which also waits
// for the fragment reads just issued for the NEXT k-step (checked on a reduced kernel: counted lgkmcnt(5/4/1) without the
// DMA or with this form, lgkmcnt(0) everywhere with the builtin).  M0 = wave-uniform LDS byte address; lane i writes
// 16 bytes (blds4: 4) at M0 + 16 i (4 i); the s_nop 0 is the wait state between the SALU write of M0 and the request.  The
// kernels count vmcnt for these requests by hand (vm_wait), and the LDS fragment reads and their lgkmcnt waits are asm for
// the same reason (lds_read16, lgkm_wait).
//
// The hazard guard: every statement whose VMEM instruction reads an SGPR operand (buffer descriptor, scalar offset, scalar
// base) opens with s_nop 4.  hipcc's hazard recogniser does not look into an asm block, and an SGPR written by a VALU
// instruction right in front of it -- v_readlane restoring a spilled scalar, v_readfirstlane, a v_cmp or carry-out into an
// SGPR -- needs 5 wait states before a VMEM instruction reads it; without them the instruction reads stale descriptor words
// and the access faults (round 6).  Whether such a write lands there depends on the register allocation, so
// every statement carries the guard; the one exception is named as such (blds16_unguarded).  glds16 needs none: its only
// scalar operand is read by the SALU s_mov to M0.
// tools/asm_hazard_scan.sh checks the built kernels (tests/test_asm_hazard_cpu.py).
#pragma once

namespace rt {

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"   // M0 is named as clobbered on purpose: nothing else in these kernels uses it

// source = 64-bit per-lane address
__device__ __forceinline__ void glds16(unsigned long long gaddr, unsigned lds_sgpr) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(gaddr), "s"(lds_sgpr) : "memory", "m0");
}
// source = 64-bit scalar base + 32-bit per-lane byte offset
__device__ __forceinline__ void glds16_so(unsigned voff, const void* sbase, unsigned lds_sgpr) {
  asm volatile("s_nop 4\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_sgpr) : "memory", "m0");
}
// source = buffer resource base + per-lane byte offset + scalar offset; a lane whose offset is beyond the resource's range
// (0x80000000 is) writes ZEROS: padding rows / pixels cost no select, and a row / slab advance is one scalar operand
__device__ __forceinline__ void blds16(unsigned voff, __amdgpu_buffer_rsrc_t rs, unsigned lds_sgpr, unsigned soff) {
  asm volatile("s_nop 4\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %3 offen lds" ::"v"(voff), "s"(rs), "s"(lds_sgpr), "s"(soff) : "memory", "m0");
}
// blds16 WITHOUT the guard, for the two kernels where the s_nop 4 measured slower than the run-to-run spread (rocprofv3 mean
// launch times, two runs each, unguarded -> guarded: k_conv16v2 on C5 703 / 707 -> 738 / 761 us, k_gemm32p on C3 633 / 704 ->
// 740 / 779 us).  Safe only while no VALU instruction writes one of its SGPR operands fewer than 5 wait states before it:
// tests/test_asm_hazard_cpu.py scans every VMEM instruction of the built library, these included.
__device__ __forceinline__ void blds16_unguarded(unsigned voff, __amdgpu_buffer_rsrc_t rs, unsigned lds_sgpr, unsigned soff) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %3 offen lds" ::"v"(voff), "s"(rs), "s"(lds_sgpr), "s"(soff) : "memory", "m0");
}
// blds16, one dword per lane, no scalar offset
__device__ __forceinline__ void blds4(unsigned voff, __amdgpu_buffer_rsrc_t rs, unsigned lds_sgpr) {
  asm volatile("s_nop 4\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dword %0, %1, 0 offen lds" ::"v"(voff), "s"(rs), "s"(lds_sgpr) : "memory", "m0");
}

#pragma clang diagnostic pop

// The tile queue: one returning global_atomic_add of 1 on *counter; the counter's old value.  (Through the builtin hipcc waits
// vmcnt(0) right behind the atomic, i.e. also for every LDS-DMA request in flight.)  Its return is counted by the caller's vmcnt.
__device__ __forceinline__ unsigned tile_queue_fetch(unsigned* counter) {
  unsigned old;
  asm volatile("s_nop 4\n\tglobal_atomic_add %0, %1, %2, %3 sc0" : "=v"(old) : "v"(0u), "v"(1u), "s"(counter) : "memory");
  return old;
}

__device__ __forceinline__ unsigned lds_addr(const void* p) { return (unsigned)(size_t)(__attribute__((address_space(3))) const char*)p; }

// ds_read_b128 at a byte address + compile-time offset, as any 16-byte vector type (h8, f32x4, u32x4).  Inside loops whose body
// holds branches hipcc falls back to lgkmcnt(0) before each MFMA group even for plain LDS reads, which waits for the prefetch
// issued just before; as asm the reads are invisible to its wait-count pass and lgkm_wait counts them.
template <typename T, int OFF = 0>
__device__ __forceinline__ T lds_read16(unsigned byte_addr) {
  static_assert(sizeof(T) == 16, "ds_read_b128 returns 16 bytes");
  static_assert(OFF >= 0 && OFF < 65536, "16-bit offset field");
  T v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(byte_addr), "n"(OFF));
  return v;
}

// Leaves the newest N LDS operations in flight and pins the order around the wait (sched_barrier: an MFMA has no memory
// operand, so a "memory" clobber alone does not keep it behind the wait).
template <int N>
__device__ __forceinline__ void lgkm_wait() {
  static_assert(N >= 0 && N <= 15, "lgkmcnt is a 4-bit counter");
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// Leaves the newest N vector-memory operations of the wave in flight.
template <int N>
__device__ __forceinline__ void vm_wait() {
  static_assert(N >= 0 && N <= 63, "vmcnt is a 6-bit counter");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// ... n at run time, 0 <= n <= MAX (the instruction takes an immediate: a chain of compares, which hipcc turns into a switch);
// a larger n waits as for MAX, i.e. for more than it must
template <int MAX, int N = 0>
__device__ __forceinline__ void vm_wait(int n) {
  static_assert(MAX >= 0 && MAX <= 63, "vmcnt is a 6-bit counter");
  if constexpr (N == MAX) vm_wait<MAX>();
  else if (n == N) vm_wait<N>();
  else vm_wait<MAX, N + 1>(n);
}

__device__ __forceinline__ int lane_id() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

}  // namespace rt
