// Device primitives shared by the hand-written kernels: LDS-DMA, buffer descriptors, counted waits, workgroup barriers,
// the XCD remap, the 128-B-row swizzle, the 4 x f16 pack, the 16-byte load of an f32 row and the 64-lane butterflies. One definition each, with its
// hazard note; a kernel file keeps only the helpers that encode its own schedule or LDS layout. Everything here is
// __forceinline__: moving a kernel onto one of these must leave its device assembly unchanged (`make isa`).
#pragma once
#include "common.h"

namespace svc {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// four 16-bit operands as one 8-byte store / load
union H4 {
  uint2 u;
  f16 h[4];
};

// ---------------------------------------------------------------------------------------------- buffer descriptors
constexpr uint32_t BUF_CFG = 0x00020000u;  // buffer descriptor dword 3 (raw, 32-bit data format)
// A voffset past every descriptor's range (extents are < 1 GiB, checked on the host, so voffset + soffset cannot wrap):
// the hardware bounds check makes the load, or the LDS-DMA, deliver zeros.
constexpr uint32_t BUF_OOR = 0x7ffffff0u;

// The descriptor as four SGPR dwords (for lds_bdma16_raw) and as the compiler's resource type (for the buffer builtins);
// a non-positive extent gives an empty range, every access to which is out of range.
__device__ __forceinline__ u32x4 buf_desc(const void* base, int64_t bytes) {
  const uint64_t a = (uint64_t)(uintptr_t)base;
  return u32x4{(uint32_t)a, (uint32_t)(a >> 32) & 0xffffu, (uint32_t)(bytes > 0 ? bytes : 0), BUF_CFG};
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* base, int64_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)(bytes > 0 ? bytes : 0), BUF_CFG);
}

// ---------------------------------------------------------------------------------------------------------- LDS-DMA
// 16 B per lane from global memory straight into LDS: lane i's bytes land at lds + 16 i (lds is wave-uniform), so an
// image's swizzle is applied on the SOURCE address. The compiler counts these on vmcnt like loads, but treats one in
// flight as a pending LDS write: __syncthreads() would drain it (vmcnt(0)), so kernels that keep DMAs in flight across
// a barrier use vm_wait<N>() and wg_barrier() below.
__device__ __forceinline__ void lds_dma16(const void* src, unsigned char* lds) {
  __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)lds, 16, 0, 0);
}
// The same through a buffer descriptor: per-lane byte offset voff, wave-uniform byte offset soff, no per-lane 64-bit
// address arithmetic; a voff of BUF_OOR lands zeros (padding rows, tiles past the end).
__device__ __forceinline__ void lds_bdma16(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff,
                                           unsigned char* lds) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)lds, 16, (int)voff, (int)soff,
                                           0, 0);
}
// The same in inline asm. It exists because the compiler does not see it: it neither counts it nor drains it before
// every LDS read it cannot prove disjoint (it did, for reads of other ring slots), so ONLY the caller's hand-counted
// vm_wait<N>() and barriers order it against the reads of its destination. It clobbers m0 (the DMA's LDS base; the
// compiler's own LDS-DMA and indexing uses all set m0 right before use, hence the silenced reserved-register warning),
// and the s_nop 0 is the wait state the hardware needs between writing m0 and the instruction that reads it.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ void lds_bdma16_raw(u32x4 d, uint32_t voff, unsigned char* lds) {
  const uint32_t m0 =
      __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)lds);
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds"
               ::"s"(m0), "v"(voff), "s"(d) : "memory", "m0");
}
#pragma clang diagnostic pop

// ------------------------------------------------------------------------------------------------ waits and barriers
// Wait until at most N of this wave's vector-memory operations are outstanding. Loads, LDS-DMAs (all three forms above)
// and stores count together, in issue order, so N is the number of operations issued after the one to retire. The
// counter has 6 bits.
template <int N>
__device__ __forceinline__ void vm_wait() {
  static_assert(N >= 0 && N < 64, "vmcnt");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// wait for this wave's LDS (and scalar-memory) operations: its ds_writes have landed, its ds_reads have returned
__device__ __forceinline__ void lgkm_wait0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// Workgroup barrier that nothing is scheduled across (the compiler hoists register-only work over a bare s_barrier).
// Unlike __syncthreads() it waits for nothing: LDS-DMAs stay in flight across it, and it does NOT drain this wave's LDS
// writes; a DMA is visible to the other waves after its issuer's vm_wait and then this barrier.
__device__ __forceinline__ void wg_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}
// the same behind this wave's LDS writes (ds_write results the other waves read after the barrier)
__device__ __forceinline__ void wg_barrier_lds() {
  __builtin_amdgcn_sched_barrier(0);
  lgkm_wait0();
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

// ------------------------------------------------------------------------------------------------- placement, layout
// blockIdx.x -> a workgroup index whose consecutive values land on one XCD (blocks are dealt round-robin over the 8
// XCDs), so tiles that share operand rows share that XCD's L2. Bijective for every grid size; speed only.
__device__ __forceinline__ int xcd_remap() {
  const int nwg = gridDim.x, orig = blockIdx.x;
  const int xcd = orig & 7, q8 = nwg >> 3, r8 = nwg & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
}

// 16-B chunk swizzle of LDS images with 128-B rows: logical k-chunk kv of row `row` sits in chunk sw128(row, kv) (an
// involution), which makes the ds_read_b128 fragment reads (16 consecutive rows per lane group) conflict-free for every
// starting row.
__device__ __forceinline__ int sw128(int row, int kv) { return kv ^ (row & 6); }

// ------------------------------------------------------------------------------------- unaligned f32 rows, 16 B at a time
// x[0..3] = row[i0 .. i0 + 4), all four inside [0, n). One 16-byte load where the address is aligned, else the two
// aligned quads that cover the four samples where both lie inside [0, n), else four 4-byte loads.
__device__ __forceinline__ void load4(const float* row, int64_t i0, int64_t n, float* x) {
  const int mis = (int)((reinterpret_cast<uintptr_t>(row + i0) >> 2) & 3);
  if (mis == 0) {
    const float4 p = *reinterpret_cast<const float4*>(row + i0);
    x[0] = p.x, x[1] = p.y, x[2] = p.z, x[3] = p.w;
  } else if (i0 - mis >= 0 && i0 - mis + 8 <= n) {
    const float4* a = reinterpret_cast<const float4*>(row + i0 - mis);
    const float4 p = a[0], q = a[1];
    if (mis == 1) x[0] = p.y, x[1] = p.z, x[2] = p.w, x[3] = q.x;
    else if (mis == 2) x[0] = p.z, x[1] = p.w, x[2] = q.x, x[3] = q.y;
    else x[0] = p.w, x[1] = q.x, x[2] = q.y, x[3] = q.z;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = row[i0 + k];
  }
}

// ---------------------------------------------------------------------------------------------- 64-lane butterflies
// Every lane of the wave gets the result; all 64 lanes must be active. (T: int, float or double. No wave_min: the one
// min butterfly, f0_global_kernel's, runs interleaved with a sum and a max in one loop.)
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
template <typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

}  // namespace svc
