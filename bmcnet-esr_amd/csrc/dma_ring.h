// LDS-DMA, counted vector-memory waits and ring helpers shared by the matrix-core kernels: the only home of LDS-DMA asm.
#pragma once
#include "bmc_common.h"

// Byte address of an LDS object, as the LDS-DMA's m0 and the ds instructions count it.
__device__ __forceinline__ unsigned lds_addr(const void* p) { return (unsigned)(size_t)(__attribute__((address_space(3))) const void*)p; }
// This lane's index, made where it is used (volatile: not a loop invariant the compiler could keep live).  In the kernels
// that have no register to spare, a lane-dependent address kept live across a stage loop is the one value the register
// allocator spills, and its reload -- a scratch load -- waits, in order, for every DMA in flight.
__device__ __forceinline__ int lane_id_pinned() {
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

// 16 bytes per lane from global memory straight into LDS (lane-linear image at the wave-uniform LDS byte address):
// address = uniform base (SGPR pair) + this lane's 32-bit byte offset.  Inline asm on purpose -- the compiler must not
// track these as LDS stores (it would drain vmcnt(0) before every later ds_read and the rings could never run ahead);
// completion is waited for with counted vmcnt (dma_wait) before the barrier that publishes a stage.
// This header is the only place that writes m0, and every write of it is hand-written asm: m0 is reserved and cannot be
// named as a clobber, so mixing these with __builtin_amdgcn_global_load_lds (whose m0 setup the compiler may hoist,
// believing an asm statement leaves m0 alone) would be a latent mis-addressing hazard.  Nothing else in the kernels uses m0.
// dma16_sgpr: base and LDS address are already wave-uniform values the compiler keeps in SGPRs.  NOPS: wait states
// between the VALU-written SGPRs / m0 and the VMEM instruction -- inline asm is opaque to the hazard recognizer (4 covers
// a readfirstlane right in front; wino4.hip and wino4_wgrad.hip, whose operands are older, were tuned with 1).
template <int NOPS = 4>
__device__ __forceinline__ void dma16_sgpr(const void* sbase, unsigned voff, unsigned lds_dst) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop %3\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_dst), "n"(NOPS) : "memory");
}
// dma16: the base pointer and the LDS address are wave-uniform, but must BE in SGPRs: readfirstlane.
template <int NOPS = 4>
__device__ __forceinline__ void dma16(const void* gbase, unsigned voff, unsigned lds_dst) {
    const unsigned long long pv = reinterpret_cast<unsigned long long>(gbase);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)pv), hi = __builtin_amdgcn_readfirstlane((unsigned)(pv >> 32));
    dma16_sgpr<NOPS>(reinterpret_cast<const void*>(((unsigned long long)hi << 32) | lo), voff, __builtin_amdgcn_readfirstlane(lds_dst));
}
// The same with a full per-lane 64-bit source address (boundary tiles: lanes outside the image point at a zero buffer).
__device__ __forceinline__ void dma16v(const void* vaddr, unsigned lds_dst) {
    const unsigned la = __builtin_amdgcn_readfirstlane(lds_dst);
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 4\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(vaddr), "s"(la) : "memory");
}
// 4 KB linear copy global -> LDS by this wave (4 LDS-DMA instructions, one asm block: the base pointer reaches its SGPR
// pair once, the instruction's immediate offset advances the global AND the LDS address alike)
__device__ __forceinline__ void dma4k(const void* gbase, unsigned lane_off, unsigned lds_dst) {
    const unsigned long long pv = reinterpret_cast<unsigned long long>(gbase);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)pv), hi = __builtin_amdgcn_readfirstlane((unsigned)(pv >> 32));
    const unsigned long long b0 = ((unsigned long long)hi << 32) | lo;
    const unsigned la = __builtin_amdgcn_readfirstlane(lds_dst);
    asm volatile(
        "s_mov_b32 m0, %2\n\ts_nop 4\n\t"
        "global_load_lds_dwordx4 %0, %1\n\t"
        "global_load_lds_dwordx4 %0, %1 offset:1024\n\t"
        "global_load_lds_dwordx4 %0, %1 offset:2048\n\t"
        "global_load_lds_dwordx4 %0, %1 offset:3072"
        ::"v"(lane_off), "s"(b0), "s"(la) : "memory");
}
template <int N>
__device__ __forceinline__ void dma_wait() {   // all but the newest N vector-memory operations of this wave are done
    static_assert(N >= 0 && N < 64, "vmcnt range");
    __builtin_amdgcn_s_waitcnt((N & 15) | (7 << 4) | (15 << 8) | ((N >> 4) << 14));
}
// Raw barrier: no vmcnt(0) drain of the rings' prefetch (a __syncthreads() would); LDS reads of this wave retire first.
__device__ __forceinline__ void ring_publish() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}
// Rows are 64 B (16 floats) without padding; the 16-byte quads of a row are XOR-swizzled with SWZ[(row >> 2) & 3] on the
// DMA's SOURCE address and on the fragment reads: conflict-free ds_read_b128 for the 16-row x 4-quad fragment shape of
// the 16x16x4 MFMA operands (lane l reads row l & 15, quad l >> 4), while the LDS destination of a DMA stays lane-linear.
__device__ __forceinline__ int swz(int row) { return (0x1320 >> (4 * ((row >> 2) & 3))) & 3; }      // {0, 2, 3, 1}
