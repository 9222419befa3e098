// LDS-DMA (global_load_lds_*): HBM / L2 -> LDS with no VGPR round trip and no ds_write pass.  Every statement of the kernels that
// writes M0 lives here.
//
// Inline asm ON PURPOSE, not __builtin_amdgcn_global_load_lds: for the builtin hipcc places `s_waitcnt vmcnt(0)` in front of the
// next ds_read (it cannot prove the DMA targets the other buffer), which serialises the DMA of tile t+1 with the MFMAs of tile t.
// With the asm form the compiler sees no outstanding VMEM operation; the kernel waits by hand (wait_vmcnt before the barrier that
// publishes the tile).
//
// M0 (the LDS base of the instruction) cannot go on the clobber list - hipcc: "reserved register, may not be preserved" - so
// every statement saves M0 and puts it back ITSELF: the compiler keeps its own values in M0 across an asm
// statement.  A new form belongs in this file, built the same way.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tllm
{
namespace dev
{

// one instruction: 64 lanes x 16 bytes from per-lane global addresses to LDS [lds_byte + lane * 16]
__device__ __forceinline__ void glds16(const void* gptr, uint32_t lds_byte)
{
    uint32_t m0_keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0" : "=&s"(m0_keep) : "v"(gptr), "s"(lds_byte) : "memory");
}

// glds16 with the nt policy (weight rows read once per token)
__device__ __forceinline__ void glds16_nt(const void* gptr, uint32_t lds_byte)
{
    uint32_t m0_keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0" : "=&s"(m0_keep) : "v"(gptr), "s"(lds_byte) : "memory");
}

// the same from a wave-uniform base + a per-lane 32-bit offset
__device__ __forceinline__ void glds16s(const char* base, uint32_t off, uint32_t lds_byte)
{
    uint32_t m0_keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0" : "=&s"(m0_keep) : "v"(off), "s"(base), "s"(lds_byte) : "memory");
}

// glds16s with the nt policy: a stream read once per token stays out of the temporal cache lines
__device__ __forceinline__ void glds16s_nt(const char* base, uint32_t off, uint32_t lds_byte)
{
    uint32_t m0_keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 nt\n\ts_mov_b32 m0, %0" : "=&s"(m0_keep) : "v"(off), "s"(base), "s"(lds_byte) : "memory");
}

// 4 bytes per lane from per-lane 64-bit addresses (scales of two different tensors in one chunk)
__device__ __forceinline__ void glds4v(const void* gptr, uint32_t lds_byte)
{
    uint32_t m0_keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0" : "=&s"(m0_keep) : "v"(gptr), "s"(lds_byte) : "memory");
}

// 4 bytes per lane from a wave-uniform base + a per-lane 32-bit offset (scales)
__device__ __forceinline__ void glds4s(const char* base, uint32_t off, uint32_t lds_byte)
{
    uint32_t m0_keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0" : "=&s"(m0_keep) : "v"(off), "s"(base), "s"(lds_byte) : "memory");
}

// the hand-kept wait: at most N of this wave's VMEM operations (the LDS-DMA among them) still outstanding
template <int N>
__device__ __forceinline__ void wait_vmcnt()
{
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit counter");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

} // namespace dev
} // namespace tllm
