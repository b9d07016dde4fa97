// The machine-level primitives the gfx950 MFMA kernels stand on (the vector types are in common.h):
//  * LDS-DMA: buffer resources, LDS byte addresses and the `buffer_load ... lds` instruction (global -> LDS without passing
//    through VGPRs; lane-linear placement, out-of-range lanes are zero-filled), with the M0 contract of its asm form
//  * counted waits on the vector-memory counter
//  * typed LDS access by 32-bit byte address
//  * MFMA 16x16x32: one through the builtin, and the in-place asm groups
// A helper that one kernel file alone uses stays in that file.
#pragma once
#include "common.h"

namespace eve {

#define EVE_LDS __attribute__((address_space(3)))
typedef __attribute__((__vector_size__(4 * sizeof(__bf16)))) __bf16 bf16x4v_t;

__device__ __forceinline__ void lds_dma16(__amdgpu_buffer_rsrc_t rsrc, const void* lds_generic_ptr, int voffset) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (EVE_LDS void*)(lds_generic_ptr), 16, voffset, 0, 0, 0);
}
#define EVE_OOB ((int)0x80000000u)   // >= num_records for every tensor we accept (< 2^31 bytes)

// The same LDS-DMA as inline asm.  hipcc treats the builtin as a store to LDS and protects every later ds_read
// with s_waitcnt vmcnt(0), which drains a multi-stage prefetch ring at every step; an asm statement is opaque to
// that bookkeeping, so the waits are exactly the counted s_waitcnt vmcnt(N) the kernel places itself.
// M0 (the LDS destination base) is written inside the statement and declared clobbered.
//
// THE M0 CONTRACT.  hipcc warns "inline asm clobber list contains reserved registers: m0" for these statements: M0 is not
// allocatable, so the clobber is advisory, and what keeps the statements safe is a property of the CODE GENERATOR, not of
// the language: AMD clang (roc-7.2.0, clang 22) never keeps a value live in M0 across other code -- every M0 consumer it
// emits (LDS-DMA builtins, movrel, sendmsg) is preceded by its own `s_mov_b32 m0, ...` in the same basic block -- and none
// of the kernels that use the asm form contains such a compiler-generated consumer (they do not mix the builtin and the
// asm DMA).  Every asm statement here writes M0 in the SAME statement that reads it, so it depends on nothing outside.
// A different compiler must be re-verified (disassemble conv_igemm / stem_fused / cgru_scan and check that no instruction
// outside an ASMSTART/ASMEND pair reads m0 without its own s_mov; then run `pytest -m gpu`, whose parity tests cover every
// LDS-DMA kernel) before this guard is widened; -DEVE_M0_CONTRACT_VERIFIED overrides it for that experiment.
#if !defined(EVE_M0_CONTRACT_VERIFIED)
static_assert(__clang_major__ == 22, "lds_dma.h: the inline-asm M0 contract was verified for AMD clang 22 (ROCm 7.2) only -- "
                                     "re-verify it for this compiler (see the comment above), then extend this guard");
#endif
typedef int eve_int4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ eve_int4 make_rsrc_words(const void* base, uint32_t bytes) {
    const uint64_t a = (uint64_t)base;
    eve_int4 r;
    r.x = (int)(uint32_t)a;
    r.y = (int)(uint32_t)((a >> 32) & 0xffffu);      // stride 0
    r.z = (int)bytes;
    r.w = 0x00020000;
    return r;
}
__device__ __forceinline__ uint32_t lds_addr_of(const void* generic_ptr) {
    return (uint32_t)(uintptr_t)((EVE_LDS void*)generic_ptr);
}
__device__ __forceinline__ void lds_dma16_asm(const eve_int4& rsrc, uint32_t lds_byte_addr, int voffset) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds"
                 :: "s"(lds_byte_addr), "v"(voffset), "s"(rsrc)
                 : "memory", "m0");
}
// ... with the uniform part of the source address in the scalar offset (no VALU work per piece), and its one-dword form
__device__ __forceinline__ void lds_dma16_asm(const eve_int4& rsrc, uint32_t lds_byte_addr, int voffset, int soffset) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
                 :: "s"(lds_byte_addr), "v"(voffset), "s"(rsrc), "s"(soffset) : "memory", "m0");
}
__device__ __forceinline__ void lds_dma4_asm(const eve_int4& rsrc, uint32_t lds_byte_addr, int voffset, int soffset) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dword %1, %2, %3 offen lds"
                 :: "s"(lds_byte_addr), "v"(voffset), "s"(rsrc), "s"(soffset) : "memory", "m0");
}
// the counted wait that goes with them: at most N vector-memory operations (DMA pieces) still in flight
template <int N> __device__ __forceinline__ void wait_vm() {
    static_assert(N >= 0 && N <= 63, "vmcnt is a 6-bit field");
    asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory");
}

// ---------------------------------------------------------------------------------------------
// LDS access by 32-bit byte address
// ---------------------------------------------------------------------------------------------
// A 16-byte fragment stays ONE vector value from the LDS load to the MFMA operand.  (Round 6: as HIP's uint4 -- a struct -- the
// load was split into two 8-byte halves by the middle end and the back end re-merged the filter fragments as ds_read2_b64: twice
// the LDS cycles of ds_read_b128 and banked differently from what the swizzles are built for.  SQ counters of the stem's forward:
// 59 % of the LDS-array cycles were bank conflicts, the array 70 % busy, 23 % of the wave cycles stalled on LDS issue.)
typedef u32x4_t frag_t;
__device__ __forceinline__ frag_t lds_read16(uint32_t addr) { return *reinterpret_cast<const EVE_LDS u32x4_t*>((uintptr_t)addr); }
__device__ __forceinline__ u32x2_t lds_read8(uint32_t addr) { return *reinterpret_cast<const EVE_LDS u32x2_t*>((uintptr_t)addr); }
__device__ __forceinline__ float lds_read_f32(uint32_t addr) { return *reinterpret_cast<const EVE_LDS float*>((uintptr_t)addr); }
__device__ __forceinline__ void lds_write8(uint32_t addr, uint32_t x, uint32_t y) {
    *reinterpret_cast<EVE_LDS u32x2_t*>((uintptr_t)addr) = u32x2_t{x, y};
}
__device__ __forceinline__ void lds_write_f32(uint32_t addr, float v) { *reinterpret_cast<EVE_LDS float*>((uintptr_t)addr) = v; }

// ---------------------------------------------------------------------------------------------
// MFMA 16x16x32 on 16-byte fragments, format chosen by H
// ---------------------------------------------------------------------------------------------
// one MFMA through the builtin: acc(16 x 16) += A(16 rows x 32 k) * B(32 k x 16 cols); a / b are the lane's 8 consecutive k
template <typename H>
__device__ __forceinline__ void mfma16(f32x4_t& acc, const frag_t& a, const frag_t& b) {
    if constexpr (Elem<H>::IS_BF16)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), acc, 0, 0, 0);
    else
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), acc, 0, 0, 0);
}

// The in-place groups: several MFMAs as ONE asm statement with every accumulator tied in place (D == C).  Each body is written
// once, as a macro that takes the opcode string.

// 16 MFMAs (4 x 4 accumulator tiles, one K=32 chunk), accumulators in AGPRs ("+a").  Left to itself hipcc ping-pongs
// loop-carried accumulators between two register sets when each gets a single MFMA per trip, and copies them back with
// v_accvgpr_mov/read/write at the loop edge (10 VALU per MFMA measured in the weight-gradient loop).  The leading s_nop covers a
// VALU-assembled operand tuple; consecutive MFMAs here never share an accumulator.
#define EVE_MMA16_BODY(OP)                                                                                               \
    asm volatile(                                                                                                        \
        "s_nop 1\n\t"                                                                                                    \
        OP " %0, %16, %20, %0\n\t"   OP " %1, %16, %21, %1\n\t"   OP " %2, %16, %22, %2\n\t"   OP " %3, %16, %23, %3\n\t"   \
        OP " %4, %17, %20, %4\n\t"   OP " %5, %17, %21, %5\n\t"   OP " %6, %17, %22, %6\n\t"   OP " %7, %17, %23, %7\n\t"   \
        OP " %8, %18, %20, %8\n\t"   OP " %9, %18, %21, %9\n\t"   OP " %10, %18, %22, %10\n\t" OP " %11, %18, %23, %11\n\t" \
        OP " %12, %19, %20, %12\n\t" OP " %13, %19, %21, %13\n\t" OP " %14, %19, %22, %14\n\t" OP " %15, %19, %23, %15"     \
        : "+a"(acc[0][0]), "+a"(acc[0][1]), "+a"(acc[0][2]), "+a"(acc[0][3]), "+a"(acc[1][0]), "+a"(acc[1][1]),          \
          "+a"(acc[1][2]), "+a"(acc[1][3]), "+a"(acc[2][0]), "+a"(acc[2][1]), "+a"(acc[2][2]), "+a"(acc[2][3]),          \
          "+a"(acc[3][0]), "+a"(acc[3][1]), "+a"(acc[3][2]), "+a"(acc[3][3])                                             \
        : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(b[0]), "v"(b[1]), "v"(b[2]), "v"(b[3]))
template <typename H>
__device__ __forceinline__ void mma16_inplace(f32x4_t (&acc)[4][4], const uint4 (&a4)[4], const uint4 (&b4)[4]) {
    u32x4_t a[4], b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { a[i] = __builtin_bit_cast(u32x4_t, a4[i]); b[i] = __builtin_bit_cast(u32x4_t, b4[i]); }
    if constexpr (Elem<H>::IS_BF16) { EVE_MMA16_BODY("v_mfma_f32_16x16x32_bf16"); }
    else { EVE_MMA16_BODY("v_mfma_f32_16x16x32_f16"); }
}
#undef EVE_MMA16_BODY
// wait states between the last asm MFMA and compiler-generated reads of the accumulators
__device__ __forceinline__ void mma_drain() { asm volatile("s_nop 15\n\ts_nop 15" ::: "memory"); }

// four in-place MFMAs sharing the A operand: c[i] += a x b[i]
#define EVE_MMA4_BODY(OP)                                                                                         \
    asm volatile(                                                                                                 \
        "s_nop 1\n\t"                                                                                             \
        OP " %0, %4, %5, %0\n\t" OP " %1, %4, %6, %1\n\t" OP " %2, %4, %7, %2\n\t" OP " %3, %4, %8, %3"             \
        : "+a"(c0), "+a"(c1), "+a"(c2), "+a"(c3)                                                                  \
        : "v"(a), "v"(b[0]), "v"(b[1]), "v"(b[2]), "v"(b[3]))
template <typename H>
__device__ __forceinline__ void mma4_inplace(f32x4_t& c0, f32x4_t& c1, f32x4_t& c2, f32x4_t& c3, const uint4& a4, const uint4 (&b4)[4]) {
    u32x4_t b[4];
    const u32x4_t a = __builtin_bit_cast(u32x4_t, a4);
#pragma unroll
    for (int i = 0; i < 4; ++i) b[i] = __builtin_bit_cast(u32x4_t, b4[i]);
    if constexpr (Elem<H>::IS_BF16) { EVE_MMA4_BODY("v_mfma_f32_16x16x32_bf16"); }
    else { EVE_MMA4_BODY("v_mfma_f32_16x16x32_f16"); }
}
#undef EVE_MMA4_BODY

// four in-place MFMAs sharing the B operand: c[i] += a[i] x b
#define EVE_MMA4B_BODY(OP)                                                                                        \
    asm volatile(                                                                                                 \
        "s_nop 1\n\t"                                                                                             \
        OP " %0, %4, %8, %0\n\t" OP " %1, %5, %8, %1\n\t" OP " %2, %6, %8, %2\n\t" OP " %3, %7, %8, %3"             \
        : "+a"(c[0]), "+a"(c[1]), "+a"(c[2]), "+a"(c[3])                                                          \
        : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(b))
template <typename H>
__device__ __forceinline__ void mma4_inplace_b(f32x4_t (&c)[4], const uint4 (&a4)[4], const uint4& b4) {
    u32x4_t a[4];
    const u32x4_t b = __builtin_bit_cast(u32x4_t, b4);
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = __builtin_bit_cast(u32x4_t, a4[i]);
    if constexpr (Elem<H>::IS_BF16) { EVE_MMA4B_BODY("v_mfma_f32_16x16x32_bf16"); }
    else { EVE_MMA4B_BODY("v_mfma_f32_16x16x32_f16"); }
}
#undef EVE_MMA4B_BODY

// three in-place MFMAs sharing the A operand (one filter row): c[i] += a x b[i], and a single one.  "+v": accumulators in
// architectural VGPRs (unified file on gfx950): the epilogue reads them without a copy out of the AGPRs
#define EVE_MMA3_BODY(OP)                                                                                         \
    asm volatile(                                                                                                 \
        "s_nop 1\n\t"                                                                                             \
        OP " %0, %3, %4, %0\n\t" OP " %1, %3, %5, %1\n\t" OP " %2, %3, %6, %2"                                     \
        : "+v"(c0), "+v"(c1), "+v"(c2)                                                                            \
        : "v"(a), "v"(b0), "v"(b1), "v"(b2))
template <typename H>
__device__ __forceinline__ void mma3_inplace(f32x4_t& c0, f32x4_t& c1, f32x4_t& c2, const uint4& a4, const uint4 (&b4)[3]) {
    const u32x4_t a = __builtin_bit_cast(u32x4_t, a4);
    const u32x4_t b0 = __builtin_bit_cast(u32x4_t, b4[0]), b1 = __builtin_bit_cast(u32x4_t, b4[1]), b2 = __builtin_bit_cast(u32x4_t, b4[2]);
    if constexpr (Elem<H>::IS_BF16) { EVE_MMA3_BODY("v_mfma_f32_16x16x32_bf16"); }
    else { EVE_MMA3_BODY("v_mfma_f32_16x16x32_f16"); }
}
#undef EVE_MMA3_BODY
#define EVE_MMA1_BODY(OP) asm volatile("s_nop 1\n\t" OP " %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b))
template <typename H>
__device__ __forceinline__ void mma1_inplace(f32x4_t& c, const uint4& a4, const uint4& b4) {
    const u32x4_t a = __builtin_bit_cast(u32x4_t, a4), b = __builtin_bit_cast(u32x4_t, b4);
    if constexpr (Elem<H>::IS_BF16) { EVE_MMA1_BODY("v_mfma_f32_16x16x32_bf16"); }
    else { EVE_MMA1_BODY("v_mfma_f32_16x16x32_f16"); }
}
#undef EVE_MMA1_BODY

}  // namespace eve
