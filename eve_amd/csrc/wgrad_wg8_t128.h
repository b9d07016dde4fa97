// Weight gradient of the 128-input-channel 3 x 3 trunk layers (layer 2 stride 1, layer 3's stride-2 convolution), eight-wave
// workgroups: 128 output channels x 384 filter-K values (one filter row: three taps x 128 input channels) per workgroup, a wave owns
// 64 x 96 (24 accumulator tiles of 16 x 16).  The sibling of wgrad_wg8_kernel (wgrad_wg8.h) for the shapes its 256 x 256 tile does
// not divide: Cout = 128 and K = 1 152 = 3 x 384 exactly, no padded K.
//
// Why: wgrad_tr_kernel<2,2> serves these layers with 128 x 128 tiles, 16 KB of LDS-DMA per 64 MFMAs; this tile moves 32 KB per
// 192 MFMAs (10.7 KB per 64) and has wgrad_wg8_kernel's instruction mix: 20 transposing reads + 4 DMAs per 24 MFMAs and wave, every
// LDS address a lane constant plus an immediate, the two-group role split.  Measurements: profiles/r08_wgrad_wg8_tile128.md.
//
// Stage layout (32 KB): dy rows [32 pixels][128 channels] = 256 B each (8 KB, one 16-byte slot per thread), then the gathered x rows
// [32 pixels][3 taps x 128 channels] = 768 B each (24 KB, three slots per thread).  Both pitches are multiples of 256 B, so every
// row starts on bank 0 and the three-bit key of tr_key (row bits 0, 1, 3, XOR-ed into bits 1..3 of the slot index) spreads the eight
// rows x 32 B a half-wave reads at once over the 64 banks; the XOR stays inside an aligned group of 16 slots, which both 16 and 48
// slots per row are made of.  (tools/probes/lds_tr_pattern.hip times these two read patterns next to a linear and an unkeyed one.)
//
// Ring: wgrad_wg8_kernel's.  4 stages of 32 KB; stage s+2 is issued in interval s by both groups (4 DMAs per thread, as there, so
// the counted wait is the same vmcnt(4)), waited for at the end of interval s+1, read in interval s+2.  Its slot held stage s-2:
// group 0 read it at the start of interval s-2 and multiplied in the same interval; group 1 read it at the end of interval s-2 and
// its multiply at the start of interval s-1 waits for those reads (lgkmcnt(0)) before the barrier that ends interval s-1 -- so when
// any wave issues into the slot in interval s, every read of it has returned.  Steps past the end of a split issue out-of-range
// (zero-fill) DMAs: the count per wave and step is uniform.
#pragma once
#include "common.h"
#include "lds_dma.h"
#include "conv_fast.h"

namespace eve {

// SLAB as in wgrad_wg8_kernel: partial filter tiles stored into slab `split` of a scratch buffer ([split][Cout][K] floats, added into
// dw by wgrad_slab_reduce_kernel), else float atomics straight into dw.  Requires (launch_wgrad): KH = KW = 3, Cin = 128,
// Cout % 128 == 0, OH and OW powers of two, tensors below 2^31 bytes.
template <typename H, bool SLAB>
__global__ __launch_bounds__(512, 2) void wgrad_wg8_t128_kernel(const GatherParams p, const H* __restrict__ x,
                                                                const H* __restrict__ dy, float* __restrict__ dw,
                                                                const uint32_t rows_per_split, const uint32_t x_bytes,
                                                                const uint32_t dy_bytes) {
    constexpr int WK = 4;                                    // waves: 2 (channel halves of 64) x 4 (K quarters of 96)
    constexpr int BCO = 128, BKK = 384;
    constexpr int PROW = BCO * 2, QROW = BKK * 2;            // bytes per pixel row: 256 / 768
    constexpr int PSL = PROW / 16, QSL = QROW / 16;          // 16-byte slots per row: 16 / 48
    constexpr int STEP = 32, NT = 512;
    constexpr int QJ = STEP * QSL / NT;                      // x slots per thread and stage: 3 (dy: STEP * PSL == NT, one)
    constexpr int QBASE = STEP * PROW;                       // x rows follow the dy rows of a stage
    constexpr int BUF = STEP * (PROW + QROW);                // 32 KB per stage
    static_assert(STEP * PSL == NT && STEP * QSL == QJ * NT && BUF == 32768, "slot count per thread");
    extern __shared__ __attribute__((aligned(16))) char lds[];

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t tk = (uint32_t)p.K / BKK, tc = (uint32_t)p.Cout / BCO;
    const uint32_t lid = tk * tc >= 4 ? xcd_remap(blockIdx.x, gridDim.x) : blockIdx.x;
    const uint32_t k0 = (lid % tk) * BKK, co0 = ((lid / tk) % tc) * BCO;
    const uint32_t m_begin = (lid / (tk * tc)) * rows_per_split;
    const uint32_t m_end = min(p.M, m_begin + rows_per_split);

    const eve_int4 rs_x = make_rsrc_words(x, x_bytes);
    const eve_int4 rs_dy = make_rsrc_words(dy, dy_bytes);
    const uint32_t lds0 = lds_addr_of(lds);

    // ---- DMA slots (lane constants): dy = P operand, gathered x = Q operand ----
    const int cin2 = p.Cin * 2, cout2 = p.Cout * 2;
    const int sh_w = __builtin_ctz((unsigned)p.OW), sh_hw = __builtin_ctz((unsigned)(p.OH * p.OW));
    int p_row, p_const, q_row[QJ], q_const[QJ], q_ty[QJ], q_tx[QJ];
    {
        const int row = tid / PSL, sl = tid % PSL;
        const int sg = sl ^ (tr_key<PROW>(row) << 1);
        p_row = row;
        p_const = row * cout2 + (int)(co0 + sg * 8) * 2;                         // (Cout is a multiple of 128: never out of range)
    }
#pragma unroll
    for (int j = 0; j < QJ; ++j) {
        const int q = tid + NT * j;
        const int row = q / QSL, sl = q % QSL;
        const int sg = sl ^ (tr_key<QROW>(row) << 1);
        q_row[j] = row;
        const uint32_t k = k0 + sg * 8;                                          // (K is a multiple of 384: never out of range)
        const uint32_t tap = fd_div(k, p.fd_cin), kh = fd_div(tap, p.fd_kw);
        const int col = (int)(k - tap * (uint32_t)p.Cin) * 2;
        const int ddy = (int)kh * p.k_mul + p.off, ddx = (int)(tap - kh * (uint32_t)p.KW) * p.k_mul + p.off;
        const uint32_t r = (uint32_t)row;
        const int n_t = (int)(r >> sh_hw), oy_t = (int)((r >> sh_w) & (uint32_t)(p.OH - 1)), ox_t = (int)(r & (uint32_t)(p.OW - 1));
        q_ty[j] = oy_t * p.o_mul + ddy;
        q_tx[j] = ox_t * p.o_mul + ddx;
        q_const[j] = ((n_t * p.IH + q_ty[j]) * p.IW + q_tx[j]) * cin2 + col;
    }
    // source offsets of the stage that starts at pixel mbase (a multiple of 32); rows past the split's end: zero fill
    auto offsets = [&](uint32_t mbase, int& vp, int* vq) {
        const uint32_t left = m_end > mbase ? m_end - mbase : 0u;
        const int pbase = (int)mbase * cout2;
        const uint32_t n_s = mbase >> sh_hw, oy_s = (mbase >> sh_w) & (uint32_t)(p.OH - 1), ox_s = mbase & (uint32_t)(p.OW - 1);
        const int sy0 = (int)oy_s * p.o_mul, sx0 = (int)ox_s * p.o_mul;
        const int qbase = (((int)n_s * p.IH + sy0) * p.IW + sx0) * cin2;
        vp = (uint32_t)p_row < left ? pbase + p_const : EVE_OOB;
#pragma unroll
        for (int j = 0; j < QJ; ++j) {
            const bool ok = ((uint32_t)q_row[j] < left) & ((uint32_t)(sy0 + q_ty[j]) < (uint32_t)p.IH) &
                            ((uint32_t)(sx0 + q_tx[j]) < (uint32_t)p.IW);
            vq[j] = ok ? qbase + q_const[j] : EVE_OOB;
        }
    };
    auto issue = [&](int slot, const int vp, const int* vq) {
        const uint32_t pb = lds0 + slot * BUF, qb = pb + QBASE;
        lds_dma16_asm(rs_dy, pb + wave * 64 * 16, vp);
#pragma unroll
        for (int j = 0; j < QJ; ++j) lds_dma16_asm(rs_x, qb + (wave * 64 + NT * j) * 16, vq[j]);
    };

    // ---- fragment addresses (lane constants; ring slot and the +4-row half are immediates) ----
    const int lane = tid & 63;
    const int wco = wave / WK, wk = wave % WK;
    const int t = lane & 15, g = lane >> 4;
    const int lrow = 8 * g + (t >> 2);
    const int key = tr_key<PROW>(lrow);                      // (bits 0, 1, 3 of the row: the same for row + 4, and for both pitches)
    static_assert(PROW % 256 == 0 && QROW % 256 == 0, "one key for both operands");
    const int half = (t & 1) * 8, hs = (t & 3) >> 1;
    uint32_t poff[4], qoff[6];
#pragma unroll
    for (int i = 0; i < 4; ++i) poff[i] = lds0 + lrow * PROW + (((wco * 8 + i * 2 + hs) ^ (key << 1)) * 16) + half;
#pragma unroll
    for (int i = 0; i < 6; ++i) qoff[i] = lds0 + QBASE + lrow * QROW + (((wk * 12 + i * 2 + hs) ^ (key << 1)) * 16) + half;

    f32x4_t acc[6][4];                                       // [16-k tile][16-channel tile]
#pragma unroll
    for (int b = 0; b < 6; ++b)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[b][c] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    if (m_begin < m_end) {
        const int nsteps = (int)((m_end - m_begin + STEP - 1) / STEP);
        const bool lead = wave < 4;
        int vp, vq[QJ];
        offsets(m_begin, vp, vq);
        issue(0, vp, vq);
        offsets(m_begin + STEP, vp, vq);
        issue(1, vp, vq);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (!lead) __builtin_amdgcn_s_setprio(2);
        uint4 fp[4], fq[6];
#pragma unroll
        for (int i = 0; i < 4; ++i) fp[i] = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (int i = 0; i < 6; ++i) fq[i] = make_uint4(0u, 0u, 0u, 0u);
        auto mma = [&]() {
#pragma unroll
            for (int i = 0; i < 6; ++i) mma4_inplace_b<H>(acc[i], fp, fq[i]);
        };
        // one step; SLOT = st & 3 is a template constant so that every fragment address is base + immediate (the offset field
        // of an LDS read is 16 bits: the upper half of the ring goes through base + 65536)
        auto step = [&](int st, auto slot_c) {
            constexpr int SLOT = decltype(slot_c)::value;
            if (!lead) mma();                                                   // step st - 1 (zeros before step 0)
            constexpr int SB = SLOT * BUF;
            constexpr int HI = SB >= 65536 ? 65536 : 0;
            static_assert(SB - HI + 4 * QROW < 65536 && SB - HI + 4 * PROW < 65536, "immediate range");
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint2 a0 = lds_tr_read<SB - HI>(poff[i] + HI);
                const uint2 a1 = lds_tr_read<SB - HI + 4 * PROW>(poff[i] + HI);
                fp[i] = make_uint4(a0.x, a0.y, a1.x, a1.y);
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const uint2 b0 = lds_tr_read<SB - HI>(qoff[i] + HI);
                const uint2 b1 = lds_tr_read<SB - HI + 4 * QROW>(qoff[i] + HI);
                fq[i] = make_uint4(b0.x, b0.y, b1.x, b1.y);
            }
            // stage st + 2 (all out of range past the end: zero fill, so every step issues and waits for the same count)
            offsets(m_begin + (uint32_t)(st + 2) * STEP, vp, vq);
            issue((SLOT + 2) & 3, vp, vq);
            if (lead) mma();
            asm volatile("s_waitcnt vmcnt(4)" ::: "memory");                  // everything older than this step's four DMAs
            __builtin_amdgcn_s_barrier();
        };
        int st = 0;
        for (; st + 4 <= nsteps; st += 4) {
            step(st, std::integral_constant<int, 0>{});
            step(st + 1, std::integral_constant<int, 1>{});
            step(st + 2, std::integral_constant<int, 2>{});
            step(st + 3, std::integral_constant<int, 3>{});
        }
        // 0..3 remaining steps (a whole number of ring turns was done, the next slot is 0 again)
        if (st < nsteps) step(st, std::integral_constant<int, 0>{});
        if (st + 1 < nsteps) step(st + 1, std::integral_constant<int, 1>{});
        if (st + 2 < nsteps) step(st + 2, std::integral_constant<int, 2>{});
        if (!lead) mma();                                                       // group 1's last step
        __builtin_amdgcn_s_setprio(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                       // the zero-fill DMAs, before LDS is released
    }
    // wait states between the last MFMA and the first read of an accumulator: the statement NAMES the accumulators (a
    // memory clobber does not order register-only instructions, conv_wg8.h)
    asm volatile("s_nop 15\n\ts_nop 15"
                 : "+a"(acc[0][0]), "+a"(acc[0][1]), "+a"(acc[0][2]), "+a"(acc[0][3]), "+a"(acc[1][0]), "+a"(acc[1][1]),
                   "+a"(acc[1][2]), "+a"(acc[1][3]), "+a"(acc[2][0]), "+a"(acc[2][1]), "+a"(acc[2][2]), "+a"(acc[2][3]) :: "memory");
    asm volatile("s_nop 15\n\ts_nop 15"
                 : "+a"(acc[3][0]), "+a"(acc[3][1]), "+a"(acc[3][2]), "+a"(acc[3][3]), "+a"(acc[4][0]), "+a"(acc[4][1]),
                   "+a"(acc[4][2]), "+a"(acc[4][3]), "+a"(acc[5][0]), "+a"(acc[5][1]), "+a"(acc[5][2]), "+a"(acc[5][3]) :: "memory");
    float* const dst = SLAB ? dw + (size_t)(lid / (tk * tc)) * ((size_t)p.Cout * p.K) : dw;      // slab of this pixel split
#pragma unroll
    for (int kt = 0; kt < 6; ++kt) {
        const uint32_t k = k0 + wk * 96 + kt * 16 + t;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint32_t co = co0 + wco * 64 + mt * 16 + g * 4 + r;
                if (SLAB) dst[(size_t)co * p.K + k] = acc[kt][mt][r];
                else atomicAdd(dst + (size_t)co * p.K + k, acc[kt][mt][r]);
            }
    }
}

// dw[i] += sum over the `splits` slabs, for MANY slabs of a SMALL filter (layer 2 at B = 32: 85 slabs of 590 KB).  There
// wgrad_slab_reduce_kernel has 144 workgroups whose threads walk the 85 slabs one dependent add after the other: 23 us for 50 MB
// (2.2 TB/s, profiles/r08_wgrad_wg8_tile128.md).  Here a workgroup owns 32 float4 columns and its eight quarter-waves take every
// eighth slab each (partials through LDS, added in a fixed order: the result does not depend on the launch's timing).
__global__ __launch_bounds__(256) void wgrad_slab_reduce_wide_kernel(const float* __restrict__ slabs, float* __restrict__ dw,
                                                                     const long long n4, const int splits) {
    __shared__ float4 part[8][32];
    const int c = threadIdx.x & 31, q = threadIdx.x >> 5;
    const long long i = (long long)blockIdx.x * 32 + c;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < n4) {
#pragma unroll 4
        for (int s = q; s < splits; s += 8) {
            const float4 b = reinterpret_cast<const float4*>(slabs)[(long long)s * n4 + i];
            a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        }
    }
    part[q][c] = a;
    __syncthreads();
    if (q == 0 && i < n4) {
        float4 r = reinterpret_cast<const float4*>(dw)[i];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float4 b = part[j][c];
            r.x += b.x; r.y += b.y; r.z += b.z; r.w += b.w;
        }
        reinterpret_cast<float4*>(dw)[i] = r;
    }
}

}  // namespace eve
