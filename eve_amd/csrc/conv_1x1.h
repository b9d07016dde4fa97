// 1x1 / stride 1 convolutions between 16..128 channels as a STREAMING kernel (round 4).
// RefineNet's skip_layer convolutions (refine_net.py:59-60 of the reference: nn.Conv2d(ic, oc, kernel_size=1)) and their data
// gradients on the two outer levels (72x128 and 36x64 pixels, 960 frames: 2.2-8.8 M pixels, 16-128 channels) move 0.7-1.7 GB
// per launch for 4-70 GFLOP: pure HBM streaming.  They ran on the LDS-DMA gather kernel through pixel grouping (F pixels as one
// 64-channel pixel and a block-diagonal filter, ops.PAIR_FACTOR_1X1) at 1.6-2.3 TB/s: that kernel stages a 64-channel K step of
// a 128-256-pixel tile through LDS behind a workgroup barrier, for a product that needs no data reuse at all.
// Here there is no LDS and no barrier: the filter (<= 128 x 128) lives in each wave's registers as MFMA A operands, a wave
// reads 16-pixel tiles as B operands straight from global memory (lane = pixel t, 8 consecutive channels g: 16 contiguous
// bytes; a wave instruction covers 1 KB contiguous for 32 channels), and the transposed product
//        D[cout][pixel] = sum_k W[cout][k] * X[pixel][k]
// leaves every lane with consecutive OUTPUT CHANNELS of ONE pixel -- the rows of two 16-row tiles are dealt so that lane (t, g)
// holds channels 32a + 8g .. 8g + 7 of pixel t: one 16-byte store, 64 contiguous bytes per pixel and tile pair.
// All loads of a batch (TB tiles, and the tensor accumulated into) are issued before the first MFMA; bounds are the buffer
// resource's (out-of-range loads return 0, stores are dropped): no branch in the loop.
// 16 input channels: a load instruction covers 32 pixels (lanes g < 2: pixels 0..15, g >= 2: pixels 16..31, 8 channels each);
// the two halves go through two MFMAs whose B operand is zeroed in the other half's lanes, the filter sits in both k halves.
#pragma once
#include "common.h"

namespace eve {


template <int CIN, int COUT>
struct C1Geom {
    static constexpr int KS = CIN <= 32 ? 1 : CIN / 32;        // MFMA k steps (32 channels each)
    static constexpr int NT = COUT / 16;                        // 16-row output tiles
    static constexpr int TB = (KS * NT <= 4) ? 4 : 2;           // 16-pixel tiles per batch and wave
    static constexpr int PIX = 16 * TB;                         // pixels per batch
};

template <typename H, int CIN, int COUT, bool ACC>
__global__ __launch_bounds__(256) void conv1x1_stream_kernel(const H* __restrict__ x, const H* __restrict__ w, const float* __restrict__ bias,
                                                             int act, H* __restrict__ out, uint32_t M, uint32_t batches_per_wave) {
    using G = C1Geom<CIN, COUT>;
    constexpr int KS = G::KS, NT = G::NT, TB = G::TB;
    constexpr int NP = NT >= 2 ? NT / 2 : 1;                    // output pieces per pixel and lane (16 bytes each; 8 for COUT = 16)
    const int lane = threadIdx.x & 63, t = lane & 15, g = lane >> 4;
    const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6);
    // ---- the filter as A operands: tile a, row r = t <-> output channel co(a, t) ----
    uint4 wa[NT][KS];
#pragma unroll
    for (int a = 0; a < NT; ++a) {
        const int co = NT >= 2 ? 32 * (a >> 1) + 8 * (t >> 2) + 4 * (a & 1) + (t & 3) : t;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int k0 = CIN == 16 ? 8 * (g & 1) : 32 * ks + 8 * g;
            wa[a][ks] = *reinterpret_cast<const uint4*>(w + (size_t)co * CIN + k0);
        }
    }
    float bv[NP][8];
#pragma unroll
    for (int a = 0; a < NP; ++a)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = NT >= 2 ? 32 * a + 8 * g + e : 4 * g + (e & 3);
            bv[a][e] = bias ? bias[c] : 0.f;
        }
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, (int)(M * (uint32_t)(CIN * 2)), 0x00020000);
    const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc((void*)out, 0, (int)(M * (uint32_t)(COUT * 2)), 0x00020000);
    for (uint32_t b = 0; b < batches_per_wave; ++b) {
        const uint32_t p0 = (wave * batches_per_wave + b) * (uint32_t)G::PIX;
        if (p0 >= M) break;                                                    // wave-uniform
        // ---- loads: the pixels (B operands) and, when accumulating, what the output holds ----
        uint4 xb[CIN == 16 ? TB / 2 : TB][KS];
        if constexpr (CIN == 16) {
#pragma unroll
            for (int j = 0; j < TB / 2; ++j) {
                const uint32_t p = p0 + 32u * j + 16u * (g >> 1) + t;
                xb[j][0] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rx, (int)(p * 32u + 16u * (g & 1)), 0, 0));
            }
        } else {
#pragma unroll
            for (int i = 0; i < TB; ++i)
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const uint32_t p = p0 + 16u * i + t;
                    xb[i][ks] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rx, (int)(p * (uint32_t)(CIN * 2) + 64u * ks + 16u * g), 0, 0));
                }
        }
        uint4 prev[ACC ? TB : 1][NP];
        if constexpr (ACC) {
#pragma unroll
            for (int i = 0; i < TB; ++i)
#pragma unroll
                for (int a = 0; a < NP; ++a) {
                    const uint32_t p = p0 + 16u * i + t;
                    if constexpr (NT >= 2) {
                        prev[i][a] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(ro, (int)(p * (uint32_t)(COUT * 2) + 64u * a + 16u * g), 0, 0));
                    } else {
                        const u32x2_t v = __builtin_amdgcn_raw_buffer_load_b64(ro, (int)(p * 32u + 8u * g), 0, 0);
                        prev[i][a] = make_uint4(v.x, v.y, 0u, 0u);
                    }
                }
        }
        // ---- products ----
        f32x4_t acc[TB][NT];
#pragma unroll
        for (int i = 0; i < TB; ++i)
#pragma unroll
            for (int a = 0; a < NT; ++a) {
                acc[i][a] = f32x4_t{0.f, 0.f, 0.f, 0.f};
                if constexpr (CIN == 16) {
                    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
                    const bool mine = (g >> 1) == (i & 1);          // this lane's load holds a pixel of tile i (else: of its neighbour)
                    Elem<H>::mfma(acc[i][a], wa[a][0], mine ? xb[i >> 1][0] : z);
                } else {
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) Elem<H>::mfma(acc[i][a], wa[a][ks], xb[i][ks]);
                }
            }
        // ---- epilogue: bias, activation, accumulate, one store per pixel and tile pair ----
#pragma unroll
        for (int i = 0; i < TB; ++i) {
            const uint32_t p = p0 + 16u * i + t;
#pragma unroll
            for (int a = 0; a < NP; ++a) {
                float o[8];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    o[e] = acc[i][NT >= 2 ? 2 * a : 0][e] + bv[a][e];
                    o[4 + e] = NT >= 2 ? acc[i][NT >= 2 ? 2 * a + 1 : 0][e] + bv[a][4 + e] : 0.f;
                }
                if (act != EVE_ACT_NONE) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) o[e] = act_fwd(o[e], act);
                }
                if constexpr (ACC) {
                    float pv[8];
                    Elem<H>::unpack(prev[i][a], pv);
#pragma unroll
                    for (int e = 0; e < 8; ++e) o[e] += pv[e];
                }
                const uint4 q = Elem<H>::pack(o);
                // (the whole offset in the vector operand, immediate 0 as the scalar one: see norm_fused.hip `stv`)
                if constexpr (NT >= 2) {
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, q), ro, (int)(p * (uint32_t)(COUT * 2) + 64u * a + 16u * g), 0, 0);
                } else {
                    u32x2_t v;
                    v.x = q.x; v.y = q.y;
                    __builtin_amdgcn_raw_buffer_store_b64(v, ro, (int)(p * 32u + 8u * g), 0, 0);
                }
            }
        }
    }
}

// true: launched.  x [M][CIN] -> out [M][COUT] (+= with EVE_EPI_ACC), w [COUT][CIN]
template <typename H>
static bool launch_conv1x1_stream(long long M, int Cin, int Cout, const void* x, const void* w, const float* bias, int epi_act,
                                  void* out, hipStream_t s) {
    if (!g_cfg.conv1x1_stream || M < 16384 || (M + 64) * (long long)Cin * 2 >= (1ll << 32) || (M + 64) * (long long)Cout * 2 >= (1ll << 32)) return false;
    const int act = epi_act & 0xff;
    const bool accf = (epi_act & EVE_EPI_ACC) != 0;
#define EVE_C1_CASE(CI, CO)                                                                                                        \
    if (Cin == CI && Cout == CO) {                                                                                                 \
        using G = C1Geom<CI, CO>;                                                                                                  \
        const long long batches = (M + G::PIX - 1) / G::PIX;                                                                       \
        long long bpw = batches / (4 * 4096);                                                                                      \
        bpw = bpw < 1 ? 1 : (bpw > 8 ? 8 : bpw);                                                                                   \
        const unsigned grid = (unsigned)((batches + 4 * bpw - 1) / (4 * bpw));                                                     \
        if (accf) EVE_LAUNCH(EVE_HNAME(H, "conv1x1_stream_kernel<", ", " #CI ", " #CO ", true>"), (conv1x1_stream_kernel<H, CI, CO, true>),  \
                             dim3(grid), dim3(256), 0, s, (const H*)x, (const H*)w, bias, act, (H*)out, (uint32_t)M, (uint32_t)bpw);         \
        else EVE_LAUNCH(EVE_HNAME(H, "conv1x1_stream_kernel<", ", " #CI ", " #CO ", false>"), (conv1x1_stream_kernel<H, CI, CO, false>),     \
                        dim3(grid), dim3(256), 0, s, (const H*)x, (const H*)w, bias, act, (H*)out, (uint32_t)M, (uint32_t)bpw);              \
        return true;                                                                                                               \
    }
    EVE_C1_CASE(16, 32) EVE_C1_CASE(32, 16) EVE_C1_CASE(16, 64) EVE_C1_CASE(64, 16) EVE_C1_CASE(32, 64) EVE_C1_CASE(64, 32)
    EVE_C1_CASE(32, 128) EVE_C1_CASE(128, 32) EVE_C1_CASE(64, 128) EVE_C1_CASE(128, 64) EVE_C1_CASE(16, 16) EVE_C1_CASE(32, 32)
    EVE_C1_CASE(64, 64)
#undef EVE_C1_CASE
    return false;
}

// ---- 1x1 / stride 2 / pad 0: the shortcut convolutions of the ResNet trunk's down-sampling blocks (64 -> 128 at 32 x 32,
// 128 -> 256 at 16 x 16; 1 920 images a step) and their data gradients added into the 3x3 branch's.
// They ran on the LDS-DMA gather kernel, whose K loop has 2-4 steps at these depths: every tile prologue, barriers and epilogue,
// at 2.2-3.0 TB/s of their own traffic.  The same streaming product as above, with ONE side strided:
//   forward        y[p][:]        = W . x[s(p)][:]          p = (n, oy, ox) contiguous, s(p) = (n, 2 oy, 2 ox) in the IH x IW image
//   data gradient  dx[s(p)][:]   += W^T . dd[p][:]          only one pixel in four of dx is read and written
// A pixel record is >= 128 bytes, so a lane group still moves whole lines.  The filter no longer fits one wave's registers
// beyond 64 <-> 128: the output channels are dealt over the four waves of a workgroup in slices of CSL, each wave holding its
// slice (16 operand registers of 16 bytes) and reading the same pixel records, which its neighbours have just pulled into the
// CU's cache.  No LDS, no barrier.  Out-of-range pixels get an offset beyond both resources.
struct C1S2Params {
    uint32_t M, bpw;                    // output-side pixels N * OH * OW; batches per pixel group
    uint32_t IH, IW, OW, OHW;
    FastDiv fd_ohw, fd_ow;
    uint32_t strided_bytes, dense_bytes;   // of the IH x IW tensor / of the OH x OW tensor
};

template <int CIN, int COUT>
struct C1S2Geom {
    static constexpr int KS = CIN / 32;                                              // MFMA k steps
    static constexpr int CSL0 = 256 / KS < 32 ? 32 : 256 / KS;                       // 16 operand registers, at least one tile pair
    static constexpr int CSL = CSL0 < COUT ? CSL0 : COUT;                            // output channels per wave
    static constexpr int NSL = COUT / CSL;                                           // slices = waves sharing a pixel group
    static constexpr int WAVES = 4;                                                  // per workgroup
    static constexpr int GPB = WAVES / NSL;                                          // pixel groups per workgroup
    static constexpr int NT = CSL / 16;                                              // 16-row output tiles per wave
    static constexpr int NP = NT / 2;                                                // 16-byte output pieces per pixel and lane
    static constexpr int TB = 2;                                                     // 16-pixel tiles per batch
    static constexpr int PIX = 16 * TB;
    static_assert(CIN % 32 == 0 && COUT % CSL == 0 && CSL % 32 == 0 && WAVES % NSL == 0, "conv1x1_s2 geometry");
};

// DGRAD false: x strided [N][IH][IW][CIN], out dense [M][COUT], stored.  true: x dense [M][CIN], out strided, accumulated into.
template <typename H, int CIN, int COUT, bool DGRAD>
__global__ __launch_bounds__((64 * C1S2Geom<CIN, COUT>::WAVES)) void conv1x1_s2_stream_kernel(const C1S2Params p, const H* __restrict__ x,
                                                                                         const H* __restrict__ w, H* __restrict__ out) {
    using G = C1S2Geom<CIN, COUT>;
    constexpr int KS = G::KS, NT = G::NT, NP = G::NP, TB = G::TB;
    constexpr uint32_t OOB = 0x80000000u;                       // both tensors are below 2 GiB (launch gate)
    const int lane = threadIdx.x & 63, t = lane & 15, g = lane >> 4;
    const uint32_t wid = threadIdx.x >> 6;
    const uint32_t group = blockIdx.x * (uint32_t)G::GPB + wid / (uint32_t)G::NSL;
    const uint32_t c0 = (wid % (uint32_t)G::NSL) * (uint32_t)G::CSL;          // this wave's first output channel
    uint4 wa[NT][KS];
#pragma unroll
    for (int a = 0; a < NT; ++a) {
        const int co = (int)c0 + 32 * (a >> 1) + 8 * (t >> 2) + 4 * (a & 1) + (t & 3);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) wa[a][ks] = *reinterpret_cast<const uint4*>(w + (size_t)co * CIN + 32 * ks + 8 * g);
    }
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, (int)(DGRAD ? p.dense_bytes : p.strided_bytes), 0x00020000);
    const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc((void*)out, 0, (int)(DGRAD ? p.strided_bytes : p.dense_bytes), 0x00020000);
    for (uint32_t b = 0; b < p.bpw; ++b) {
        const uint32_t p0 = (group * p.bpw + b) * (uint32_t)G::PIX;
        if (p0 >= p.M) break;                                                  // wave-uniform
        uint32_t xo[TB], oo[TB];                                               // byte offsets of this lane's pixel in x / out
#pragma unroll
        for (int i = 0; i < TB; ++i) {
            const uint32_t q = p0 + 16u * i + t;
            const uint32_t n = fd_div(q, p.fd_ohw), r = q - n * p.OHW;
            const uint32_t oy = fd_div(r, p.fd_ow), ox = r - oy * p.OW;
            const uint32_t sp = (n * p.IH + 2u * oy) * p.IW + 2u * ox;          // the strided side's pixel
            const bool ok = q < p.M;
            xo[i] = ok ? (DGRAD ? q : sp) * (uint32_t)(CIN * 2) + 16u * g : OOB;
            oo[i] = ok ? (DGRAD ? sp : q) * (uint32_t)(COUT * 2) + c0 * 2u + 16u * g : OOB;
        }
        uint4 xb[TB][KS];
#pragma unroll
        for (int i = 0; i < TB; ++i)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
                xb[i][ks] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rx, (int)(xo[i] + 64u * ks), 0, 0));
        uint4 prev[DGRAD ? TB : 1][NP];
        if constexpr (DGRAD) {
#pragma unroll
            for (int i = 0; i < TB; ++i)
#pragma unroll
                for (int a = 0; a < NP; ++a)
                    prev[i][a] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(ro, (int)(oo[i] + 64u * a), 0, 0));
        }
        f32x4_t acc[TB][NT];
#pragma unroll
        for (int i = 0; i < TB; ++i)
#pragma unroll
            for (int a = 0; a < NT; ++a) {
                acc[i][a] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) Elem<H>::mfma(acc[i][a], wa[a][ks], xb[i][ks]);
            }
#pragma unroll
        for (int i = 0; i < TB; ++i)
#pragma unroll
            for (int a = 0; a < NP; ++a) {
                float o[8];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    o[e] = acc[i][2 * a][e];
                    o[4 + e] = acc[i][2 * a + 1][e];
                }
                if constexpr (DGRAD) {
                    float pv[8];
                    Elem<H>::unpack(prev[i][a], pv);
#pragma unroll
                    for (int e = 0; e < 8; ++e) o[e] += pv[e];
                }
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, Elem<H>::pack(o)), ro, (int)(oo[i] + 64u * a), 0, 0);
            }
    }
}

// true: launched.  Forward (dgrad false): in = x [N][IH][IW][Cin], w [Cout][Cin], out = y [N][OH][OW][Cout].  Data gradient added
// into dx (dgrad true): in = dy [N][OH][OW][Cout], w [Cin][Cout], out = dx [N][IH][IW][Cin].  conv1x1_stream = 2 keeps these
// shapes on the gather kernel while the stride-1 kernel above stays on.
template <typename H>
static bool launch_conv1x1_s2_stream(const eve_conv_desc* d, bool dgrad, const void* in, const void* w, void* out, hipStream_t s) {
    if (g_cfg.conv1x1_stream != 1 || d->KH != 1 || d->KW != 1 || d->stride != 2 || d->pad != 0) return false;
    if (d->OH != (d->IH - 1) / 2 + 1 || d->OW != (d->IW - 1) / 2 + 1) return false;
    const long long M = (long long)d->N * d->OH * d->OW;
    const long long sb = (long long)d->N * d->IH * d->IW * d->Cin * 2, db = M * d->Cout * 2;
    if (M < 1 || M + 64 >= (1ll << 31) || sb >= (1ll << 31) || db >= (1ll << 31)) return false;
    C1S2Params p;
    p.M = (uint32_t)M; p.IH = (uint32_t)d->IH; p.IW = (uint32_t)d->IW; p.OW = (uint32_t)d->OW; p.OHW = (uint32_t)(d->OH * d->OW);
    p.fd_ohw = make_fastdiv(p.OHW); p.fd_ow = make_fastdiv(p.OW);
    p.strided_bytes = (uint32_t)sb; p.dense_bytes = (uint32_t)db;
    const int ci = dgrad ? d->Cout : d->Cin, co = dgrad ? d->Cin : d->Cout;          // of the product
#define EVE_C1S2_CASE(CI, CO, DG)                                                                                                  \
    if (ci == CI && co == CO && dgrad == DG) {                                                                                     \
        using G = C1S2Geom<CI, CO>;                                                                                                \
        const long long batches = (M + G::PIX - 1) / G::PIX;                                                                       \
        long long bpw = batches * G::NSL / 4096;                             /* a wave keeps its filter slice for bpw batches */   \
        bpw = bpw < 1 ? 1 : (bpw > 8 ? 8 : bpw);                                                                                   \
        p.bpw = (uint32_t)bpw;                                                                                                     \
        const long long groups = (batches + bpw - 1) / bpw;                                                                        \
        const unsigned grid = (unsigned)((groups + G::GPB - 1) / G::GPB);                                                          \
        EVE_LAUNCH(EVE_HNAME(H, "conv1x1_s2_stream_kernel<", ", " #CI ", " #CO ", " #DG ">"), (conv1x1_s2_stream_kernel<H, CI, CO, DG>), \
                   dim3(grid), dim3(64 * G::WAVES), 0, s, p, (const H*)in, (const H*)w, (H*)out);                                  \
        return true;                                                                                                               \
    }
    // (256 <-> 512 at 8 x 8 stays on the gather kernel: 30 720 output pixels against a 256 KB filter is a product WITH reuse --
    //  eight waves with 64-channel slices re-read the filter once per 32 pixels and measured 41 / 69 us against its 25 / 34)
    EVE_C1S2_CASE(64, 128, false) EVE_C1S2_CASE(128, 256, false)
    EVE_C1S2_CASE(128, 64, true) EVE_C1S2_CASE(256, 128, true)
#undef EVE_C1S2_CASE
    return false;
}

}  // namespace eve
