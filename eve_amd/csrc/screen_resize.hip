// Live screen captures on the device: exact area (box) down-sampling of uint8 N x IH x IW x C frames (C = 3 or 4, a fourth
// channel ignored) to RefineNet's float N x 3 x OH x OW screen input in [0, 1] (include/eve_hip.h eve_screen_u8_area_to_nchw).
//
// Source pixel (iy, ix) and output pixel (oy, ox) overlap by wy * wx, in units of 1 / (OH * OW) source pixels, with
//   wy = |[iy*OH, (iy+1)*OH) n [oy*IH, (oy+1)*IH)|      wx = |[ix*OW, (ix+1)*OW) n [ox*IW, (ox+1)*IW)|
// The sum S = sum wy * wx * v is an integer <= 255 * IH * IW, exact in 32 unsigned bits for IH * IW <= 16 843 009, and
//   y = float(double(S) / double(IH * IW)) * float(1 / 255)
// one correctly rounded double division and one rounded float multiply: no order of summation to agree on, so the result is
// the same bits wherever it is evaluated (tests/screen_resize_ref.py evaluates it in numpy).
//
// The kernel is a read stream (6.2 MB in, 110 KB out per 1080p frame).  A workgroup takes one (frame, output row) at a time:
//   1. each thread owns fixed 16-byte columns of the source rows under the output row and sums wy * byte per byte column in
//      registers (eight rows' loads in flight), then parks the 16 sums in LDS: every source byte is loaded once, by one
//      coalesced 16-byte load -- rows shared by two output rows (fractional ratios only) by both workgroups;
//   2. after one barrier the 3 * OW outputs each take their wx-weighted sum over at most ceil(IW / OW) + 1 LDS entries, divide
//      and store into the three planes.
// A row pitch IW * C that is no multiple of 16 (1366 x 768 x 3), or an unaligned base, takes the byte-column form of step 1:
// thread j owns byte columns j, j + 256, ...; the loads are single bytes, still consecutive across the lanes.
#include "common.h"

namespace eve {
namespace {

constexpr int SR_THREADS = 256;
constexpr int SR_ROWS = 8;               // source rows whose loads one thread keeps in flight
constexpr int SR_MAX_BLOCKS = 4096;      // (frame, output row) items beyond that are taken in a grid-stride loop
constexpr long long SR_MAX_PIXELS = 16843009;     // 255 * IH * IW <= 2^32 - 1

// |[i*O, (i+1)*O) n [o*I, (o+1)*I)| for source index i under output index o (I source / O output pixels along the axis)
__device__ __forceinline__ uint32_t overlap(long long i, long long o, long long I, long long O) {
    const long long lo = i * O > o * I ? i * O : o * I;
    const long long hi = (i + 1) * O < (o + 1) * I ? (i + 1) * O : (o + 1) * I;
    return (uint32_t)(hi - lo);
}

// BGR: output plane c reads source channel 2 - c (eve_screen_u8_area_bgr_to_nchw); nothing else differs
template <bool VEC, bool BGR = false>
__global__ __launch_bounds__(SR_THREADS) void screen_u8_area_kernel(const long long items, const int IH, const int IW, const int C,
                                                                    const uint8_t* __restrict__ src, const int OH, const int OW,
                                                                    float* __restrict__ dst) {
    extern __shared__ __attribute__((aligned(16))) uint32_t colsum[];        // [IW * C]: sum over the rows of wy * byte
    const int tid = threadIdx.x;
    const int pitch = IW * C;
    const double area = (double)((long long)IH * IW);
    const float scale = (float)(1.0 / 255.0);
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const long long n = item / OH;
        const int oy = (int)(item - n * OH);
        const int iy0 = (int)((long long)oy * IH / OH);
        const int iy1 = (int)((((long long)oy + 1) * IH + OH - 1) / OH);      // <= IH
        const uint8_t* frame = src + (size_t)n * IH * pitch;
        if (VEC) {
            const int nvec = pitch >> 4;
            for (int v = tid; v < nvec; v += SR_THREADS) {
                uint32_t acc[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) acc[k] = 0u;
                for (int iy = iy0; iy < iy1; iy += SR_ROWS) {
                    uint4 q[SR_ROWS];
#pragma unroll
                    for (int r = 0; r < SR_ROWS; ++r)
                        if (iy + r < iy1) q[r] = *reinterpret_cast<const uint4*>(frame + (size_t)(iy + r) * pitch + (size_t)v * 16);
#pragma unroll
                    for (int r = 0; r < SR_ROWS; ++r)
                        if (iy + r < iy1) {
                            const uint32_t wy = overlap(iy + r, oy, IH, OH);
                            const uint32_t w[4] = {q[r].x, q[r].y, q[r].z, q[r].w};
#pragma unroll
                            for (int k = 0; k < 16; ++k) acc[k] += wy * ((w[k >> 2] >> (8 * (k & 3))) & 0xffu);
                        }
                }
                uint4* out = reinterpret_cast<uint4*>(colsum + (size_t)v * 16);
#pragma unroll
                for (int k = 0; k < 4; ++k) out[k] = make_uint4(acc[4 * k], acc[4 * k + 1], acc[4 * k + 2], acc[4 * k + 3]);
            }
        } else {
            for (int j = tid; j < pitch; j += SR_THREADS) {
                uint32_t acc = 0u;
                for (int iy = iy0; iy < iy1; iy += SR_ROWS) {
                    uint32_t b[SR_ROWS];
#pragma unroll
                    for (int r = 0; r < SR_ROWS; ++r)
                        if (iy + r < iy1) b[r] = frame[(size_t)(iy + r) * pitch + j];
#pragma unroll
                    for (int r = 0; r < SR_ROWS; ++r)
                        if (iy + r < iy1) acc += overlap(iy + r, oy, IH, OH) * b[r];
                }
                colsum[j] = acc;
            }
        }
        __syncthreads();
        for (int t = tid; t < 3 * OW; t += SR_THREADS) {
            const int c = t / OW, ox = t - c * OW;
            const int ix0 = (int)((long long)ox * IW / OW);
            const int ix1 = (int)((((long long)ox + 1) * IW + OW - 1) / OW);  // <= IW
            uint32_t s = 0u;
            for (int ix = ix0; ix < ix1; ++ix) s += overlap(ix, ox, IW, OW) * colsum[(size_t)ix * C + (BGR ? 2 - c : c)];
            dst[((n * 3 + c) * OH + oy) * OW + ox] = (float)((double)s / area) * scale;
        }
        __syncthreads();                 // the next item overwrites colsum
    }
}

}  // namespace
}  // namespace eve

using namespace eve;

// both entry points; `who` names the caller in a refusal
static int screen_u8_area(const char* who, bool bgr, long long N, int IH, int IW, int C, const uint8_t* src_nhwc, int OH, int OW,
                          float* dst_nchw, eve_stream_t stream) {
    char msg[192];
    const char* why = nullptr;
    const long long pitch = (long long)IW * C;
    const size_t lds = (size_t)pitch * sizeof(uint32_t);
    if (N <= 0 || IH <= 0 || IW <= 0 || OH <= 0 || OW <= 0 || !src_nhwc || !dst_nchw) why = "bad arguments";
    else if (C != 3 && C != 4) why = "C must be 3 or 4 (a fourth channel is ignored)";
    else if (OH > IH || OW > IW) why = "upscaling is not supported (OH <= IH and OW <= IW)";
    else if ((long long)IH * IW > SR_MAX_PIXELS) why = "frame too large (IH * IW <= 16843009 keeps the 32-bit sums exact)";
    else if (lds > (size_t)LDS_CU) why = "row too wide (IW * C <= 40960 bytes: one row of sums in LDS)";
    else if (N > (long long)0x7fffffff / OH) why = "N * OH must fit 31 bits";
    if (why) {
        snprintf(msg, sizeof(msg), "%s: %s", who, why);
        return set_error_msg(msg);
    }
    const long long items = N * OH;
    const dim3 grid((unsigned)(items < SR_MAX_BLOCKS ? items : SR_MAX_BLOCKS));
    const bool vec = pitch % 16 == 0 && (reinterpret_cast<uintptr_t>(src_nhwc) & 15) == 0;
    if (bgr) {
        if (vec)
            EVE_LAUNCH("screen_u8_area_bgr_kernel<true>", (screen_u8_area_kernel<true, true>), grid, dim3(SR_THREADS), lds, (hipStream_t)stream,
                       items, IH, IW, C, src_nhwc, OH, OW, dst_nchw);
        else
            EVE_LAUNCH("screen_u8_area_bgr_kernel<false>", (screen_u8_area_kernel<false, true>), grid, dim3(SR_THREADS), lds, (hipStream_t)stream,
                       items, IH, IW, C, src_nhwc, OH, OW, dst_nchw);
    } else if (vec)
        EVE_LAUNCH("screen_u8_area_kernel<true>", screen_u8_area_kernel<true>, grid, dim3(SR_THREADS), lds, (hipStream_t)stream, items, IH, IW,
                   C, src_nhwc, OH, OW, dst_nchw);
    else
        EVE_LAUNCH("screen_u8_area_kernel<false>", screen_u8_area_kernel<false>, grid, dim3(SR_THREADS), lds, (hipStream_t)stream, items, IH,
                   IW, C, src_nhwc, OH, OW, dst_nchw);
    EVE_CHECK_LAUNCH();
    return 0;
}

extern "C" int eve_screen_u8_area_to_nchw(long long N, int IH, int IW, int C, const uint8_t* src_nhwc, int OH, int OW, float* dst_nchw,
                                          eve_stream_t stream) {
    return screen_u8_area("screen_u8_area_to_nchw", false, N, IH, IW, C, src_nhwc, OH, OW, dst_nchw, stream);
}

extern "C" int eve_screen_u8_area_bgr_to_nchw(long long N, int IH, int IW, int C, const uint8_t* src_nhwc, int OH, int OW, float* dst_nchw,
                                              eve_stream_t stream) {
    return screen_u8_area("screen_u8_area_bgr_to_nchw", true, N, IH, IW, C, src_nhwc, OH, OW, dst_nchw, stream);
}
