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
// NV12, I420 and YUYV captures (eve_screen_area_fmt_to_nchw) have a kernel of the same shape further down.
// Surfaces -- pitched, cropped, NV21 / YV12 / UYVY / P010 / pitched BGRA (eve_screen_area_surface_to_nchw) -- have two behind it.
#include "common.h"
#include "surface.h"
#include "yuv_rgb.h"

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

// ---------------------------------------------------------------------------------------------- NV12 / I420 / YUYV captures
// eve_screen_area_fmt_to_nchw: the same area average of a frame that is converted to RGB pixel by pixel as it is read (yuv_rgb.h),
// CONVERT, THEN AVERAGE -- the clamps make the conversion non-linear.  The shape is screen_u8_area_kernel's: a workgroup per
// (frame, output row), phase 1 sums wy * (R, G, B) per source column into colsum[IW][3], phase 2 applies wx.  In phase 1 a thread
// owns YR_COLS luma columns -- one load per row -- and walks the rows in GROUPS that share chroma: a row pair and the YR_COLS chroma
// bytes under it for NV12 (half of them from each plane for I420), a single row of 2 * YR_COLS bytes for YUYV.  The three chroma
// terms are computed once per sample and group; the 3 * YR_COLS sums stay in registers.  An output row whose range begins on an odd
// source row (1080 / 72 = 15: every second one) gives the first row of its first group weight 0; the chroma row is read by both
// neighbours.  The byte form (a width that is no multiple of YR_COLS, I420 chroma rows of odd length, an unaligned base) gives a
// thread one pixel PAIR and single-byte loads.
// The kernel is bound by its integer work (18.5 VALU instructions per pixel), not by the bytes it reads, so YR_COLS is chosen to
// fill the lanes: 8 columns give a 1920-wide row to 240 of the 256 threads, 16 columns to 120 -- two of the four waves idle, 138 us
// against 106 us for 64 frames of 1080p NV12 (profiles/screen_yuv_notes.md).
// wy <= OH <= IH <= 16 843 009 / 2 (IW >= 2) < 2^24, and the converted value is 8 bits: wy * value is a 24-bit multiply.
// overlap_x: overlap() along a row in 32 bits -- OW <= IW <= 13 653 (one row of sums in LDS), so every product stays below 2^28;
// phase 2's two divisions and its overlaps are per-lane work that costs this kernel time where a read stream hides it.
__device__ __forceinline__ uint32_t overlap_x(const uint32_t i, const uint32_t o, const uint32_t I, const uint32_t O) {
    const uint32_t lo = i * O > o * I ? i * O : o * I;
    const uint32_t hi = (i + 1u) * O < (o + 1u) * I ? (i + 1u) * O : (o + 1u) * I;
    return hi - lo;
}

constexpr int YR_GROUPS = 4;             // chroma groups whose loads one thread keeps in flight (4:2:0: up to eight luma rows)

template <int FMT>
__host__ __device__ constexpr size_t yuv_frame_bytes(const int IH, const int IW) {
    return FMT == EVE_PIX_YUYV ? (size_t)IH * IW * 2 : (size_t)IH * IW / 2 * 3;
}

constexpr int YR_COLS = SURF_VEC_COLS;   // luma columns a thread of the vector form owns (8 or 16); load_words, byte_of: surface.h

// acc[0..2] += wy * (r, g, b) of the pixel with luma Y under chroma c
__device__ __forceinline__ void add_pixel(uint32_t* __restrict__ acc, const uint32_t wy, const int Y, const YuvChroma& c, const YuvCoef& coef) {
    uint32_t rgb[3];
    yuv_pixel<true>(Y, c, coef, rgb);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) acc[ch] += __umul24(wy, rgb[ch]);
}

// FMT: EVE_PIX_NV12, _I420 or _YUYV
template <int FMT, bool VEC>
__global__ __launch_bounds__(SR_THREADS) void screen_area_fmt_kernel(const long long items, const int IH, const int IW, const YuvCoef coef,
                                                                     const uint8_t* __restrict__ src, const int OH, const int OW,
                                                                     float* __restrict__ dst) {
    extern __shared__ __attribute__((aligned(16))) uint32_t colsum[];        // [IW][3]: sum over the rows of wy * (r, g, b)
    constexpr bool PACKED = FMT == EVE_PIX_YUYV;
    constexpr int RPG = PACKED ? 1 : 2;                                      // luma rows per chroma group
    const int tid = threadIdx.x;
    const double area = (double)((long long)IH * IW);
    const float scale = (float)(1.0 / 255.0);
    const size_t luma = (size_t)IH * IW;                                     // 4:2:0: where the chroma begins
    const size_t plane = (size_t)(IH >> 1) * (IW >> 1);                      // I420: from a U sample to its V sample
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const long long n = item / OH;
        const int oy = (int)(item - n * OH);
        const int iy0 = (int)((long long)oy * IH / OH);
        const int iy1 = (int)((((long long)oy + 1) * IH + OH - 1) / OH);      // <= IH
        const int g0 = iy0 / RPG, g1 = (iy1 + RPG - 1) / RPG;                 // <= IH / RPG
        const uint8_t* frame = src + (size_t)n * yuv_frame_bytes<FMT>(IH, IW);
        if (VEC) {
            constexpr int LW = YR_COLS / 4;                                   // dwords of a thread's piece of a luma (or NV12 chroma) row
            for (int v = tid; v < IW / YR_COLS; v += SR_THREADS) {
                uint32_t acc[3 * YR_COLS];
#pragma unroll
                for (int k = 0; k < 3 * YR_COLS; ++k) acc[k] = 0u;
                for (int g = g0; g < g1; g += YR_GROUPS) {
                    uint32_t yq[YR_GROUPS][RPG][PACKED ? 2 * LW : LW];        // 4:2:0: the group's two luma rows; YUYV: Y U Y V per pixel pair
                    uint32_t cq[YR_GROUPS][LW];                               // NV12: YR_COLS / 2 x (U, V); I420: the U bytes, then the V bytes
#pragma unroll
                    for (int i = 0; i < YR_GROUPS; ++i)
                        if (g + i < g1) {
                            if constexpr (PACKED) {
                                load_words(frame + (size_t)(g + i) * IW * 2 + (size_t)v * (2 * YR_COLS), yq[i][0]);
                            } else {
#pragma unroll
                                for (int r = 0; r < 2; ++r) {
                                    const int iy = (g + i) * 2 + r;
                                    if (iy >= iy0 && iy < iy1) {
                                        load_words(frame + (size_t)iy * IW + (size_t)v * YR_COLS, yq[i][r]);
                                    } else {                                  // the other output row's: weight 0 below
#pragma unroll
                                        for (int k = 0; k < LW; ++k) yq[i][r][k] = 0u;
                                    }
                                }
                                if constexpr (FMT == EVE_PIX_NV12) {
                                    load_words(frame + luma + (size_t)(g + i) * IW + (size_t)v * YR_COLS, cq[i]);
                                } else {
                                    const uint8_t* u = frame + luma + (size_t)(g + i) * (IW >> 1) + (size_t)v * (YR_COLS / 2);
                                    uint32_t a[LW / 2], b[LW / 2];
                                    load_words(u, a);
                                    load_words(u + plane, b);
#pragma unroll
                                    for (int k = 0; k < LW / 2; ++k) { cq[i][k] = a[k]; cq[i][LW / 2 + k] = b[k]; }
                                }
                            }
                        }
#pragma unroll
                    for (int i = 0; i < YR_GROUPS; ++i)
                        if (g + i < g1) {
                            if constexpr (PACKED) {
                                const uint32_t wy = overlap(g + i, oy, IH, OH);
#pragma unroll
                                for (int j = 0; j < YR_COLS / 2; ++j) {       // dword j: Y0 U Y1 V of pixels 2j, 2j + 1
                                    const uint32_t w = yq[i][0][j];
                                    const YuvChroma c = yuv_chroma<true>((int)((w >> 8) & 0xffu), (int)(w >> 24), coef);
                                    add_pixel(acc + 6 * j, wy, (int)(w & 0xffu), c, coef);
                                    add_pixel(acc + 6 * j + 3, wy, (int)((w >> 16) & 0xffu), c, coef);
                                }
                            } else {
                                const int iya = (g + i) * 2;
                                // a row of the group outside [iy0, iy1) -- the first of an odd start, the second of an odd end --
                                // belongs to the neighbouring output row: weight 0 (iya < iy1 and iya + 1 >= iy0 always hold here)
                                const uint32_t wa = iya >= iy0 ? overlap(iya, oy, IH, OH) : 0u, wb = iya + 1 < iy1 ? overlap(iya + 1, oy, IH, OH) : 0u;
#pragma unroll
                                for (int j = 0; j < YR_COLS / 2; ++j) {       // chroma sample j: luma columns 2j, 2j + 1 of both rows
                                    const int U = (int)byte_of(cq[i], FMT == EVE_PIX_NV12 ? 2 * j : j);
                                    const int V = (int)byte_of(cq[i], FMT == EVE_PIX_NV12 ? 2 * j + 1 : YR_COLS / 2 + j);
                                    const YuvChroma c = yuv_chroma<true>(U, V, coef);
#pragma unroll
                                    for (int e = 0; e < 2; ++e) {
                                        add_pixel(acc + 3 * (2 * j + e), wa, (int)byte_of(yq[i][0], 2 * j + e), c, coef);
                                        add_pixel(acc + 3 * (2 * j + e), wb, (int)byte_of(yq[i][1], 2 * j + e), c, coef);
                                    }
                                }
                            }
                        }
                }
                uint4* out = reinterpret_cast<uint4*>(colsum + (size_t)v * (3 * YR_COLS));
#pragma unroll
                for (int k = 0; k < 3 * YR_COLS / 4; ++k) out[k] = make_uint4(acc[4 * k], acc[4 * k + 1], acc[4 * k + 2], acc[4 * k + 3]);
            }
        } else {
            for (int p = tid; p < (IW >> 1); p += SR_THREADS) {               // pixel pair p: columns 2p, 2p + 1, one chroma sample
                uint32_t acc[6];
#pragma unroll
                for (int k = 0; k < 6; ++k) acc[k] = 0u;
                for (int g = g0; g < g1; g += YR_GROUPS) {
                    uint32_t yb[YR_GROUPS][RPG][2], ub[YR_GROUPS], vb[YR_GROUPS];
#pragma unroll
                    for (int i = 0; i < YR_GROUPS; ++i)
                        if (g + i < g1) {
                            if constexpr (PACKED) {
                                const uint8_t* q = frame + (size_t)(g + i) * IW * 2 + (size_t)p * 4;
                                yb[i][0][0] = q[0]; ub[i] = q[1]; yb[i][0][1] = q[2]; vb[i] = q[3];
                            } else {
#pragma unroll
                                for (int r = 0; r < RPG; ++r) {
                                    const int iy = (g + i) * 2 + r;
                                    if (iy >= iy0 && iy < iy1) {
                                        const uint8_t* q = frame + (size_t)iy * IW + (size_t)p * 2;
                                        yb[i][r][0] = q[0]; yb[i][r][1] = q[1];
                                    }
                                }
                                if constexpr (FMT == EVE_PIX_NV12) {
                                    const uint8_t* q = frame + luma + (size_t)(g + i) * IW + (size_t)p * 2;
                                    ub[i] = q[0]; vb[i] = q[1];
                                } else {
                                    const uint8_t* q = frame + luma + (size_t)(g + i) * (IW >> 1) + p;
                                    ub[i] = q[0]; vb[i] = q[plane];
                                }
                            }
                        }
#pragma unroll
                    for (int i = 0; i < YR_GROUPS; ++i)
                        if (g + i < g1) {
                            const YuvChroma c = yuv_chroma<true>((int)ub[i], (int)vb[i], coef);
#pragma unroll
                            for (int r = 0; r < RPG; ++r) {
                                const int iy = (g + i) * RPG + r;
                                if (iy >= iy0 && iy < iy1) {
                                    const uint32_t wy = overlap(iy, oy, IH, OH);
                                    add_pixel(acc, wy, (int)yb[i][r][0], c, coef);
                                    add_pixel(acc + 3, wy, (int)yb[i][r][1], c, coef);
                                }
                            }
                        }
                }
#pragma unroll
                for (int k = 0; k < 6; ++k) colsum[(size_t)p * 6 + k] = acc[k];
            }
        }
        __syncthreads();
        for (int t = tid; t < 3 * OW; t += SR_THREADS) {
            const int c = t / OW, ox = t - c * OW;
            const int ix0 = (int)((uint32_t)ox * (uint32_t)IW / (uint32_t)OW);
            const int ix1 = (int)((((uint32_t)ox + 1u) * (uint32_t)IW + (uint32_t)OW - 1u) / (uint32_t)OW);      // <= IW
            uint32_t s = 0u;
            for (int ix = ix0; ix < ix1; ++ix) s += overlap_x(ix, ox, IW, OW) * colsum[ix * 3 + c];
            dst[((n * 3 + c) * OH + oy) * OW + ox] = (float)((double)s / area) * scale;
        }
        __syncthreads();                 // the next item overwrites colsum
    }
}

// ---------------------------------------------------------------------------------------------- surfaces (surface.h)
// eve_screen_area_surface_to_nchw: the same area average of the VISIBLE region of a decoder's or capture API's surface, every
// pixel read through the descriptor's address rule, converted (EVE_SURF_YUV), then averaged.  Shape, LDS and phase 2 are
// screen_area_fmt_kernel's.  Two kernels:
//   yuv420   8-bit 4:2:0 with luma step 1, chroma semi-planar in either order (NV12, NV21) or planar (I420, YV12), any pitches
//            and plane offsets: screen_area_fmt_kernel's phase 1 with the row, plane and frame strides taken from the
//            descriptor.  The vector form loads 8 luma bytes per row and 8 interleaved (or 4 + 4 planar) chroma bytes per row
//            pair; the chroma words are sorted into a U word and a V word after the load, so one instantiation serves the four
//            layouts.  A crop puts pixel (0, 0) `skew` bytes (even, < 8) behind an 8-byte boundary: the thread's eight columns are
//            then the ALIGNED group, 8v - skew .. 8v - skew + 7, and the columns of the first and last group that lie outside
//            the visible region are loaded (they are bytes of the same row of the same frame: the host checks it) but never
//            stored.  The byte form gives a thread one pixel pair and single-byte loads through the address rule.
//   generic  everything else (packed YUV, P010's high bytes, RGB kinds, 4:2:2, 4:4:4): a thread owns one column, three byte loads
//            per pixel, SR_ROWS rows in flight.
struct SurfAreaArgs {
    long long items;
    int IH, IW, OH, OW;
    int yuv;                             // generic: the kind is EVE_SURF_YUV
    int planar;                          // yuv420: U and V in planes of their own (step 1); else interleaved (step 2)
    int skew;                            // yuv420 vector form: bytes from the 8-byte boundary below pixel (0, 0) to it, even
    YuvCoef coef;
    Surf sf;
};

// phase 2 of both kernels: colsum[IW][3] -> the three planes of output row oy of frame n
__device__ __forceinline__ void surf_area_row_out(const uint32_t* colsum, const long long n, const int oy, const int IH, const int IW,
                                                  const int OH, const int OW, float* __restrict__ dst) {
    const double area = (double)((long long)IH * IW);
    const float scale = (float)(1.0 / 255.0);
    for (int t = threadIdx.x; t < 3 * OW; t += SR_THREADS) {
        const int c = t / OW, ox = t - c * OW;
        const int ix0 = (int)((uint32_t)ox * (uint32_t)IW / (uint32_t)OW);
        const int ix1 = (int)((((uint32_t)ox + 1u) * (uint32_t)IW + (uint32_t)OW - 1u) / (uint32_t)OW);      // <= IW
        uint32_t s = 0u;
        for (int ix = ix0; ix < ix1; ++ix) s += overlap_x(ix, ox, IW, OW) * colsum[ix * 3 + c];
        dst[((n * 3 + c) * OH + oy) * OW + ox] = (float)((double)s / area) * scale;
    }
}

template <bool VEC>
__device__ __forceinline__ void surf_area_yuv420_items(const SurfAreaArgs& a, const uint8_t* __restrict__ src, float* __restrict__ dst,
                                                       uint32_t* colsum) {
    const int tid = threadIdx.x;
    const int IH = a.IH, IW = a.IW, OH = a.OH;
    const YuvCoef coef = a.coef;
    const long long oY = a.sf.offset[0], oU = a.sf.offset[1], oV = a.sf.offset[2];
    const long long pY = a.sf.pitch[0], pU = a.sf.pitch[1], pV = a.sf.pitch[2];
    const bool planar = a.planar != 0;
    const bool v_first = oV < oU;                                            // interleaved: NV21's order
    const long long oC = v_first ? oV : oU;                                  // interleaved: where a row's chroma pairs begin
    for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
        const long long n = item / OH;
        const int oy = (int)(item - n * OH);
        const int iy0 = (int)((long long)oy * IH / OH);
        const int iy1 = (int)((((long long)oy + 1) * IH + OH - 1) / OH);      // <= IH
        const int g0 = iy0 / 2, g1 = (iy1 + 1) / 2;                           // row pairs: <= (IH + 1) / 2
        const uint8_t* frame = src + n * a.sf.frame_stride;
        if (VEC) {
            const int skew = a.skew;
            for (int v = tid; v < (skew + IW + YR_COLS - 1) / YR_COLS; v += SR_THREADS) {
                const long long x0 = (long long)v * YR_COLS - skew;           // the group's first column: >= -6, even
                uint32_t acc[3 * YR_COLS];
#pragma unroll
                for (int k = 0; k < 3 * YR_COLS; ++k) acc[k] = 0u;
                for (int g = g0; g < g1; g += YR_GROUPS) {
                    uint32_t yq[YR_GROUPS][2][2];                             // the group's two luma rows, 8 columns each
                    uint32_t cq[YR_GROUPS][2];                                // interleaved: 4 chroma pairs; planar: 4 U bytes, 4 V bytes
#pragma unroll
                    for (int i = 0; i < YR_GROUPS; ++i)
                        if (g + i < g1) {
#pragma unroll
                            for (int r = 0; r < 2; ++r) {
                                const int iy = (g + i) * 2 + r;
                                if (iy >= iy0 && iy < iy1) {
                                    load_words(frame + oY + iy * pY + x0, yq[i][r]);
                                } else {                                      // the other output row's: weight 0 below
                                    yq[i][r][0] = yq[i][r][1] = 0u;
                                }
                            }
                            if (planar) {
                                uint32_t u[1], w[1];
                                load_words(frame + oU + (g + i) * pU + x0 / 2, u);
                                load_words(frame + oV + (g + i) * pV + x0 / 2, w);
                                cq[i][0] = u[0]; cq[i][1] = w[0];
                            } else {
                                load_words(frame + oC + (g + i) * pU + x0, cq[i]);
                            }
                        }
#pragma unroll
                    for (int i = 0; i < YR_GROUPS; ++i)
                        if (g + i < g1) {
                            const int iya = (g + i) * 2;
                            const uint32_t wa = iya >= iy0 ? overlap(iya, oy, IH, OH) : 0u, wb = iya + 1 < iy1 ? overlap(iya + 1, oy, IH, OH) : 0u;
                            const uint32_t even = every_second_byte<false>(cq[i][0], cq[i][1]), odd = every_second_byte<true>(cq[i][0], cq[i][1]);
                            const uint32_t uw = planar ? cq[i][0] : v_first ? odd : even;
                            const uint32_t vw = planar ? cq[i][1] : v_first ? even : odd;
#pragma unroll
                            for (int j = 0; j < YR_COLS / 2; ++j) {           // chroma sample j: luma columns 2j, 2j + 1 of both rows
                                const YuvChroma c = yuv_chroma<true>((int)((uw >> (8 * j)) & 0xffu), (int)((vw >> (8 * j)) & 0xffu), coef);
#pragma unroll
                                for (int e = 0; e < 2; ++e) {
                                    add_pixel(acc + 3 * (2 * j + e), wa, (int)byte_of(yq[i][0], 2 * j + e), c, coef);
                                    add_pixel(acc + 3 * (2 * j + e), wb, (int)byte_of(yq[i][1], 2 * j + e), c, coef);
                                }
                            }
                        }
                }
                if (skew == 0 && x0 + YR_COLS <= IW) {
                    uint4* out = reinterpret_cast<uint4*>(colsum + (size_t)v * (3 * YR_COLS));
#pragma unroll
                    for (int k = 0; k < 3 * YR_COLS / 4; ++k) out[k] = make_uint4(acc[4 * k], acc[4 * k + 1], acc[4 * k + 2], acc[4 * k + 3]);
                } else {                                                      // a skewed or partial group: the visible columns only
#pragma unroll
                    for (int k = 0; k < YR_COLS; ++k)
                        if (x0 + k >= 0 && x0 + k < IW) {
#pragma unroll
                            for (int c = 0; c < 3; ++c) colsum[(x0 + k) * 3 + c] = acc[3 * k + c];
                        }
                }
            }
        } else {
            const long long sY = a.sf.step[0], sU = a.sf.step[1], sV = a.sf.step[2];
            for (int p = tid; p < ((IW + 1) >> 1); p += SR_THREADS) {         // pixel pair p: columns 2p, 2p + 1, one chroma sample
                const bool second = 2 * p + 1 < IW;                           // an odd width's last pair is one column
                uint32_t acc[6];
#pragma unroll
                for (int k = 0; k < 6; ++k) acc[k] = 0u;
                for (int g = g0; g < g1; g += YR_GROUPS) {
                    uint32_t yb[YR_GROUPS][2][2], ub[YR_GROUPS], vb[YR_GROUPS];
#pragma unroll
                    for (int i = 0; i < YR_GROUPS; ++i)
                        if (g + i < g1) {
#pragma unroll
                            for (int r = 0; r < 2; ++r) {
                                const int iy = (g + i) * 2 + r;
                                yb[i][r][0] = yb[i][r][1] = 0u;
                                if (iy >= iy0 && iy < iy1) {
                                    const uint8_t* q = frame + oY + iy * pY + (long long)(2 * p) * sY;
                                    yb[i][r][0] = q[0];
                                    if (second) yb[i][r][1] = q[sY];
                                }
                            }
                            ub[i] = frame[oU + (g + i) * pU + p * sU];
                            vb[i] = frame[oV + (g + i) * pV + p * sV];
                        }
#pragma unroll
                    for (int i = 0; i < YR_GROUPS; ++i)
                        if (g + i < g1) {
                            const YuvChroma c = yuv_chroma<true>((int)ub[i], (int)vb[i], coef);
#pragma unroll
                            for (int r = 0; r < 2; ++r) {
                                const int iy = (g + i) * 2 + r;
                                if (iy >= iy0 && iy < iy1) {
                                    const uint32_t wy = overlap(iy, oy, IH, OH);
                                    add_pixel(acc, wy, (int)yb[i][r][0], c, coef);
                                    add_pixel(acc + 3, wy, (int)yb[i][r][1], c, coef);
                                }
                            }
                        }
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) colsum[(size_t)p * 6 + k] = acc[k];
                if (second) {
#pragma unroll
                    for (int k = 3; k < 6; ++k) colsum[(size_t)p * 6 + k] = acc[k];
                }
            }
        }
        __syncthreads();
        surf_area_row_out(colsum, n, oy, IH, IW, OH, a.OW, dst);
        __syncthreads();                 // the next item overwrites colsum
    }
}

__device__ __forceinline__ void surf_area_generic_items(const SurfAreaArgs& a, const uint8_t* __restrict__ src, float* __restrict__ dst,
                                                        uint32_t* colsum) {
    const int IH = a.IH, IW = a.IW, OH = a.OH;
    const YuvCoef coef = a.coef;
    const Surf sf = a.sf;
    for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
        const long long n = item / OH;
        const int oy = (int)(item - n * OH);
        const int iy0 = (int)((long long)oy * IH / OH);
        const int iy1 = (int)((((long long)oy + 1) * IH + OH - 1) / OH);      // <= IH
        const uint8_t* frame = src + n * sf.frame_stride;
        for (int x = threadIdx.x; x < IW; x += SR_THREADS) {
            uint32_t acc[3] = {0u, 0u, 0u};
            for (int iy = iy0; iy < iy1; iy += SR_ROWS) {
                uint32_t b[SR_ROWS][3];
#pragma unroll
                for (int r = 0; r < SR_ROWS; ++r)
                    if (iy + r < iy1) surf_components(frame, sf, iy + r, x, b[r]);
#pragma unroll
                for (int r = 0; r < SR_ROWS; ++r)
                    if (iy + r < iy1) {
                        const uint32_t wy = overlap(iy + r, oy, IH, OH);
                        uint32_t rgb[3] = {b[r][0], b[r][1], b[r][2]};
                        if (a.yuv) yuv_pixel<true>((int)b[r][0], yuv_chroma<true>((int)b[r][1], (int)b[r][2], coef), coef, rgb);
#pragma unroll
                        for (int c = 0; c < 3; ++c) acc[c] += wy * rgb[c];
                    }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) colsum[(size_t)x * 3 + c] = acc[c];
        }
        __syncthreads();
        surf_area_row_out(colsum, n, oy, IH, IW, OH, a.OW, dst);
        __syncthreads();                 // the next item overwrites colsum
    }
}

constexpr int SURF_YUV420 = 0, SURF_GENERIC = 1;

// FORM: SURF_YUV420 (VEC: its vector form) or SURF_GENERIC (the byte form only)
template <int FORM, bool VEC>
__global__ __launch_bounds__(SR_THREADS) void screen_area_surface_kernel(const SurfAreaArgs a, const uint8_t* __restrict__ src,
                                                                         float* __restrict__ dst) {
    extern __shared__ __attribute__((aligned(16))) uint32_t colsum[];        // [IW][3]: sum over the rows of wy * (r, g, b)
    if constexpr (FORM == SURF_YUV420) surf_area_yuv420_items<VEC>(a, src, dst, colsum);
    else surf_area_generic_items(a, src, dst, colsum);
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

// one launch of screen_area_fmt_kernel<FMT, vec> under its name, "screen_area_fmt_kernel<nv12,true>"
#define SR_FMT_CASE(FMT, fmt)                                                                                                          \
    case FMT:                                                                                                                          \
        if (vec) EVE_LAUNCH("screen_area_fmt_kernel<" fmt ",true>", (screen_area_fmt_kernel<FMT, true>), SR_FMT_ARGS);                \
        else EVE_LAUNCH("screen_area_fmt_kernel<" fmt ",false>", (screen_area_fmt_kernel<FMT, false>), SR_FMT_ARGS);                  \
        break;
#define SR_FMT_ARGS grid, dim3(SR_THREADS), lds, (hipStream_t)stream, items, IH, IW, YUV_MATRICES[matrix], src, OH, OW, dst_nchw

extern "C" int eve_screen_area_fmt_to_nchw(int format, int matrix, long long N, int IH, int IW, const uint8_t* src, int OH, int OW,
                                           float* dst_nchw, eve_stream_t stream) {
    static const char who[] = "screen_area_fmt_to_nchw";
    if (format == EVE_PIX_BGR || format == EVE_PIX_BGRA)
        return screen_u8_area(who, true, N, IH, IW, format == EVE_PIX_BGRA ? 4 : 3, src, OH, OW, dst_nchw, stream);
    char msg[192];
    const char* why = nullptr;
    const size_t lds = (size_t)IW * 3 * sizeof(uint32_t);
    if (N <= 0 || IH <= 0 || IW <= 0 || OH <= 0 || OW <= 0 || !src || !dst_nchw) why = "bad arguments";
    else if (format < EVE_PIX_BGR || format > EVE_PIX_YUYV) why = "unknown format (EVE_PIX_BGR, _BGRA, _NV12, _I420 or _YUYV)";
    else if (matrix < EVE_YUV_BT601 || matrix > EVE_YUV_JFIF) why = "unknown matrix (EVE_YUV_BT601, _BT709 or _JFIF)";
    else if (format != EVE_PIX_YUYV && ((IH | IW) & 1)) why = "IH and IW must be even (2 x 2 chroma blocks)";
    else if (format == EVE_PIX_YUYV && (IW & 1)) why = "IW must be even (chroma pairs)";
    else if (OH > IH || OW > IW) why = "upscaling is not supported (OH <= IH and OW <= IW)";
    else if ((long long)IH * IW > SR_MAX_PIXELS) why = "frame too large (IH * IW <= 16843009 keeps the 32-bit sums exact)";
    else if (lds > (size_t)LDS_CU) why = "row too wide (IW * 12 <= 163840 bytes: one row of three sums per column in LDS)";
    else if (N > (long long)0x7fffffff / OH) why = "N * OH must fit 31 bits";
    if (why) {
        snprintf(msg, sizeof(msg), "%s: %s", who, why);
        return set_error_msg(msg);
    }
    const long long items = N * OH;
    const dim3 grid((unsigned)(items < SR_MAX_BLOCKS ? items : SR_MAX_BLOCKS));
    // then every row, plane and frame starts on YR_COLS bytes (I420 chroma: half of that; a YUYV row on 2 * YR_COLS)
    const bool vec = IW % YR_COLS == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0;
    switch (format) {
        SR_FMT_CASE(EVE_PIX_NV12, "nv12")
        SR_FMT_CASE(EVE_PIX_I420, "i420")
        SR_FMT_CASE(EVE_PIX_YUYV, "yuyv")
    }
    EVE_CHECK_LAUNCH();
    return 0;
}

extern "C" int eve_screen_area_surface_to_nchw(const eve_surface* surface, int matrix, long long N, const uint8_t* src, int OH, int OW,
                                               float* dst_nchw, eve_stream_t stream) {
    static const char who[] = "screen_area_surface_to_nchw";
    char msg[192];
    const char* why = surface_refusal(surface, matrix, N);
    const int IH = why ? 0 : surface->height, IW = why ? 0 : surface->width;
    const size_t lds = (size_t)IW * 3 * sizeof(uint32_t);
    if (why) {}
    else if (N <= 0 || OH <= 0 || OW <= 0 || !src || !dst_nchw) why = "bad arguments";
    else if (OH > IH || OW > IW) why = "upscaling is not supported (OH <= height and OW <= width)";
    else if ((long long)IH * IW > SR_MAX_PIXELS) why = "frame too large (width * height <= 16843009 keeps the 32-bit sums exact)";
    else if (lds > (size_t)LDS_CU) why = "row too wide (width * 12 <= 163840 bytes: one row of three sums per column in LDS)";
    else if (N > (long long)0x7fffffff / OH) why = "N * OH must fit 31 bits";
    if (why) {
        snprintf(msg, sizeof(msg), "%s: %s", who, why);
        return set_error_msg(msg);
    }
    const eve_surface& s = *surface;
    SurfAreaArgs a;
    a.items = N * OH;
    a.IH = IH; a.IW = IW; a.OH = OH; a.OW = OW;
    a.yuv = s.kind == EVE_SURF_YUV;
    a.coef = YUV_MATRICES[a.yuv ? matrix : 0];
    a.sf = surf_of(s);
    // 8-bit 4:2:0 with luma step 1 keeps the wide loads where every load lies on its own size (surface.h surf_form)
    const SurfForm form = surf_form(s, N, src);
    a.planar = form.planar;
    a.skew = form.skew;
    const dim3 grid((unsigned)(a.items < SR_MAX_BLOCKS ? a.items : SR_MAX_BLOCKS));
    if (form.yuv420) {
        const bool vec = form.vec;
        if (vec)
            EVE_LAUNCH("screen_area_surface_kernel<yuv420,true>", (screen_area_surface_kernel<SURF_YUV420, true>), grid, dim3(SR_THREADS), lds,
                       (hipStream_t)stream, a, src, dst_nchw);
        else
            EVE_LAUNCH("screen_area_surface_kernel<yuv420,false>", (screen_area_surface_kernel<SURF_YUV420, false>), grid, dim3(SR_THREADS), lds,
                       (hipStream_t)stream, a, src, dst_nchw);
    } else {
        EVE_LAUNCH("screen_area_surface_kernel<generic,false>", (screen_area_surface_kernel<SURF_GENERIC, false>), grid, dim3(SR_THREADS), lds,
                   (hipStream_t)stream, a, src, dst_nchw);
    }
    EVE_CHECK_LAUNCH();
    return 0;
}
