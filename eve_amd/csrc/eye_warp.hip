// Live camera frames on the device: the two eye patches cut from whole uint8 N x IH x IW x C frames (C = 3 or 4, a fourth channel
// ignored) through one 3 x 3 homography per frame, sampled bilinearly and normalised as the reference normalises its pre-cut
// patches (datasources/eve_sequences.py:196-203).  The contract is in include/eve_hip.h (eve_eye_warp_u8_to_nchw) and in numpy in
// tests/eye_warp_ref.py; in short, for output pixel (oy, ox) of patch n with matrix m = warps[n] (patch pixel -> camera pixel):
//   X = (m00*ox + m01*oy) + m02,  Y = (m10*ox + m11*oy) + m12,  Wd = (m20*ox + m21*oy) + m22     in float64
//   u = X / Wd, v = Y / Wd                                      correctly rounded float64 divisions
//   inside  iff  Wd > 0 && u > -1 && u < IW && v > -1 && v < IH                   (a NaN fails every comparison)
//   fu = floor(u*256 + 0.5), x0 = fu >> 8, ax = fu & 255; the same for v          8 fractional bits per axis
//   S  = (256-ax)(256-ay) p00 + ax(256-ay) p01 + (256-ax)ay p10 + ax ay p11       taps outside the frame read 0; S = 0 outside
//   out = float(S) * 2^-16 * float(2/255) + (-1.0f)                               one rounded multiply, one rounded add
// Every product m * o is exact in float64 (24 bits by at most 13), so a fused multiply-add changes nothing as long as the
// association stays; the coordinate of a pixel is computed from (oy, ox) alone, never stepped along the row.
//
// The lens variant (eve_eye_warp_lens_u8_to_nchw / _to_stem, tests/eye_warp_lens_ref.py) takes raw frames of a camera with lens
// distortion: (u, v) is then a pixel of the UNDISTORTED image, and one row L = (fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6) per
// patch -- OpenCV's pinhole + radial / tangential / rational model -- carries it to the raw frame before the taps are read:
//   x = (u - cx) / fx, y = (v - cy) / fy, xx = x*x, yy = y*y, xy = x*y, r2 = xx + yy, a = xy + xy
//   rad = (((k3*r2 + k2)*r2 + k1)*r2 + 1) / (((k6*r2 + k5)*r2 + k4)*r2 + 1)          den, the divisor, must be > 0
//   xd = (x*rad + p1*a) + p2*(r2 + (xx + xx)),  yd = (y*rad + p1*(r2 + (yy + yy))) + p2*a,  ud = fx*xd + cx,  vd = fy*yd + cy
// in float64, every operation rounded on its own (no contraction: these products are not exact); (ud, vd) then stands where (u, v)
// stands above.  A row whose eight coefficients are all zero takes the plain arithmetic (fx*((u - cx)/fx) + cx is not u): the
// decision is uniform over the patch, so over the workgroup's item.  No undistorted frame ever exists.
//
// The kernel is a gather stream: a 128 x 128 patch touches 12 bytes per output pixel and channel triple, 197 KB of loads for
// 196 KB (float) or 147 KB (packed) of stores, out of a frame region the L2 holds.  A workgroup takes one (patch, band of EW_BAND
// output rows) at a time with its lanes along ox: neighbouring lanes read neighbouring source bytes (as far as the warp keeps
// neighbours together) and their stores are consecutive -- 4 bytes per lane and plane for the float form, one 8-byte pixel per
// lane for the stem's packed form, whose rows include the pad ring, written as zeros by the same loop.  The nine matrix entries
// are uniform over the workgroup.  The taps are single-byte loads, so `frames` needs no alignment.
//
// The format variant (eve_eye_warp_fmt_to_nchw / _to_stem, tests/pixel_format_ref.py) takes the frames as cameras and decoders
// deliver them -- BGR(A), NV12, I420, YUYV -- and converts ONLY the four taps of an output pixel, in the same launch: tap_rgb<FMT>
// stands where the three byte loads of the RGB tap stand, everything before it (coordinates, lens) and behind it (weights, blend,
// warp_value, layouts) is the same code.  A YUV tap is three single-byte loads (luma, and the nearest chroma sample of its 2 x 2
// block or pair) and the integer matrix of include/eve_hip.h; a tap outside the frame adds nothing, as before.  The plain
// kernels are the FMT = PIX_RGB instantiation of the same templates and compile to the instructions they had without them.
//
// The surface variant (eve_eye_warp_surface_to_nchw / _to_stem, surface.h, tests/surface_ref.py) takes the frames as a decoder or a
// capture API leaves them in memory -- rows with a pitch, coded rows, aligned planes, a crop; NV21, YV12, UYVY, P010's high bytes,
// pitched BGRA -- through the descriptor's address rule: where tap_rgb<FMT> stands, three byte loads at
// offset[c] + (y >> ys) * pitch[c] + (x >> xs) * step[c] in 64-bit arithmetic (surf_tap_terms: a row term and a column term per
// component, shared by the four taps), the descriptor by value in the kernel's arguments.
// The two surface codes are two more values of FMT; the kernels above keep their instructions (compared in the assembly).
#include "common.h"
#include "surface.h"
#include "yuv_rgb.h"

namespace eve {
namespace {

constexpr int EW_THREADS = 256;
constexpr int EW_BAND = 2;               // output rows per item: 256 lanes cover two rows of a 128-wide patch
constexpr int EW_MAX_BLOCKS = 1024;      // (patch, band) items beyond that are taken in a grid-stride loop
constexpr int EW_MAX_FRAME = 16384;      // IH, IW: the fixed-point coordinate stays below 2^22
constexpr int EW_MAX_PATCH = 4096;       // OH, OW: m * o is exact in float64 with room to spare

struct EyeWarpArgs {
    long long items;                     // N * bands
    int bands;                           // bands per patch
    int IH, IW, C, OH, OW;
};

// what a frame holds (EVE_PIX_* of include/eve_hip.h; PIX_RGB is the four existing entry points' layout, C = 3 or 4)
constexpr int PIX_RGB = -1;
// a surface (surface.h): the taps go through the descriptor's address rule; components R, G, B or Y, U, V
constexpr int PIX_SURF_RGB = -2, PIX_SURF_YUV = -3;
constexpr bool is_surface(const int FMT) { return FMT == PIX_SURF_RGB || FMT == PIX_SURF_YUV; }

struct EyeWarpFmtArgs {
    EyeWarpArgs a;                       // a.C: 3, or 4 for BGRA; the YUV formats do not read it
    YuvCoef coef;                        // the integer YUV -> RGB matrix of the launch (yuv_rgb.h; unused by the BGR formats)
};

// bytes of one frame
template <int FMT>
__device__ __forceinline__ size_t frame_bytes(const int IH, const int IW, const int C) {
    if constexpr (FMT == EVE_PIX_NV12 || FMT == EVE_PIX_I420) return (size_t)IH * IW / 2 * 3;
    else if constexpr (FMT == EVE_PIX_YUYV) return (size_t)IH * IW * 2;
    else return (size_t)IH * IW * C;
}

// the 8-bit (r, g, b) of pixel (y, x), 0 <= y < IH, 0 <= x < IW, of one frame: single-byte loads, chroma the nearest sample
template <int FMT>
__device__ __forceinline__ void tap_rgb(const uint8_t* __restrict__ frame, const int IH, const int IW, const int y, const int x,
                                        const YuvCoef& k, uint32_t (&rgb)[3]) {
    if constexpr (FMT == EVE_PIX_BGR || FMT == EVE_PIX_BGRA) {
        const uint8_t* p = frame + ((size_t)y * IW + x) * (FMT == EVE_PIX_BGRA ? 4 : 3);
        rgb[0] = p[2]; rgb[1] = p[1]; rgb[2] = p[0];
    } else {
        int Y, U, V;
        if constexpr (FMT == EVE_PIX_NV12) {
            const uint8_t* c = frame + (size_t)IH * IW + (size_t)(y >> 1) * IW + (x & ~1);
            Y = frame[(size_t)y * IW + x]; U = c[0]; V = c[1];
        } else if constexpr (FMT == EVE_PIX_I420) {
            const size_t plane = (size_t)(IH >> 1) * (IW >> 1);
            const uint8_t* c = frame + (size_t)IH * IW + (size_t)(y >> 1) * (IW >> 1) + (x >> 1);
            Y = frame[(size_t)y * IW + x]; U = c[0]; V = c[plane];
        } else {                         // YUYV: Y0 U Y1 V per pixel pair
            const uint8_t* row = frame + (size_t)y * IW * 2;
            Y = row[2 * x]; U = row[2 * (x & ~1) + 1]; V = row[2 * (x | 1) + 1];
        }
        yuv_to_rgb(Y, U, V, k, rgb);
    }
}

// one patch's camera model, widened to float64; `on` is false for a row whose eight coefficients are all +-0 (a NaN is not zero)
struct Lens {
    double fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6;
    bool on;
};

__device__ __forceinline__ Lens load_lens(const float* __restrict__ row) {
    Lens L;
    L.fx = (double)row[0]; L.fy = (double)row[1]; L.cx = (double)row[2]; L.cy = (double)row[3];
    L.k1 = (double)row[4]; L.k2 = (double)row[5]; L.p1 = (double)row[6]; L.p2 = (double)row[7];
    L.k3 = (double)row[8]; L.k4 = (double)row[9]; L.k5 = (double)row[10]; L.k6 = (double)row[11];
    bool zero = true;
#pragma unroll
    for (int i = 4; i < 12; ++i) zero = zero && row[i] == 0.0f;
    L.on = !zero;
    return L;
}

// the three channels' fixed-point sums S (<= 255 * 65536) of output pixel (oy, ox); all zero outside.  LENS: (u, v) goes through
// the distortion model of L first, unless L.on is false.  FMT: the taps come through tap_rgb<FMT> (coef: its matrix), or through
// the address terms of the descriptor sf for the two surface codes.
template <bool LENS, int FMT = PIX_RGB>
__device__ __forceinline__ void warp_sums(const double (&m)[9], const Lens& L, const uint8_t* __restrict__ frame, const int IH, const int IW,
                                          const int C, const int oy, const int ox, uint32_t (&S)[3], const YuvCoef& coef = YuvCoef(),
                                          const Surf& sf = Surf()) {
#pragma clang fp contract(off)
    const double dx = (double)ox, dy = (double)oy;
    const double X = (m[0] * dx + m[1] * dy) + m[2];
    const double Y = (m[3] * dx + m[4] * dy) + m[5];
    const double Wd = (m[6] * dx + m[7] * dy) + m[8];
    double u = X / Wd, v = Y / Wd;
    bool pole = false;                                   // at or beyond the rational model's pole, where rad changes sign
    if constexpr (LENS) {
        if (L.on) {
            const double x = (u - L.cx) / L.fx, y = (v - L.cy) / L.fy;
            const double xx = x * x, yy = y * y, xy = x * y;
            const double r2 = xx + yy;
            const double num = ((L.k3 * r2 + L.k2) * r2 + L.k1) * r2 + 1.0;
            const double den = ((L.k6 * r2 + L.k5) * r2 + L.k4) * r2 + 1.0;
            const double rad = num / den, a = xy + xy;
            const double xd = (x * rad + L.p1 * a) + L.p2 * (r2 + (xx + xx));
            const double yd = (y * rad + L.p1 * (r2 + (yy + yy))) + L.p2 * a;
            u = L.fx * xd + L.cx;
            v = L.fy * yd + L.cy;
            pole = !(den > 0.0);
        }
    }
    S[0] = S[1] = S[2] = 0u;
    if (!(Wd > 0.0 && u > -1.0 && u < (double)IW && v > -1.0 && v < (double)IH) || pole) return;
    const int fu = (int)floor(u * 256.0 + 0.5), fv = (int)floor(v * 256.0 + 0.5);      // in [-256, 256 * 16384]
    const int x0 = fu >> 8, y0 = fv >> 8;                                              // in [-1, IW] / [-1, IH]
    const uint32_t ax = (uint32_t)(fu & 255), ay = (uint32_t)(fv & 255);
    const uint32_t w[4] = {(256u - ax) * (256u - ay), ax * (256u - ay), (256u - ax) * ay, ax * ay};
    long long row[2][3], col[2][3];                      // a surface's address terms, shared by the four taps
    if constexpr (is_surface(FMT)) surf_tap_terms<FMT == PIX_SURF_YUV>(sf, y0, x0, row, col);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int y = y0 + (t >> 1), x = x0 + (t & 1);
        if (y >= 0 && y < IH && x >= 0 && x < IW) {
            if constexpr (FMT == PIX_RGB) {
                const uint8_t* p = frame + ((size_t)y * IW + x) * C;
#pragma unroll
                for (int c = 0; c < 3; ++c) S[c] += w[t] * (uint32_t)p[c];
            } else if constexpr (is_surface(FMT)) {
                uint32_t rgb[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) rgb[c] = frame[row[t >> 1][c] + col[t & 1][c]];
                if constexpr (FMT == PIX_SURF_YUV) yuv_to_rgb((int)rgb[0], (int)rgb[1], (int)rgb[2], coef, rgb);
#pragma unroll
                for (int c = 0; c < 3; ++c) S[c] += w[t] * rgb[c];
            } else {
                uint32_t rgb[3];
                tap_rgb<FMT>(frame, IH, IW, y, x, coef, rgb);
#pragma unroll
                for (int c = 0; c < 3; ++c) S[c] += w[t] * rgb[c];
            }
        }
    }
}

__device__ __forceinline__ float warp_value(uint32_t S) {
#pragma clang fp contract(off)          // as normalise_u8 (stem_conv.hip): the multiply and the add round separately
    const float val = (float)S * 0x1p-16f;                  // exact: S < 2^24
    const float f = val * (float)(2.0 / 255.0);
    return f + (-1.0f);
}

// O = float: dst is float [N][3][OH][OW].  O = bf16_t / f16_t: dst is the stem's packed [N][OH+6][OW+8][4], pixel at (y+3, x+4).
// LENS: lens is float [N][12], read once per item like the matrix.  The body of both kernels.  Keep the pointers plain here (the
// kernels' own parameters carry __restrict__) and the arguments by value: qualified pointers or a reference make the compiler
// schedule the plain kernels differently from a kernel that holds this loop itself.
template <typename O, bool LENS, int FMT = PIX_RGB>
__device__ __forceinline__ void eye_warp_items(const EyeWarpArgs a, const uint8_t* src, const float* warps, const float* lens, void* dst,
                                               const YuvCoef coef = YuvCoef(), const Surf sf = Surf()) {
    constexpr bool PACKED = !std::is_same<O, float>::value;
    const int rows = PACKED ? a.OH + 6 : a.OH, cols = PACKED ? a.OW + 8 : a.OW;      // of the output image, pad ring included
    for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
        const long long n = item / a.bands;
        const int r0 = (int)(item - n * a.bands) * EW_BAND;
        const int nr = rows - r0 < EW_BAND ? rows - r0 : EW_BAND;
        double m[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) m[i] = (double)warps[n * 9 + i];
        Lens L = {};
        if constexpr (LENS) L = load_lens(lens + n * 12);
        const uint8_t* frame;
        if constexpr (is_surface(FMT)) frame = src + n * sf.frame_stride;
        else frame = src + (FMT == PIX_RGB ? (size_t)n * a.IH * a.IW * a.C : (size_t)n * frame_bytes<FMT>(a.IH, a.IW, a.C));
        for (int t = threadIdx.x; t < nr * cols; t += EW_THREADS) {
            const int r = r0 + t / cols, col = t % cols;
            const int oy = PACKED ? r - 3 : r, ox = PACKED ? col - 4 : col;
            const bool pixel = !PACKED || (oy >= 0 && oy < a.OH && ox >= 0 && ox < a.OW);
            uint32_t S[3] = {0u, 0u, 0u};
            if (pixel) warp_sums<LENS, FMT>(m, L, frame, a.IH, a.IW, a.C, oy, ox, S, coef, sf);
            if constexpr (PACKED) {
                uint2 q = make_uint2(0u, 0u);
                if (pixel) {
                    q.x = Elem<O>::pack2(warp_value(S[0]), warp_value(S[1]));
                    q.y = Elem<O>::pack2(warp_value(S[2]), 0.f);
                }
                reinterpret_cast<uint2*>(dst)[((size_t)n * rows + r) * cols + col] = q;
            } else {
                float* out = reinterpret_cast<float*>(dst) + ((size_t)n * 3 * rows + r) * cols + col;
#pragma unroll
                for (int c = 0; c < 3; ++c) out[(size_t)c * rows * cols] = warp_value(S[c]);
            }
        }
    }
}

template <typename O>
__global__ __launch_bounds__(EW_THREADS) void eye_warp_u8_kernel(const EyeWarpArgs a, const uint8_t* __restrict__ src,
                                                                 const float* __restrict__ warps, void* __restrict__ dst) {
    eye_warp_items<O, false>(a, src, warps, nullptr, dst);
}

template <typename O>
__global__ __launch_bounds__(EW_THREADS) void eye_warp_lens_u8_kernel(const EyeWarpArgs a, const uint8_t* __restrict__ src,
                                                                      const float* __restrict__ warps, const float* __restrict__ lens,
                                                                      void* __restrict__ dst) {
    eye_warp_items<O, true>(a, src, warps, lens, dst);
}

// FMT: one of EVE_PIX_*; lens is read only with LENS
template <int FMT, bool LENS, typename O>
__global__ __launch_bounds__(EW_THREADS) void eye_warp_fmt_kernel(const EyeWarpFmtArgs fa, const uint8_t* __restrict__ src,
                                                                  const float* __restrict__ warps, const float* __restrict__ lens,
                                                                  void* __restrict__ dst) {
    eye_warp_items<O, LENS, FMT>(fa.a, src, warps, lens, dst, fa.coef);
}

// YUV: the surface's kind; sa.a.IH x sa.a.IW is its visible region; lens is read only with LENS
struct EyeWarpSurfArgs {
    EyeWarpArgs a;
    YuvCoef coef;
    Surf sf;
};

template <bool YUV, bool LENS, typename O>
__global__ __launch_bounds__(EW_THREADS) void eye_warp_surface_kernel(const EyeWarpSurfArgs sa, const uint8_t* __restrict__ src,
                                                                      const float* __restrict__ warps, const float* __restrict__ lens,
                                                                      void* __restrict__ dst) {
    eye_warp_items<O, LENS, YUV ? PIX_SURF_YUV : PIX_SURF_RGB>(sa.a, src, warps, lens, dst, sa.coef, sa.sf);
}

// the checks the entry points share; -> nullptr or what is wrong
const char* eye_warp_refusal(long long N, int IH, int IW, int C, const void* frames, const void* warps, int OH, int OW, const void* dst) {
    if (N <= 0 || IH <= 0 || IW <= 0 || OH <= 0 || OW <= 0 || !frames || !warps || !dst) return "bad arguments";
    if (C != 3 && C != 4) return "C must be 3 or 4 (a fourth channel is ignored)";
    if (IH > EW_MAX_FRAME || IW > EW_MAX_FRAME) return "frame too large (IH and IW <= 16384)";
    if (OH > EW_MAX_PATCH || OW > EW_MAX_PATCH) return "patch too large (OH and OW <= 4096)";
    if (N > (long long)0x7fffffff / (OH + 6)) return "N * (OH + 6) must fit 31 bits";
    return nullptr;
}

EyeWarpArgs eye_warp_args(long long N, int IH, int IW, int C, int OH, int OW, int rows) {
    EyeWarpArgs a;
    a.bands = (rows + EW_BAND - 1) / EW_BAND;
    a.items = N * a.bands;
    a.IH = IH; a.IW = IW; a.C = C; a.OH = OH; a.OW = OW;
    return a;
}

// the format entry points' checks on top of eye_warp_refusal; -> nullptr or what is wrong
const char* eye_warp_fmt_refusal(int format, int matrix, long long N, int IH, int IW, const void* frames, const void* warps, int OH, int OW,
                                 const void* dst) {
    if (format < EVE_PIX_BGR || format > EVE_PIX_YUYV) return "unknown format (EVE_PIX_BGR, _BGRA, _NV12, _I420 or _YUYV)";
    const bool yuv = format != EVE_PIX_BGR && format != EVE_PIX_BGRA;
    if (yuv && (matrix < EVE_YUV_BT601 || matrix > EVE_YUV_JFIF)) return "unknown matrix (EVE_YUV_BT601, _BT709 or _JFIF)";
    if (const char* why = eye_warp_refusal(N, IH, IW, format == EVE_PIX_BGRA ? 4 : 3, frames, warps, OH, OW, dst)) return why;
    if ((format == EVE_PIX_NV12 || format == EVE_PIX_I420) && ((IH | IW) & 1)) return "IH and IW must be even (2 x 2 chroma blocks)";
    if (format == EVE_PIX_YUYV && (IW & 1)) return "IW must be even (chroma pairs)";
    return nullptr;
}

EyeWarpFmtArgs eye_warp_fmt_args(int format, int matrix, long long N, int IH, int IW, int OH, int OW, int rows) {
    EyeWarpFmtArgs fa;
    fa.a = eye_warp_args(N, IH, IW, format == EVE_PIX_BGRA ? 4 : 3, OH, OW, rows);
    fa.coef = YUV_MATRICES[format == EVE_PIX_BGR || format == EVE_PIX_BGRA ? 0 : matrix];
    return fa;
}

// one launch of eye_warp_fmt_kernel<FMT, lens != NULL, O> under its name, "eye_warp_fmt_kernel<nv12,lens,eve::bf16_t>"
#define EW_FMT_NAME(fmt, lens, O) "eye_warp_fmt_kernel<" fmt "," lens "," O ">"
#define EW_FMT_CASE(FMT, fmt)                                                                                                      \
    case FMT:                                                                                                                      \
        if (lens) {                                                                                                                \
            if (dtype == EVE_DT_F32) EVE_LAUNCH(EW_FMT_NAME(fmt, "lens", "float"), (eye_warp_fmt_kernel<FMT, true, float>), EW_FMT_ARGS);   \
            else if (dtype == EVE_DT_BF16) EVE_LAUNCH(EW_FMT_NAME(fmt, "lens", "eve::bf16_t"), (eye_warp_fmt_kernel<FMT, true, bf16_t>), EW_FMT_ARGS); \
            else EVE_LAUNCH(EW_FMT_NAME(fmt, "lens", "eve::f16_t"), (eye_warp_fmt_kernel<FMT, true, f16_t>), EW_FMT_ARGS);         \
        } else {                                                                                                                   \
            if (dtype == EVE_DT_F32) EVE_LAUNCH(EW_FMT_NAME(fmt, "plain", "float"), (eye_warp_fmt_kernel<FMT, false, float>), EW_FMT_ARGS); \
            else if (dtype == EVE_DT_BF16) EVE_LAUNCH(EW_FMT_NAME(fmt, "plain", "eve::bf16_t"), (eye_warp_fmt_kernel<FMT, false, bf16_t>), EW_FMT_ARGS); \
            else EVE_LAUNCH(EW_FMT_NAME(fmt, "plain", "eve::f16_t"), (eye_warp_fmt_kernel<FMT, false, f16_t>), EW_FMT_ARGS);       \
        }                                                                                                                          \
        break;
#define EW_FMT_ARGS grid, dim3(EW_THREADS), 0, stream, fa, frames, warps, lens, dst

// dtype: EVE_DT_F32 for the float form (rows = OH), EVE_DT_BF16 / EVE_DT_F16 for the packed one (rows = OH + 6)
void eye_warp_fmt_launch(int dtype, int format, const EyeWarpFmtArgs& fa, const uint8_t* frames, const float* warps, const float* lens,
                         void* dst, hipStream_t stream) {
    const dim3 grid((unsigned)(fa.a.items < EW_MAX_BLOCKS ? fa.a.items : EW_MAX_BLOCKS));
    switch (format) {
        EW_FMT_CASE(EVE_PIX_BGR, "bgr")
        EW_FMT_CASE(EVE_PIX_BGRA, "bgra")
        EW_FMT_CASE(EVE_PIX_NV12, "nv12")
        EW_FMT_CASE(EVE_PIX_I420, "i420")
        EW_FMT_CASE(EVE_PIX_YUYV, "yuyv")
    }
}

// one launch of eye_warp_surface_kernel<kind == YUV, lens != NULL, O> under its name, "eye_warp_surface_kernel<yuv,plain,float>"
#define EW_SURF_NAME(kind, lens, O) "eye_warp_surface_kernel<" kind "," lens "," O ">"
#define EW_SURF_ARGS grid, dim3(EW_THREADS), 0, stream, sa, frames, warps, lens, dst
#define EW_SURF_CASE(YUV, kind, LENS, lname)                                                                                       \
    if (dtype == EVE_DT_F32) EVE_LAUNCH(EW_SURF_NAME(kind, lname, "float"), (eye_warp_surface_kernel<YUV, LENS, float>), EW_SURF_ARGS);            \
    else if (dtype == EVE_DT_BF16) EVE_LAUNCH(EW_SURF_NAME(kind, lname, "eve::bf16_t"), (eye_warp_surface_kernel<YUV, LENS, bf16_t>), EW_SURF_ARGS); \
    else EVE_LAUNCH(EW_SURF_NAME(kind, lname, "eve::f16_t"), (eye_warp_surface_kernel<YUV, LENS, f16_t>), EW_SURF_ARGS);

// both surface entry points behind their checks: dtype EVE_DT_F32 is the float form, the other two the packed one
int eye_warp_surface(const char* who, int dtype, bool packed, const eve_surface* surface, int matrix, long long N, const uint8_t* frames,
                     const float* warps, const float* lens, int OH, int OW, void* dst, hipStream_t stream) {
    char msg[192];
    const char* why = surface_refusal(surface, matrix, N);
    if (!why) why = eye_warp_refusal(N, surface->height, surface->width, 3, frames, warps, OH, OW, dst);
    if (!why && packed && dtype != EVE_DT_BF16 && dtype != EVE_DT_F16) why = "dtype must be bf16 or f16 (the stem's packed input)";
    if (why) {
        snprintf(msg, sizeof(msg), "%s: %s", who, why);
        return set_error_msg(msg);
    }
    const bool yuv = surface->kind == EVE_SURF_YUV;
    EyeWarpSurfArgs sa;
    sa.a = eye_warp_args(N, surface->height, surface->width, 3, OH, OW, packed ? OH + 6 : OH);
    sa.coef = YUV_MATRICES[yuv ? matrix : 0];
    sa.sf = surf_of(*surface);
    const dim3 grid((unsigned)(sa.a.items < EW_MAX_BLOCKS ? sa.a.items : EW_MAX_BLOCKS));
    if (yuv) {
        if (lens) { EW_SURF_CASE(true, "yuv", true, "lens") } else { EW_SURF_CASE(true, "yuv", false, "plain") }
    } else {
        if (lens) { EW_SURF_CASE(false, "rgb", true, "lens") } else { EW_SURF_CASE(false, "rgb", false, "plain") }
    }
    return 0;
}

}  // namespace
}  // namespace eve

using namespace eve;

extern "C" int eve_eye_warp_u8_to_nchw(long long N, int IH, int IW, int C, const uint8_t* frames_nhwc, const float* warps, int OH, int OW,
                                       float* dst_nchw, eve_stream_t stream) {
    char msg[128];
    if (const char* why = eye_warp_refusal(N, IH, IW, C, frames_nhwc, warps, OH, OW, dst_nchw)) {
        snprintf(msg, sizeof(msg), "eye_warp_u8_to_nchw: %s", why);
        return set_error_msg(msg);
    }
    const EyeWarpArgs a = eye_warp_args(N, IH, IW, C, OH, OW, OH);
    const dim3 grid((unsigned)(a.items < EW_MAX_BLOCKS ? a.items : EW_MAX_BLOCKS));
    EVE_LAUNCH("eye_warp_u8_kernel<float>", eye_warp_u8_kernel<float>, grid, dim3(EW_THREADS), 0, (hipStream_t)stream, a, frames_nhwc, warps,
               (void*)dst_nchw);
    EVE_CHECK_LAUNCH();
    return 0;
}

extern "C" int eve_eye_warp_u8_to_stem(int dtype, long long N, int IH, int IW, int C, const uint8_t* frames_nhwc, const float* warps, int OH,
                                       int OW, void* x_padded, eve_stream_t stream) {
    char msg[128];
    const char* why = eye_warp_refusal(N, IH, IW, C, frames_nhwc, warps, OH, OW, x_padded);
    if (!why && dtype != EVE_DT_BF16 && dtype != EVE_DT_F16) why = "dtype must be bf16 or f16 (the stem's packed input)";
    if (why) {
        snprintf(msg, sizeof(msg), "eye_warp_u8_to_stem: %s", why);
        return set_error_msg(msg);
    }
    const EyeWarpArgs a = eye_warp_args(N, IH, IW, C, OH, OW, OH + 6);
    const dim3 grid((unsigned)(a.items < EW_MAX_BLOCKS ? a.items : EW_MAX_BLOCKS));
    EVE_DISPATCH_H16(dtype, EVE_LAUNCH(EVE_HNAME(H, "eye_warp_u8_kernel<", ">"), eye_warp_u8_kernel<H>, grid, dim3(EW_THREADS), 0,
                                       (hipStream_t)stream, a, frames_nhwc, warps, x_padded));
    EVE_CHECK_LAUNCH();
    return 0;
}

extern "C" int eve_eye_warp_lens_u8_to_nchw(long long N, int IH, int IW, int C, const uint8_t* frames_nhwc, const float* warps,
                                            const float* lens, int OH, int OW, float* dst_nchw, eve_stream_t stream) {
    char msg[128];
    const char* why = eye_warp_refusal(N, IH, IW, C, frames_nhwc, warps, OH, OW, dst_nchw);
    if (!why && !lens) why = "bad arguments";
    if (why) {
        snprintf(msg, sizeof(msg), "eye_warp_lens_u8_to_nchw: %s", why);
        return set_error_msg(msg);
    }
    const EyeWarpArgs a = eye_warp_args(N, IH, IW, C, OH, OW, OH);
    const dim3 grid((unsigned)(a.items < EW_MAX_BLOCKS ? a.items : EW_MAX_BLOCKS));
    EVE_LAUNCH("eye_warp_lens_u8_kernel<float>", eye_warp_lens_u8_kernel<float>, grid, dim3(EW_THREADS), 0, (hipStream_t)stream, a,
               frames_nhwc, warps, lens, (void*)dst_nchw);
    EVE_CHECK_LAUNCH();
    return 0;
}

extern "C" int eve_eye_warp_lens_u8_to_stem(int dtype, long long N, int IH, int IW, int C, const uint8_t* frames_nhwc, const float* warps,
                                            const float* lens, int OH, int OW, void* x_padded, eve_stream_t stream) {
    char msg[128];
    const char* why = eye_warp_refusal(N, IH, IW, C, frames_nhwc, warps, OH, OW, x_padded);
    if (!why && !lens) why = "bad arguments";
    if (!why && dtype != EVE_DT_BF16 && dtype != EVE_DT_F16) why = "dtype must be bf16 or f16 (the stem's packed input)";
    if (why) {
        snprintf(msg, sizeof(msg), "eye_warp_lens_u8_to_stem: %s", why);
        return set_error_msg(msg);
    }
    const EyeWarpArgs a = eye_warp_args(N, IH, IW, C, OH, OW, OH + 6);
    const dim3 grid((unsigned)(a.items < EW_MAX_BLOCKS ? a.items : EW_MAX_BLOCKS));
    EVE_DISPATCH_H16(dtype, EVE_LAUNCH(EVE_HNAME(H, "eye_warp_lens_u8_kernel<", ">"), eye_warp_lens_u8_kernel<H>, grid, dim3(EW_THREADS), 0,
                                       (hipStream_t)stream, a, frames_nhwc, warps, lens, x_padded));
    EVE_CHECK_LAUNCH();
    return 0;
}

extern "C" int eve_eye_warp_fmt_to_nchw(int format, int matrix, long long N, int IH, int IW, const uint8_t* frames, const float* warps,
                                        const float* lens, int OH, int OW, float* dst_nchw, eve_stream_t stream) {
    char msg[160];
    if (const char* why = eye_warp_fmt_refusal(format, matrix, N, IH, IW, frames, warps, OH, OW, dst_nchw)) {
        snprintf(msg, sizeof(msg), "eye_warp_fmt_to_nchw: %s", why);
        return set_error_msg(msg);
    }
    eye_warp_fmt_launch(EVE_DT_F32, format, eye_warp_fmt_args(format, matrix, N, IH, IW, OH, OW, OH), frames, warps, lens, dst_nchw,
                        (hipStream_t)stream);
    EVE_CHECK_LAUNCH();
    return 0;
}

extern "C" int eve_eye_warp_fmt_to_stem(int dtype, int format, int matrix, long long N, int IH, int IW, const uint8_t* frames,
                                        const float* warps, const float* lens, int OH, int OW, void* x_padded, eve_stream_t stream) {
    char msg[160];
    const char* why = eye_warp_fmt_refusal(format, matrix, N, IH, IW, frames, warps, OH, OW, x_padded);
    if (!why && dtype != EVE_DT_BF16 && dtype != EVE_DT_F16) why = "dtype must be bf16 or f16 (the stem's packed input)";
    if (why) {
        snprintf(msg, sizeof(msg), "eye_warp_fmt_to_stem: %s", why);
        return set_error_msg(msg);
    }
    eye_warp_fmt_launch(dtype, format, eye_warp_fmt_args(format, matrix, N, IH, IW, OH, OW, OH + 6), frames, warps, lens, x_padded,
                        (hipStream_t)stream);
    EVE_CHECK_LAUNCH();
    return 0;
}

extern "C" int eve_eye_warp_surface_to_nchw(const eve_surface* surface, int matrix, long long N, const uint8_t* frames, const float* warps,
                                            const float* lens, int OH, int OW, float* dst_nchw, eve_stream_t stream) {
    if (const int rc = eye_warp_surface("eye_warp_surface_to_nchw", EVE_DT_F32, false, surface, matrix, N, frames, warps, lens, OH, OW, dst_nchw,
                                        (hipStream_t)stream))
        return rc;
    EVE_CHECK_LAUNCH();
    return 0;
}

extern "C" int eve_eye_warp_surface_to_stem(int dtype, const eve_surface* surface, int matrix, long long N, const uint8_t* frames,
                                            const float* warps, const float* lens, int OH, int OW, void* x_padded, eve_stream_t stream) {
    if (const int rc = eye_warp_surface("eye_warp_surface_to_stem", dtype, true, surface, matrix, N, frames, warps, lens, OH, OW, x_padded,
                                        (hipStream_t)stream))
        return rc;
    EVE_CHECK_LAUNCH();
    return 0;
}
