// The integer YUV -> RGB conversion of the pixel-format entry points (include/eve_hip.h eve_eye_warp_fmt_to_nchw,
// eve_screen_area_fmt_to_nchw; tests/pixel_format_ref.py has it in numpy): the one copy of the matrices and of the arithmetic.
//   yy = max(0, Y - y0) * CY + 2^19;   u = U - 128;   v = V - 128
//   R = clamp((yy + CVR*v) >> 20, 0, 255)   G = clamp((yy - CVG*v - CUG*u) >> 20, 0, 255)   B = clamp((yy + CUB*u) >> 20, 0, 255)
// in int32 with arithmetic shifts; every sum stays below 2^30 in magnitude.  The three chroma terms depend on the chroma sample
// alone, so a caller that converts several pixels of one sample (a 2 x 2 block, a pixel pair) takes yuv_chroma once and
// yuv_pixel per pixel; yuv_to_rgb is the two together.  Every factor fits 24 signed bits (max(0, Y - y0) <= 255, |u|, |v| <= 128,
// each constant < 2^23): with MUL24 the products are written as full-rate 24-bit multiplies (v_mul_i32_i24 / v_mad_i32_i24), which
// the compiler cannot choose by itself for the luma product (y0 is a kernel argument); the values are the same either way.  The
// area resize, bound by this arithmetic, asks for them; the eye warp (four taps per output pixel) keeps the plain products and
// with them the instructions it had.
#pragma once
#include <stdint.h>

namespace eve {

// the integer matrix of one launch, by value in the kernel's arguments
struct YuvCoef {
    int y0, cy, cvr, cug, cvg, cub;
};

// (y0, CY, CVR, CUG, CVG, CUB), each constant floor(c * 2^20 + 0.5) of its coefficient (include/eve_hip.h), indexed by EVE_YUV_*
constexpr YuvCoef YUV_MATRICES[3] = {
    {16, 1220542, 1673527, 409993, 852492, 2116026},      // bt601: 1.164, 1.596, 0.391, 0.813, 2.018 (OpenCV's COLOR_YUV2RGB_NV12)
    {16, 1220542, 1880097, 223347, 558891, 2214593},      // bt709: 1.164, 1.793, 0.213, 0.533, 2.112
    {0, 1048576, 1470104, 360853, 748826, 1858077},       // jfif:  1, 1.402, 0.344136, 0.714136, 1.772
};

// what one chroma sample adds to the luma term of R, G and B
struct YuvChroma {
    int r, g, b;
};

template <bool MUL24>
__device__ __forceinline__ int yuv_mul(const int a, const int b) {
    if constexpr (MUL24) return __mul24(a, b);
    else return a * b;
}

template <bool MUL24 = false>
__device__ __forceinline__ YuvChroma yuv_chroma(const int U, const int V, const YuvCoef& k) {
    const int u = U - 128, v = V - 128;
    YuvChroma c;
    c.r = yuv_mul<MUL24>(k.cvr, v);
    c.g = -yuv_mul<MUL24>(k.cvg, v) - yuv_mul<MUL24>(k.cug, u);
    c.b = yuv_mul<MUL24>(k.cub, u);
    return c;
}

__device__ __forceinline__ uint32_t yuv_clamp(const int s) {
    const int q = s >> 20;
    return (uint32_t)(q < 0 ? 0 : q > 255 ? 255 : q);
}

// the 8-bit (r, g, b) of a pixel with luma Y under the chroma sample behind c
template <bool MUL24 = false>
__device__ __forceinline__ void yuv_pixel(const int Y, const YuvChroma& c, const YuvCoef& k, uint32_t (&rgb)[3]) {
    const int yy = yuv_mul<MUL24>(Y - k.y0 > 0 ? Y - k.y0 : 0, k.cy) + (1 << 19);
    rgb[0] = yuv_clamp(yy + c.r);
    rgb[1] = yuv_clamp(yy + c.g);
    rgb[2] = yuv_clamp(yy + c.b);
}

__device__ __forceinline__ void yuv_to_rgb(const int Y, const int U, const int V, const YuvCoef& k, uint32_t (&rgb)[3]) {
    yuv_pixel(Y, yuv_chroma(U, V, k), k, rgb);
}

// The forward direction, RGB -> YUV, of the overlay's output (include/eve_hip.h eve_overlay_render; tests/overlay_ref.py):
//   Y = clamp((KYR*R + KYG*G + KYB*B + (y0  << 20) + 2^19) >> 20, 0, 255)
//   U = clamp((KUR*R + KUG*G + KUB*B + (128 << 20) + 2^19) >> 20, 0, 255)        V likewise with its row
// in int32 with arithmetic shifts (every sum stays below 2^29 in magnitude); Y per pixel, U and V from a 2 x 2 block's rounded mean.
struct RgbYuvCoef {
    int y0, y[3], u[3], v[3];
};

// each constant sign(c) * floor(|c| * 2^20 + 0.5) of its coefficient, indexed by EVE_YUV_*
constexpr RgbYuvCoef RGB_YUV_MATRICES[3] = {
    {16, {269484, 528482, 102760}, {-155189, -305136, 460325}, {460325, -385876, -74449}},   // bt601: (0.257, 0.504, 0.098), (-0.148, -0.291, 0.439), (0.439, -0.368, -0.071)
    {16, {191889, 643826, 65012}, {-105906, -355467, 460325}, {460325, -418382, -41943}},    // bt709: (0.183, 0.614, 0.062), (-0.101, -0.339, 0.439), (0.439, -0.399, -0.040)
    {0, {313524, 615514, 119538}, {-176933, -347355, 524288}, {524288, -439026, -85262}},    // jfif:  (0.299, 0.587, 0.114), (-0.168736, -0.331264, 0.5), (0.5, -0.418688, -0.081312)
};

// one row of the forward matrix applied to 8-bit (r, g, b); offset is y0 for the Y row and 128 for U and V.
// The empty asm hides the clamped value's origin from the compiler.  Callers OR these values into dwords byte by byte, and hipcc
// (ROCm 7's clang for gfx950) then fuses two "shift right, clamp to 0..255" results into one v_ashr_pk_u8_i32 and ORs the other
// bytes on top of its destination as if the instruction had cleared bits 31:16 -- the hardware leaves them as they were, so the
// old register contents bled into bytes 2 and 3 of every packed dword (seen on an MI355X: NV12 / I420 output of the vector form).
__device__ __forceinline__ uint32_t rgb_yuv_row(const int (&k)[3], const int offset, const uint32_t r, const uint32_t g, const uint32_t b) {
    uint32_t v = yuv_clamp(k[0] * (int)r + k[1] * (int)g + k[2] * (int)b + (offset << 20) + (1 << 19));
    asm("" : "+v"(v));
    return v;
}

}  // namespace eve
