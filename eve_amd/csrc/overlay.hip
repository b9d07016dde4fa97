// The tracking overlay on the device (include/eve_hip.h eve_overlay_render; tests/overlay_ref.py states it in numpy): one pass over
// a full-resolution capture that converts it to RGB, blends the up-sampled heat map, replaces the inset rectangle, draws up to
// eight anti-aliased discs and writes the frame an encoder or a display reads (rgb, bgr, nv12 or i420).  Everything after three
// float32 quantisations (heat value, marker centre x and y) is integer arithmetic, so the result is the same bits wherever it is
// evaluated.
//
// Shape: a workgroup takes one (frame, row pair) at a time (grid-stride over the items, as screen_resize.hip does); a thread owns
// a tile of 2 rows x 8 columns, which holds four whole 2 x 2 chroma blocks on both sides: a YUV capture is one 8-byte luma load per
// row plus the chroma bytes under it, an RGB capture 24 bytes per row, an NV12 result one 8-byte luma store per row plus one 8-byte
// chroma store.  The 48 channel values of the tile stay in registers between the layers (every index is a compile-time constant:
// no scratch).  A 1920-wide row pair gives 240 of the 256 threads a tile.  The byte form (a width that is no multiple of 8, an odd
// height, a base that is not 16-byte aligned) keeps the tiles and moves single bytes, each pixel under its own bounds test.
//
// Bounds: every address is computed from the pixel the thread owns.  A marker only changes VALUES: its centre is compared with
// pixel coordinates and never indexed with.  The heat indices are clamped to [0, H - 1] as the contract states; the inset is read
// only by pixels inside its rectangle, which the entry point has checked to lie inside the frame.
//
// The marker table of a frame (<= 8 entries) is read through uniform loads and quantised per thread (an LDS copy behind a barrier
// per item cost more than it saved: a workgroup has one tile per thread between two items).  A tile culls each marker by its bounding box, then each pixel does, before any sub-sample test: far from every marker a pixel
// costs a handful of compares.  After the cull |8X + k - qx| <= 8 * 255 + 7, so the squared distances fit 32 bits.
//
// Heat taps in 32 bits: t = (2X + 1) * HW * 128 <= 32767 * 1024 * 128 < 2^32 for X < 16384 and HW <= 1024, and
//   fx = max(nx, 0) * 128 // IW = max(t // IW - 128, 0)      (nx = (2X + 1) * HW - IW;  t - 128 * IW = 128 * nx)
// so one unsigned division gives the first column's quotient and remainder, and the next column's follow by adding the quotient
// and remainder of 256 * HW / IW (uniform): never a value above the first t is formed.
#include "common.h"
#include "yuv_rgb.h"

namespace eve {
namespace {

constexpr int OV_THREADS = 256;
constexpr int OV_COLS = 8;               // columns of a thread's tile (two rows high)
constexpr int OV_MAX_BLOCKS = 4096;      // (frame, row pair) items beyond that are taken in a grid-stride loop
constexpr int OV_MAX_MARKERS = 8;
constexpr int OV_MAX_HEAT = 1024;
constexpr int OV_MAX_DIM = 16384;
constexpr float OV_Q_LIMIT = 1048576.0f; // |q| <= 2^20 eighths of a pixel

struct OverlayArgs {
    long long items;                     // N * ceil(IH / 2)
    int IH, IW;
    const uint8_t* src;
    uint8_t* dst;
    YuvCoef inv;
    RgbYuvCoef fwd;
    int M;
    const float* centres;                // [N][M][2]
    const uint8_t* marker_valid;         // [N][M] or null
    const int* table;                    // [M][4]
    float sx, sy;
    const float* heat;                   // [N][HH][HW] or null
    int HH, HW, heat_rgb, amax;
    const uint8_t* inset;                // [N][ih][iw][3] or null
    int ih, iw, ix0, iy0, zoom, mirror;
    const uint8_t* frame_valid;          // [N] or null
};

__host__ __device__ constexpr size_t ov_frame_bytes(const int fmt, const int IH, const int IW) {
    return fmt == EVE_PIX_NV12 || fmt == EVE_PIX_I420 ? (size_t)IH * IW / 2 * 3
           : (size_t)IH * IW * (fmt == EVE_PIX_YUYV ? 2 : fmt == EVE_PIX_BGRA || fmt == EVE_PIX_RGBA ? 4 : 3);
}

template <int W>
__device__ __forceinline__ uint32_t ov_byte(const uint32_t (&w)[W], const int k) { return (w[k >> 2] >> (8 * (k & 3))) & 0xffu; }

__device__ __forceinline__ void ov_load8(const uint8_t* __restrict__ p, uint32_t* w) {
    const uint2 q = *reinterpret_cast<const uint2*>(p);
    w[0] = q.x; w[1] = q.y;
}
__device__ __forceinline__ void ov_load16(const uint8_t* __restrict__ p, uint32_t* w) {
    const uint4 q = *reinterpret_cast<const uint4*>(p);
    w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
}

// ------------------------------------------------------------------------------------------------------------- layer 1: source
// px[r][c][0..2] = (R, G, B) of pixel (Y0 + r, X0 + c); pixels outside the frame (byte form only) are left 0
template <int FMT, bool VEC>
__device__ __forceinline__ void ov_load_tile(const uint8_t* __restrict__ frame, const int IH, const int IW, const int Y0, const int X0,
                                             const YuvCoef& coef, uint32_t (&px)[2][OV_COLS][3]) {
    constexpr bool PACKED_RGB = FMT == EVE_PIX_RGB || FMT == EVE_PIX_RGBA || FMT == EVE_PIX_BGR || FMT == EVE_PIX_BGRA;
    constexpr bool SWAP = FMT == EVE_PIX_BGR || FMT == EVE_PIX_BGRA;
    constexpr int C = FMT == EVE_PIX_RGBA || FMT == EVE_PIX_BGRA ? 4 : 3;
    if constexpr (!VEC) {
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < OV_COLS; ++c)
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) px[r][c][ch] = 0u;
    }
    if constexpr (PACKED_RGB) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const uint8_t* row = frame + ((size_t)(Y0 + r) * IW + X0) * C;
            if constexpr (VEC) {
                uint32_t w[2 * C];
                if constexpr (C == 3) { ov_load8(row, w); ov_load8(row + 8, w + 2); ov_load8(row + 16, w + 4); }
                else { ov_load16(row, w); ov_load16(row + 16, w + 4); }
#pragma unroll
                for (int c = 0; c < OV_COLS; ++c)
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) px[r][c][SWAP ? 2 - ch : ch] = ov_byte(w, c * C + ch);
            } else {
#pragma unroll
                for (int c = 0; c < OV_COLS; ++c)
                    if (Y0 + r < IH && X0 + c < IW) {
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) px[r][c][SWAP ? 2 - ch : ch] = row[c * C + ch];
                    }
            }
        }
    } else if constexpr (FMT == EVE_PIX_YUYV) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const uint8_t* row = frame + ((size_t)(Y0 + r) * IW + X0) * 2;
            if constexpr (VEC) {
                uint32_t w[4];
                ov_load16(row, w);
#pragma unroll
                for (int j = 0; j < OV_COLS / 2; ++j) {       // dword j: Y0 U Y1 V of pixels 2j, 2j + 1
                    const YuvChroma k = yuv_chroma<true>((int)((w[j] >> 8) & 0xffu), (int)(w[j] >> 24), coef);
                    yuv_pixel<true>((int)(w[j] & 0xffu), k, coef, px[r][2 * j]);
                    yuv_pixel<true>((int)((w[j] >> 16) & 0xffu), k, coef, px[r][2 * j + 1]);
                }
            } else {
#pragma unroll
                for (int j = 0; j < OV_COLS / 2; ++j)
                    if (Y0 + r < IH && X0 + 2 * j < IW) {     // IW is even: the pair is whole
                        const uint8_t* q = row + 4 * j;
                        const YuvChroma k = yuv_chroma<true>((int)q[1], (int)q[3], coef);
                        yuv_pixel<true>((int)q[0], k, coef, px[r][2 * j]);
                        yuv_pixel<true>((int)q[2], k, coef, px[r][2 * j + 1]);
                    }
            }
        }
    } else {                                                  // NV12, I420: IH and IW even, so every 2 x 2 block is whole
        const size_t luma = (size_t)IH * IW;
        const size_t plane = (size_t)(IH >> 1) * (IW >> 1);
        const int cy = Y0 >> 1;
        if constexpr (VEC) {
            uint32_t yq[2][2], cq[2];
            ov_load8(frame + (size_t)Y0 * IW + X0, yq[0]);
            ov_load8(frame + (size_t)(Y0 + 1) * IW + X0, yq[1]);
            if constexpr (FMT == EVE_PIX_NV12) {
                ov_load8(frame + luma + (size_t)cy * IW + X0, cq);
            } else {
                const uint8_t* u = frame + luma + (size_t)cy * (IW >> 1) + (X0 >> 1);
                cq[0] = *reinterpret_cast<const uint32_t*>(u);
                cq[1] = *reinterpret_cast<const uint32_t*>(u + plane);
            }
#pragma unroll
            for (int j = 0; j < OV_COLS / 2; ++j) {
                const int U = (int)ov_byte(cq, FMT == EVE_PIX_NV12 ? 2 * j : j);
                const int V = (int)ov_byte(cq, FMT == EVE_PIX_NV12 ? 2 * j + 1 : 4 + j);
                const YuvChroma k = yuv_chroma<true>(U, V, coef);
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int e = 0; e < 2; ++e) yuv_pixel<true>((int)ov_byte(yq[r], 2 * j + e), k, coef, px[r][2 * j + e]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < OV_COLS / 2; ++j)
                if (Y0 < IH && X0 + 2 * j < IW) {
                    int U, V;
                    if constexpr (FMT == EVE_PIX_NV12) {
                        const uint8_t* q = frame + luma + (size_t)cy * IW + X0 + 2 * j;
                        U = q[0]; V = q[1];
                    } else {
                        const uint8_t* q = frame + luma + (size_t)cy * (IW >> 1) + (X0 >> 1) + j;
                        U = q[0]; V = q[plane];
                    }
                    const YuvChroma k = yuv_chroma<true>(U, V, coef);
#pragma unroll
                    for (int r = 0; r < 2; ++r) {
                        const uint8_t* q = frame + (size_t)(Y0 + r) * IW + X0 + 2 * j;
                        yuv_pixel<true>((int)q[0], k, coef, px[r][2 * j]);
                        yuv_pixel<true>((int)q[1], k, coef, px[r][2 * j + 1]);
                    }
                }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------- layer 5: output
template <int FMT, bool VEC>
__device__ __forceinline__ void ov_store_tile(uint8_t* __restrict__ out, const int IH, const int IW, const int Y0, const int X0,
                                              const RgbYuvCoef& k, const uint32_t (&px)[2][OV_COLS][3]) {
    if constexpr (FMT == EVE_PIX_RGB || FMT == EVE_PIX_BGR) {
        constexpr bool SWAP = FMT == EVE_PIX_BGR;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            uint8_t* row = out + ((size_t)(Y0 + r) * IW + X0) * 3;
            if constexpr (VEC) {
                uint32_t w[6] = {0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
                for (int c = 0; c < OV_COLS; ++c)
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) w[(c * 3 + ch) >> 2] |= px[r][c][SWAP ? 2 - ch : ch] << (8 * ((c * 3 + ch) & 3));
#pragma unroll
                for (int i = 0; i < 3; ++i) *reinterpret_cast<uint2*>(row + 8 * i) = make_uint2(w[2 * i], w[2 * i + 1]);
            } else {
#pragma unroll
                for (int c = 0; c < OV_COLS; ++c)
                    if (Y0 + r < IH && X0 + c < IW) {
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) row[c * 3 + ch] = (uint8_t)px[r][c][SWAP ? 2 - ch : ch];
                    }
            }
        }
    } else {                                                  // NV12, I420: IH and IW even
        const size_t luma = (size_t)IH * IW;
        const size_t plane = (size_t)(IH >> 1) * (IW >> 1);
        const int cy = Y0 >> 1;
        uint32_t U[OV_COLS / 2], V[OV_COLS / 2];
#pragma unroll
        for (int j = 0; j < OV_COLS / 2; ++j) {
            uint32_t m[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) m[ch] = (px[0][2 * j][ch] + px[0][2 * j + 1][ch] + px[1][2 * j][ch] + px[1][2 * j + 1][ch] + 2u) >> 2;
            U[j] = rgb_yuv_row(k.u, 128, m[0], m[1], m[2]);
            V[j] = rgb_yuv_row(k.v, 128, m[0], m[1], m[2]);
        }
        if constexpr (VEC) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                uint32_t w[2] = {0u, 0u};
#pragma unroll
                for (int c = 0; c < OV_COLS; ++c) w[c >> 2] |= rgb_yuv_row(k.y, k.y0, px[r][c][0], px[r][c][1], px[r][c][2]) << (8 * (c & 3));
                *reinterpret_cast<uint2*>(out + (size_t)(Y0 + r) * IW + X0) = make_uint2(w[0], w[1]);
            }
            if constexpr (FMT == EVE_PIX_NV12) {
                uint32_t w[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) w[i] = U[2 * i] | (V[2 * i] << 8) | (U[2 * i + 1] << 16) | (V[2 * i + 1] << 24);
                *reinterpret_cast<uint2*>(out + luma + (size_t)cy * IW + X0) = make_uint2(w[0], w[1]);
            } else {
                uint8_t* u = out + luma + (size_t)cy * (IW >> 1) + (X0 >> 1);
                *reinterpret_cast<uint32_t*>(u) = U[0] | (U[1] << 8) | (U[2] << 16) | (U[3] << 24);
                *reinterpret_cast<uint32_t*>(u + plane) = V[0] | (V[1] << 8) | (V[2] << 16) | (V[3] << 24);
            }
        } else {
#pragma unroll
            for (int j = 0; j < OV_COLS / 2; ++j)
                if (Y0 < IH && X0 + 2 * j < IW) {
#pragma unroll
                    for (int r = 0; r < 2; ++r)
#pragma unroll
                        for (int e = 0; e < 2; ++e) {
                            const int c = 2 * j + e;
                            out[(size_t)(Y0 + r) * IW + X0 + c] = (uint8_t)rgb_yuv_row(k.y, k.y0, px[r][c][0], px[r][c][1], px[r][c][2]);
                        }
                    if constexpr (FMT == EVE_PIX_NV12) {
                        uint8_t* q = out + luma + (size_t)cy * IW + X0 + 2 * j;
                        q[0] = (uint8_t)U[j]; q[1] = (uint8_t)V[j];
                    } else {
                        uint8_t* q = out + luma + (size_t)cy * (IW >> 1) + (X0 >> 1) + j;
                        q[0] = (uint8_t)U[j]; q[plane] = (uint8_t)V[j];
                    }
                }
        }
    }
}

// ----------------------------------------------------------------------------------------------------------- layer 2: heat map
// the taps of `count` consecutive output pixels from `first` along an axis of I output pixels over H heat cells
template <int COUNT>
__device__ __forceinline__ void ov_heat_taps(const uint32_t first, const uint32_t I, const uint32_t H, const uint32_t qs, const uint32_t rs,
                                             uint32_t (&i0)[COUNT], uint32_t (&i1)[COUNT], uint32_t (&w)[COUNT]) {
    // first < 16384 at every call: a tile begins inside the frame
    const uint32_t t = (2u * first + 1u) * H * 128u;
    uint32_t q = t / I, rem = t - q * I;
#pragma unroll
    for (int k = 0; k < COUNT; ++k) {
        const uint32_t f = q > 128u ? q - 128u : 0u;
        const uint32_t a = f >> 8;
        i0[k] = a < H - 1u ? a : H - 1u;
        i1[k] = i0[k] + 1u < H - 1u ? i0[k] + 1u : H - 1u;
        w[k] = f & 255u;
        q += qs;
        rem += rs;
        if (rem >= I) { rem -= I; ++q; }
    }
}

// rint(clamp(h, 0, 1) * 255) in float32, NaN -> 0
__device__ __forceinline__ uint32_t ov_heat_q(const float h) {
    const float lo = h > 0.0f ? h : 0.0f;                     // false for NaN
    const float c = lo < 1.0f ? lo : 1.0f;
    return (uint32_t)__float2int_rn(c * 255.0f);
}

__device__ __forceinline__ uint32_t ov_sel2(const uint32_t a0, const uint32_t a1, const uint32_t i) { return i == 0u ? a0 : a1; }
__device__ __forceinline__ uint32_t ov_sel3(const uint32_t a0, const uint32_t a1, const uint32_t a2, const uint32_t i) {
    return i == 0u ? a0 : i == 1u ? a1 : a2;
}

__device__ __forceinline__ void ov_heat_blend(const uint32_t q00, const uint32_t q01, const uint32_t q10, const uint32_t q11, const uint32_t wx,
                                              const uint32_t wy, const uint32_t amax, const uint32_t (&col)[3], uint32_t (&v)[3]) {
    const uint32_t ux = 256u - wx, uy = 256u - wy;
    const uint32_t s = (q00 * ux * uy + q01 * wx * uy + q10 * ux * wy + q11 * wx * wy + 32768u) >> 16;
    const uint32_t alpha = (s * amax + 127u) / 255u;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) v[ch] = (v[ch] * (255u - alpha) + col[ch] * alpha + 127u) / 255u;
}

// Where the map is up-sampled (a 1080p frame over 72 x 128 cells: 15 pixels per cell) the taps of a whole tile lie in a 3 x 3 block
// of cells: nine loads and quantisations for the tile's sixteen pixels, the taps chosen by selects -- and a tile whose nine cells
// are all 0 (most of a frame under a Gaussian) is done, since alpha = 0 leaves every value as it is.  A tile that spans more cells
// (a map finer than 8 x 2 pixels per cell) loads its four taps per pixel.  Same values either way.
__device__ __forceinline__ void ov_heat_layer(const float* __restrict__ heat, const OverlayArgs& a, const int Y0, const int X0, const uint32_t qsx,
                                              const uint32_t rsx, const uint32_t qsy, const uint32_t rsy, uint32_t (&px)[2][OV_COLS][3]) {
    uint32_t x0[OV_COLS], x1[OV_COLS], wx[OV_COLS], y0[2], y1[2], wy[2];
    ov_heat_taps<OV_COLS>((uint32_t)X0, (uint32_t)a.IW, (uint32_t)a.HW, qsx, rsx, x0, x1, wx);
    ov_heat_taps<2>((uint32_t)Y0, (uint32_t)a.IH, (uint32_t)a.HH, qsy, rsy, y0, y1, wy);
    const uint32_t col[3] = {((uint32_t)a.heat_rgb >> 16) & 0xffu, ((uint32_t)a.heat_rgb >> 8) & 0xffu, (uint32_t)a.heat_rgb & 0xffu};
    const uint32_t amax = (uint32_t)a.amax;
    const uint32_t xs = x0[0], ys = y0[0];                    // the taps are monotonic along both axes
    if (x0[OV_COLS - 1] - xs <= 1u && y0[1] - ys <= 1u) {     // every tap lies in cells [ys, ys + 2] x [xs, xs + 2], clamped to the map
        uint32_t q[3][3], any = 0u;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const uint32_t yi = ys + i < (uint32_t)a.HH - 1u ? ys + i : (uint32_t)a.HH - 1u;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const uint32_t xj = xs + j < (uint32_t)a.HW - 1u ? xs + j : (uint32_t)a.HW - 1u;
                q[i][j] = ov_heat_q(heat[(size_t)yi * a.HW + xj]);
                any |= q[i][j];
            }
        }
        if (any == 0u) return;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const uint32_t ty = y0[r] - ys, by = y1[r] - ys;  // 0..1 and 0..2
            uint32_t top[3], bot[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                top[j] = ov_sel2(q[0][j], q[1][j], ty);
                bot[j] = ov_sel3(q[0][j], q[1][j], q[2][j], by);
            }
#pragma unroll
            for (int c = 0; c < OV_COLS; ++c) {
                const uint32_t tx = x0[c] - xs, bx = x1[c] - xs;
                ov_heat_blend(ov_sel2(top[0], top[1], tx), ov_sel3(top[0], top[1], top[2], bx), ov_sel2(bot[0], bot[1], tx),
                              ov_sel3(bot[0], bot[1], bot[2], bx), wx[c], wy[r], amax, col, px[r][c]);
            }
        }
        return;
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const float* top = heat + (size_t)y0[r] * a.HW;
        const float* bot = heat + (size_t)y1[r] * a.HW;
#pragma unroll
        for (int c = 0; c < OV_COLS; ++c)
            ov_heat_blend(ov_heat_q(top[x0[c]]), ov_heat_q(top[x1[c]]), ov_heat_q(bot[x0[c]]), ov_heat_q(bot[x1[c]]), wx[c], wy[r], amax, col, px[r][c]);
    }
}

// -------------------------------------------------------------------------------------------------------------- layer 3: inset
__device__ __forceinline__ uint32_t ov_div_zoom(const uint32_t d, const int zoom) {
    return zoom == 1 ? d : zoom == 2 ? d >> 1 : zoom == 3 ? d / 3u : d >> 2;
}

__device__ __forceinline__ void ov_inset_layer(const uint8_t* __restrict__ inset, const OverlayArgs& a, const int Y0, const int X0,
                                               uint32_t (&px)[2][OV_COLS][3]) {
    const int zw = a.zoom * a.iw, zh = a.zoom * a.ih;
    if (X0 + OV_COLS <= a.ix0 || X0 >= a.ix0 + zw || Y0 + 2 <= a.iy0 || Y0 >= a.iy0 + zh) return;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < OV_COLS; ++c) {
            const int dx = X0 + c - a.ix0, dy = Y0 + r - a.iy0;
            if (dx >= 0 && dx < zw && dy >= 0 && dy < zh) {     // so 0 <= i < ih and 0 <= j < iw below
                const uint32_t i = ov_div_zoom((uint32_t)dy, a.zoom);
                uint32_t j = ov_div_zoom((uint32_t)dx, a.zoom);
                if (a.mirror) j = (uint32_t)a.iw - 1u - j;
                const uint8_t* p = inset + ((size_t)i * a.iw + j) * 3;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) px[r][c][ch] = p[ch];
            }
        }
}

// ------------------------------------------------------------------------------------------------------------ layer 4: markers
__device__ __forceinline__ void ov_disc(const int (&dx2)[4], const int (&dy2)[4], const int r, const int color, uint32_t (&v)[3]) {
    const int lim = 64 * r * r;
    uint32_t n = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) n += dx2[i] + dy2[j] <= lim ? 1u : 0u;
    const uint32_t col[3] = {((uint32_t)color >> 16) & 0xffu, ((uint32_t)color >> 8) & 0xffu, (uint32_t)color & 0xffu};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) v[ch] = (v[ch] * (16u - n) + col[ch] * n + 8u) >> 4;
}

// The frame's marker rows are read at addresses that are the same for the whole workgroup (uniform loads through the scalar cache:
// no LDS staging and no barrier) and quantised by every thread: a dozen operations per marker and tile.
__device__ __forceinline__ void ov_marker_layer(const OverlayArgs& a, const long long n, const int Y0, const int X0, uint32_t (&px)[2][OV_COLS][3]) {
    for (int m = 0; m < a.M; ++m) {
        const size_t e = (size_t)n * a.M + m;
        if (a.marker_valid && a.marker_valid[e] == 0) continue;
        const float fx = rintf((a.centres[2 * e] * a.sx) * 8.0f), fy = rintf((a.centres[2 * e + 1] * a.sy) * 8.0f);
        // a NaN or infinite coordinate gives a NaN or infinite product (sx, sy are finite): both compare false
        if (!(fabsf(fx) <= OV_Q_LIMIT && fabsf(fy) <= OV_Q_LIMIT)) continue;
        const int qx = (int)fx, qy = (int)fy;
        const int r_fill = a.table[4 * m], r_out = a.table[4 * m + 1], c_fill = a.table[4 * m + 2], c_out = a.table[4 * m + 3];
        const int R8 = 8 * (r_out > r_fill ? r_out : r_fill);
        // the tile's sub-samples lie in [8*X0 + 1, 8*X0 + 63] x [8*Y0 + 1, 8*Y0 + 15]; |q| <= 2^20 and 8 * X < 2^17: no overflow
        const int tx = 8 * X0 - qx, ty = 8 * Y0 - qy;
        if (tx + 63 < -R8 || tx + 1 > R8 || ty + 15 < -R8 || ty + 1 > R8) continue;
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < OV_COLS; ++c) {
                const int bx = tx + 8 * c, by = ty + 8 * r;
                if (bx + 7 < -R8 || bx + 1 > R8 || by + 7 < -R8 || by + 1 > R8) continue;      // no sub-sample inside either disc
                int dx2[4], dy2[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    dx2[i] = (bx + 2 * i + 1) * (bx + 2 * i + 1);
                    dy2[i] = (by + 2 * i + 1) * (by + 2 * i + 1);
                }
                if (r_out > 0) ov_disc(dx2, dy2, r_out, c_out, px[r][c]);
                ov_disc(dx2, dy2, r_fill, c_fill, px[r][c]);
            }
    }
}

template <int IN, int OUT, bool VEC>
__global__ __launch_bounds__(OV_THREADS) void overlay_kernel(const OverlayArgs a) {
    const int tid = threadIdx.x;
    const int IH = a.IH, IW = a.IW;
    const int pairs = (IH + 1) >> 1, groups = (IW + OV_COLS - 1) / OV_COLS;
    const size_t in_bytes = ov_frame_bytes(IN, IH, IW), out_bytes = ov_frame_bytes(OUT, IH, IW);
    uint32_t qsx = 0u, rsx = 0u, qsy = 0u, rsy = 0u;
    if (a.heat) {
        qsx = 256u * (uint32_t)a.HW / (uint32_t)IW; rsx = 256u * (uint32_t)a.HW - qsx * (uint32_t)IW;
        qsy = 256u * (uint32_t)a.HH / (uint32_t)IH; rsy = 256u * (uint32_t)a.HH - qsy * (uint32_t)IH;
    }
    for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
        const long long n = item / pairs;
        const int Y0 = 2 * (int)(item - n * pairs);
        const uint8_t* frame = a.src + (size_t)n * in_bytes;
        uint8_t* out = a.dst + (size_t)n * out_bytes;
        const bool draw = !a.frame_valid || a.frame_valid[n] != 0;
        for (int g = tid; g < groups; g += OV_THREADS) {
            const int X0 = g * OV_COLS;
            uint32_t px[2][OV_COLS][3];
            ov_load_tile<IN, VEC>(frame, IH, IW, Y0, X0, a.inv, px);
            if (draw) {
                if (a.heat) ov_heat_layer(a.heat + (size_t)n * a.HH * a.HW, a, Y0, X0, qsx, rsx, qsy, rsy, px);
                if (a.inset) ov_inset_layer(a.inset + (size_t)n * a.ih * a.iw * 3, a, Y0, X0, px);
                ov_marker_layer(a, n, Y0, X0, px);
            }
            ov_store_tile<OUT, VEC>(out, IH, IW, Y0, X0, a.fwd, px);
        }
    }
}

}  // namespace
}  // namespace eve

using namespace eve;

#define OV_LAUNCH(IN, in, OUT, out)                                                                                                \
    if (vec) EVE_LAUNCH("overlay_kernel<" in "," out ",true>", (overlay_kernel<IN, OUT, true>), grid, dim3(OV_THREADS), 0, (hipStream_t)stream, a); \
    else EVE_LAUNCH("overlay_kernel<" in "," out ",false>", (overlay_kernel<IN, OUT, false>), grid, dim3(OV_THREADS), 0, (hipStream_t)stream, a);
#define OV_OUT_CASES(IN, in)                                            \
    case IN:                                                            \
        switch (out_format) {                                           \
            case EVE_PIX_RGB: OV_LAUNCH(IN, in, EVE_PIX_RGB, "rgb") break;    \
            case EVE_PIX_BGR: OV_LAUNCH(IN, in, EVE_PIX_BGR, "bgr") break;    \
            case EVE_PIX_NV12: OV_LAUNCH(IN, in, EVE_PIX_NV12, "nv12") break; \
            case EVE_PIX_I420: OV_LAUNCH(IN, in, EVE_PIX_I420, "i420") break; \
        }                                                               \
        break;

extern "C" int eve_overlay_render(int in_format, int out_format, int matrix, long long N, int IH, int IW, const uint8_t* src, uint8_t* dst,
                                  int M, const float* centres, const uint8_t* marker_valid, const int* marker_table, float sx, float sy,
                                  const float* heat, int HH, int HW, int heat_rgb, int amax, const uint8_t* inset, int ih, int iw, int ix0,
                                  int iy0, int zoom, int mirror, const uint8_t* frame_valid, eve_stream_t stream) {
    const char* why = nullptr;
    const bool yuv_in = in_format == EVE_PIX_NV12 || in_format == EVE_PIX_I420, yuv_out = out_format == EVE_PIX_NV12 || out_format == EVE_PIX_I420;
    if (N <= 0 || IH <= 0 || IW <= 0 || !src || !dst) why = "bad arguments";
    else if (in_format < EVE_PIX_BGR || in_format > EVE_PIX_RGBA) why = "unknown format (EVE_PIX_RGB, _RGBA, _BGR, _BGRA, _NV12, _I420 or _YUYV)";
    else if (out_format != EVE_PIX_RGB && out_format != EVE_PIX_BGR && !yuv_out) why = "unknown output format (EVE_PIX_RGB, _BGR, _NV12 or _I420)";
    else if (matrix < EVE_YUV_BT601 || matrix > EVE_YUV_JFIF) why = "unknown matrix (EVE_YUV_BT601, _BT709 or _JFIF)";
    else if (IH > OV_MAX_DIM || IW > OV_MAX_DIM) why = "frame too large (IH, IW <= 16384)";
    else if (yuv_in && ((IH | IW) & 1)) why = "IH and IW must be even for an NV12 or I420 capture (2 x 2 chroma blocks)";
    else if (in_format == EVE_PIX_YUYV && (IW & 1)) why = "IW must be even for a YUYV capture (chroma pairs)";
    else if (yuv_out && ((IH | IW) & 1)) why = "IH and IW must be even for NV12 or I420 output (2 x 2 chroma blocks)";
    else if (N > (long long)0x7fffffff / ((IH + 1) / 2)) why = "N * ceil(IH / 2) must fit 31 bits";
    else if (M < 0 || M > OV_MAX_MARKERS) why = "M must be in 0..8";
    else if (M > 0 && (!centres || !marker_table)) why = "markers need centres and marker_table";
    else if (M > 0 && !(fabsf(sx) <= 3.0e38f && fabsf(sy) <= 3.0e38f)) why = "sx and sy must be finite";
    else if (heat && (HH < 1 || HW < 1 || HH > OV_MAX_HEAT || HW > OV_MAX_HEAT)) why = "heat map too large (1 <= HH, HW <= 1024)";
    else if (heat && (amax < 0 || amax > 255 || heat_rgb < 0 || heat_rgb > 0xffffff)) why = "amax must be in 0..255 and the heat colour 0xRRGGBB";
    else if (inset && (zoom < 1 || zoom > 4)) why = "zoom must be in 1..4";
    else if (inset && (ih < 1 || iw < 1 || ih > OV_MAX_DIM || iw > OV_MAX_DIM)) why = "bad inset size";
    else if (inset && (ix0 < 0 || iy0 < 0 || (long long)ix0 + (long long)zoom * iw > IW || (long long)iy0 + (long long)zoom * ih > IH))
        why = "the inset rectangle must lie inside the frame";
    if (why) {
        char msg[192];
        snprintf(msg, sizeof(msg), "overlay_render: %s", why);
        return set_error_msg(msg);
    }
    OverlayArgs a;
    a.items = N * ((IH + 1) / 2);
    a.IH = IH; a.IW = IW; a.src = src; a.dst = dst;
    a.inv = YUV_MATRICES[matrix]; a.fwd = RGB_YUV_MATRICES[matrix];
    a.M = M; a.centres = centres; a.marker_valid = marker_valid; a.table = marker_table; a.sx = sx; a.sy = sy;
    a.heat = heat; a.HH = HH; a.HW = HW; a.heat_rgb = heat_rgb; a.amax = amax;
    a.inset = inset; a.ih = ih; a.iw = iw; a.ix0 = ix0; a.iy0 = iy0; a.zoom = zoom; a.mirror = mirror ? 1 : 0;
    a.frame_valid = frame_valid;
    const dim3 grid((unsigned)(a.items < OV_MAX_BLOCKS ? a.items : OV_MAX_BLOCKS));
    // then every row, plane and frame of both buffers starts where the widest access of its format needs it
    const bool vec = IW % OV_COLS == 0 && IH % 2 == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
    switch (in_format) {
        OV_OUT_CASES(EVE_PIX_RGB, "rgb")
        OV_OUT_CASES(EVE_PIX_RGBA, "rgba")
        OV_OUT_CASES(EVE_PIX_BGR, "bgr")
        OV_OUT_CASES(EVE_PIX_BGRA, "bgra")
        OV_OUT_CASES(EVE_PIX_NV12, "nv12")
        OV_OUT_CASES(EVE_PIX_I420, "i420")
        OV_OUT_CASES(EVE_PIX_YUYV, "yuyv")
    }
    EVE_CHECK_LAUNCH();
    return 0;
}
