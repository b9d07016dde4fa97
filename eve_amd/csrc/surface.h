// A decoder's or capture API's surface (include/eve_hip.h eve_surface): a frame addressed through plane offsets, pitches and sample
// steps in place of a byte-linear layout.  The whole contract is one address rule -- component c of pixel (x, y) is the byte
//   frame + offset[c] + (y >> ys) * pitch[c] + (x >> xs) * step[c]         xs = ys = 0 for component 0 and for EVE_SURF_RGB
// in 64-bit arithmetic -- so NV12 / NV21, I420 / YV12, YUYV / UYVY, P010's high bytes, pitched BGRA and every crop of them are
// numbers in the descriptor, not kernels.  This header holds what the eye-patch warp, the screen area resize and the screen luminance share: the part
// of the descriptor a kernel reads (by value in its arguments, uniform over the launch), the address rule for one pixel and for the 2 x 2 taps of a bilinear sample, and the host-side refusals.
#pragma once
#include "common.h"
#include "yuv_rgb.h"

namespace eve {

// what a kernel needs of an eve_surface; width and height travel with the kernel's own IW and IH
struct Surf {
    long long frame_stride;
    long long offset[3];
    int pitch[3];
    int step[3];
    int xshift, yshift;
};

inline Surf surf_of(const eve_surface& s) {
    Surf d;
    d.frame_stride = s.frame_stride;
    for (int c = 0; c < 3; ++c) { d.offset[c] = s.offset[c]; d.pitch[c] = s.pitch[c]; d.step[c] = s.step[c]; }
    d.xshift = s.xshift; d.yshift = s.yshift;
    return d;
}

// the three component bytes of pixel (y, x), 0 <= y < height, 0 <= x < width, of one frame: the address rule, three byte loads
__device__ __forceinline__ void surf_components(const uint8_t* __restrict__ frame, const Surf& s, const int y, const int x, uint32_t (&v)[3]) {
    const long long ys = y >> s.yshift, xs = x >> s.xshift;
    v[0] = frame[s.offset[0] + (long long)y * s.pitch[0] + (long long)x * s.step[0]];
    v[1] = frame[s.offset[1] + ys * s.pitch[1] + xs * s.step[1]];
    v[2] = frame[s.offset[2] + ys * s.pitch[2] + xs * s.step[2]];
}

// The same addresses for the 2 x 2 taps of a bilinear sample at rows y0, y0 + 1 and columns x0, x0 + 1, split into a row term
// (offset included) and a column term per component: tap (i, j) reads component c at frame[row[i][c] + col[j][c]].  A coordinate
// of -1 or of the frame's size gives a term no tap inside the frame uses.
template <bool YUV>
__device__ __forceinline__ void surf_tap_terms(const Surf& s, const int y0, const int x0, long long (&row)[2][3], long long (&col)[2][3]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int y = y0 + i, x = x0 + i;
        const long long yc = YUV ? y >> s.yshift : y, xc = YUV ? x >> s.xshift : x;
        row[i][0] = s.offset[0] + (long long)y * s.pitch[0];
        col[i][0] = (long long)x * s.step[0];
#pragma unroll
        for (int c = 1; c < 3; ++c) {
            row[i][c] = s.offset[c] + yc * s.pitch[c];
            col[i][c] = xc * s.step[c];
        }
    }
}

// ---- the wide loads of the 8-bit 4:2:0 vector form, shared by the screen area resize and the screen luminance
constexpr int SURF_VEC_COLS = 8;           // luma columns a thread of the vector form owns: one 8-byte load per row

// W = 1, 2 or 4 dwords from p (aligned to 4 * W bytes) as one load
template <int W>
__device__ __forceinline__ void load_words(const uint8_t* __restrict__ p, uint32_t (&w)[W]) {
    static_assert(W == 1 || W == 2 || W == 4, "one dword, dwordx2 or dwordx4 load");
    if constexpr (W == 4) {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
    } else if constexpr (W == 2) {
        const uint2 q = *reinterpret_cast<const uint2*>(p);
        w[0] = q.x; w[1] = q.y;
    } else {
        w[0] = *reinterpret_cast<const uint32_t*>(p);
    }
}

template <int W>
__device__ __forceinline__ uint32_t byte_of(const uint32_t (&w)[W], const int k) { return (w[k >> 2] >> (8 * (k & 3))) & 0xffu; }

// bytes 0 and 2 of lo, then of hi (ODD: bytes 1 and 3): every second byte of eight
template <bool ODD>
__device__ __forceinline__ uint32_t every_second_byte(const uint32_t lo, const uint32_t hi) {
    constexpr int s = ODD ? 8 : 0;
    return ((lo >> s) & 0xffu) | (((lo >> (16 + s)) & 0xffu) << 8) | (((hi >> s) & 0xffu) << 16) | (((hi >> (16 + s)) & 0xffu) << 24);
}

// Which load form N frames of a (checked) descriptor at `src` take.  yuv420: 8-bit 4:2:0 with luma step 1 and chroma either
// interleaved (U and V one byte apart, step 2, one pitch) or in two planes (step 1).  vec: its vector form -- 8 luma bytes and 8
// interleaved chroma bytes (planar: 4 + 4) per load, each load on its own size in every row of every frame.  The loads start `skew`
// bytes below pixel (0, 0) and end on the boundary behind the row's last pixel: every plane must hold those bytes inside
// [0, frame_bytes), and luma and chroma must share the skew.
struct SurfForm {
    bool yuv420, planar, vec;
    int skew;
};

inline SurfForm surf_form(const eve_surface& s, const long long N, const uint8_t* src) {
    SurfForm f = {false, false, false, 0};
    const int IH = s.height, IW = s.width;
    const long long duv = s.offset[2] - s.offset[1];
    const bool semi = s.step[1] == 2 && s.step[2] == 2 && (duv == 1 || duv == -1) && s.pitch[1] == s.pitch[2];
    f.planar = s.step[1] == 1 && s.step[2] == 1;
    f.yuv420 = s.kind == EVE_SURF_YUV && s.xshift == 1 && s.yshift == 1 && s.step[0] == 1 && (semi || f.planar) && IW >= 2;
    if (!f.yuv420) return f;
    const uintptr_t base = reinterpret_cast<uintptr_t>(src);
    const int skew = (int)((base + (uintptr_t)s.offset[0]) & (SURF_VEC_COLS - 1));
    const long long span = (skew + (long long)IW + SURF_VEC_COLS - 1) / SURF_VEC_COLS * SURF_VEC_COLS;      // bytes of luma a row's groups cover
    const long long crows = (IH + 1) / 2;
    const auto plane_ok = [&](long long offset, int pitch, long long rows, int bytes, int skew_c, long long span_c) {
        return (int)((base + (uintptr_t)offset) & (bytes - 1)) == skew_c && pitch % bytes == 0 && (N == 1 || s.frame_stride % bytes == 0) &&
               offset >= skew_c && offset - skew_c + (rows - 1) * pitch + span_c <= s.frame_bytes;
    };
    const long long oc = duv > 0 ? s.offset[1] : s.offset[2];
    f.vec = skew % 2 == 0 && plane_ok(s.offset[0], s.pitch[0], IH, SURF_VEC_COLS, skew, span) &&
            (f.planar ? plane_ok(s.offset[1], s.pitch[1], crows, SURF_VEC_COLS / 2, skew / 2, span / 2) &&
                            plane_ok(s.offset[2], s.pitch[2], crows, SURF_VEC_COLS / 2, skew / 2, span / 2)
                      : plane_ok(oc, s.pitch[1], crows, SURF_VEC_COLS, skew, span));
    if (f.vec) f.skew = skew;
    return f;
}

constexpr int SURF_MAX_SIDE = 1 << 24;    // keeps every product of the bound check far inside 64 bits; the kernels ask for less

// what is wrong with the descriptor itself for N frames, or nullptr: everything that can be told without the kernel's own limits
inline const char* surface_refusal(const eve_surface* s, const int matrix, const long long N) {
    if (!s) return "bad arguments";
    if (s->struct_bytes != (int)sizeof(eve_surface)) return "struct_bytes is not sizeof(eve_surface)";
    if (s->kind != EVE_SURF_RGB && s->kind != EVE_SURF_YUV) return "unknown kind (EVE_SURF_RGB or EVE_SURF_YUV)";
    if (s->kind == EVE_SURF_YUV && (matrix < EVE_YUV_BT601 || matrix > EVE_YUV_JFIF)) return "unknown matrix (EVE_YUV_BT601, _BT709 or _JFIF)";
    if (s->xshift < 0 || s->xshift > 1 || s->yshift < 0 || s->yshift > 1) return "xshift and yshift must be 0 or 1";
    if (s->kind == EVE_SURF_RGB && (s->xshift || s->yshift)) return "xshift and yshift must be 0 for EVE_SURF_RGB";
    if (s->width <= 0 || s->height <= 0 || s->width > SURF_MAX_SIDE || s->height > SURF_MAX_SIDE) return "bad arguments";
    for (int c = 0; c < 3; ++c) {
        if (s->pitch[c] < 1 || s->step[c] < 1) return "every pitch and step must be >= 1";
        if (s->offset[c] < 0) return "an offset is negative";
    }
    for (int c = 0; c < 3; ++c) {
        const int xs = c ? s->xshift : 0, ys = c ? s->yshift : 0;
        const long long last = s->offset[c] + (long long)((s->height - 1) >> ys) * s->pitch[c] + (long long)((s->width - 1) >> xs) * s->step[c];
        if (last >= s->frame_bytes) return "a component's last addressed byte lies at or beyond frame_bytes";
    }
    if (N > 1 && s->frame_bytes > s->frame_stride) return "frame_bytes exceeds frame_stride with N > 1";
    return nullptr;
}

}  // namespace eve
