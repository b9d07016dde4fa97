// Screen luminance on the device (include/eve_hip.h eve_screen_luminance): the mean relative luminance of every delivered capture,
// over the whole visible region and over up to four concentric discs around a per-frame centre, computed per pixel at capture
// resolution -- read through the surface's address rule (surface.h), converted (yuv_rgb.h), linearised through a display response
// table, weighted, summed.  Integers up to one float64 division, so the bits do not depend on the grid, the band height or the
// order of the sums (tests/screen_luminance_ref.py has it in numpy).
//
// The kernel is one read stream over the surfaces as they lie.  A workgroup takes one (frame, band of LUM_BAND_ROWS rows):
//   1. the table goes to LDS once per workgroup, each entry multiplied by its channel's weight (3 x 256 dwords: k_c * response[c][v]
//      <= 65536 * 65535 fits 32 bits, and so does the sum of three with the rounding term), so a pixel is three LDS reads, two adds
//      and a shift;
//   2. each thread walks its columns of the band through one of screen_area_surface_kernel's three load forms and keeps its sums
//      in 32 bits: a band gives a thread at most LUM_BAND_ROWS * 16384 / 256 = 2048 pixels of at most 65535 each, far below the
//      65536 pixels a 32-bit sum takes.  Whether the band's rows meet the largest disc's rows is uniform over the workgroup:
//      a band that does not -- most of them -- runs the loop without a disc test, and in one that does a thread whose columns lie
//      outside the disc's bounding box skips it;
//   3. the sums are widened to 64 bits, reduced across the wave and across the four waves in LDS, and one thread adds the 1 + R
//      pairs to sums / counts with integer atomics.  The entry point zeroes both on the stream first.
// screen_luminance_finish_kernel then writes the means.  No workgroup waits on another.
#include "common.h"
#include "surface.h"
#include "yuv_rgb.h"

namespace eve {
namespace {

constexpr int LUM_THREADS = 256;
constexpr int LUM_BAND_ROWS = 32;        // rows of a band (even: a band starts on a chroma row); kernels.py mirrors it for the tests
constexpr int LUM_ROWS = 8;              // generic form: rows whose loads one thread keeps in flight
constexpr int LUM_GROUPS = 4;            // yuv420 forms: row pairs whose loads one thread keeps in flight
constexpr int LUM_MAX_SIDE = 16384;
constexpr int LUM_MAX_DISCS = 4;
constexpr long long LUM_MAX_BLOCKS = 1 << 20;      // (frame, band) items beyond that are taken in a grid-stride loop
constexpr int LUM_Q_MAX = 1 << 20;       // |q| beyond that: no disc (keeps every difference far inside 32 bits)
static_assert(LUM_BAND_ROWS % 2 == 0 && (long long)LUM_BAND_ROWS * LUM_MAX_SIDE / LUM_THREADS <= 65536, "a thread's 32-bit sums");

struct LumArgs {
    long long items;                     // frames * bands
    int IH, IW, T, R, bands;
    int yuv;                             // generic: the kind is EVE_SURF_YUV
    int planar, skew;                    // yuv420: as SurfAreaArgs'
    int kr, kg, kb;
    float sx, sy;
    uint32_t two_r_max;                  // 2 * radii[R - 1] <= 2^15
    uint32_t four_r2[LUM_MAX_DISCS];     // 4 * r_k^2 <= 2^30 (k < R)
    YuvCoef coef;
    Surf sf;
};

// a thread's sums over its pixels of one band
struct LumAcc {
    uint32_t sum;
    uint32_t dsum[LUM_MAX_DISCS], dcnt[LUM_MAX_DISCS];
};

// the disc's centre of one frame, in half pixels
struct LumCentre {
    int qx, qy;
};

// do columns x_lo .. x_hi (a thread's columns: fixed over the band's rows) meet the largest disc's bounding box?
__device__ __forceinline__ bool lum_near(const LumArgs& a, const LumCentre& q, const int x_lo, const int x_hi) {
    return 2 * x_lo + 1 - q.qx <= (int)a.two_r_max && q.qx - (2 * x_hi + 1) <= (int)a.two_r_max;
}

// near: lum_near of the thread's columns; where it is false the pixel is in no disc and the test is skipped
template <bool DISC>
__device__ __forceinline__ void lum_add(LumAcc& acc, const uint32_t* tab, const LumArgs& a, const LumCentre& q, const bool near, const int X,
                                        const int Y, const uint32_t (&rgb)[3]) {
    const uint32_t y = (tab[rgb[0]] + tab[256 + rgb[1]] + tab[512 + rgb[2]] + 32768u) >> 16;
    acc.sum += y;
    if constexpr (DISC) {
        if (!near) return;
        // The contract's 64-bit test in 32 bits: |q| <= 2^20 keeps the differences in an int; a pixel outside the largest disc's
        // bounding box is in no disc, and inside it both squares are <= (2 * 16384)^2 = 2^30, their sum <= 2^31.
        const int dx = 2 * X + 1 - q.qx, dy = 2 * Y + 1 - q.qy;
        const uint32_t ax = (uint32_t)(dx < 0 ? -dx : dx), ay = (uint32_t)(dy < 0 ? -dy : dy);
        if (ax <= a.two_r_max && ay <= a.two_r_max) {
            const uint32_t dd = ax * ax + ay * ay;
#pragma unroll
            for (int k = 0; k < LUM_MAX_DISCS; ++k) {
                const bool in = k < a.R && dd <= a.four_r2[k];
                acc.dsum[k] += in ? y : 0u;
                acc.dcnt[k] += in ? 1u : 0u;
            }
        }
    }
}

// rows [y0, y1) of one frame, y0 even: the 8-bit 4:2:0 forms (surf_area_yuv420_items' loads without the row weights)
template <bool VEC, bool DISC>
__device__ __forceinline__ void lum_band_yuv420(LumAcc& acc, const uint32_t* tab, const LumArgs& a, const LumCentre& q,
                                                const uint8_t* __restrict__ frame, const int y0, const int y1) {
    const int tid = threadIdx.x;
    const int IW = a.IW;
    const YuvCoef coef = a.coef;
    const long long oY = a.sf.offset[0], oU = a.sf.offset[1], oV = a.sf.offset[2];
    const long long pY = a.sf.pitch[0], pU = a.sf.pitch[1], pV = a.sf.pitch[2];
    const bool planar = a.planar != 0;
    const bool v_first = oV < oU;                                            // interleaved: NV21's order
    const long long oC = v_first ? oV : oU;                                  // interleaved: where a row's chroma pairs begin
    const int g0 = y0 / 2, g1 = (y1 + 1) / 2;                                // row pairs: <= (IH + 1) / 2
    if constexpr (VEC) {
        const int skew = a.skew;
        for (int v = tid; v < (skew + IW + SURF_VEC_COLS - 1) / SURF_VEC_COLS; v += LUM_THREADS) {
            const int x0 = v * SURF_VEC_COLS - skew;                         // the group's first column: >= -6, even
            const bool near = DISC && lum_near(a, q, x0, x0 + SURF_VEC_COLS - 1);
            for (int g = g0; g < g1; g += LUM_GROUPS) {
                uint32_t yq[LUM_GROUPS][2][2];                               // the group's two luma rows, 8 columns each
                uint32_t cq[LUM_GROUPS][2];                                  // interleaved: 4 chroma pairs; planar: 4 U bytes, 4 V bytes
#pragma unroll
                for (int i = 0; i < LUM_GROUPS; ++i)
                    if (g + i < g1) {
#pragma unroll
                        for (int r = 0; r < 2; ++r) {
                            const int iy = (g + i) * 2 + r;
                            if (iy < y1) load_words(frame + oY + iy * pY + x0, yq[i][r]);
                            else yq[i][r][0] = yq[i][r][1] = 0u;             // below an odd height's last row: never summed
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
                for (int i = 0; i < LUM_GROUPS; ++i)
                    if (g + i < g1) {
                        const int iya = (g + i) * 2;
                        const uint32_t even = every_second_byte<false>(cq[i][0], cq[i][1]), odd = every_second_byte<true>(cq[i][0], cq[i][1]);
                        const uint32_t uw = planar ? cq[i][0] : v_first ? odd : even;
                        const uint32_t vw = planar ? cq[i][1] : v_first ? even : odd;
#pragma unroll
                        for (int j = 0; j < SURF_VEC_COLS / 2; ++j) {        // chroma sample j: luma columns 2j, 2j + 1 of both rows
                            const YuvChroma c = yuv_chroma<true>((int)((uw >> (8 * j)) & 0xffu), (int)((vw >> (8 * j)) & 0xffu), coef);
#pragma unroll
                            for (int e = 0; e < 2; ++e) {
                                const int X = x0 + 2 * j + e;
                                if (X >= 0 && X < IW) {                      // a skewed or partial group: the visible columns only
#pragma unroll
                                    for (int r = 0; r < 2; ++r)
                                        if (iya + r < y1) {
                                            uint32_t rgb[3];
                                            yuv_pixel<true>((int)byte_of(yq[i][r], 2 * j + e), c, coef, rgb);
                                            lum_add<DISC>(acc, tab, a, q, near, X, iya + r, rgb);
                                        }
                                }
                            }
                        }
                    }
            }
        }
    } else {
        const long long sY = a.sf.step[0], sU = a.sf.step[1], sV = a.sf.step[2];
        for (int p = tid; p < ((IW + 1) >> 1); p += LUM_THREADS) {           // pixel pair p: columns 2p, 2p + 1, one chroma sample
            const bool second = 2 * p + 1 < IW;                              // an odd width's last pair is one column
            const bool near = DISC && lum_near(a, q, 2 * p, 2 * p + 1);
            for (int g = g0; g < g1; g += LUM_GROUPS) {
                uint32_t yb[LUM_GROUPS][2][2], ub[LUM_GROUPS], vb[LUM_GROUPS];
#pragma unroll
                for (int i = 0; i < LUM_GROUPS; ++i)
                    if (g + i < g1) {
#pragma unroll
                        for (int r = 0; r < 2; ++r) {
                            const int iy = (g + i) * 2 + r;
                            yb[i][r][0] = yb[i][r][1] = 0u;
                            if (iy < y1) {
                                const uint8_t* p0 = frame + oY + iy * pY + (long long)(2 * p) * sY;
                                yb[i][r][0] = p0[0];
                                if (second) yb[i][r][1] = p0[sY];
                            }
                        }
                        ub[i] = frame[oU + (g + i) * pU + p * sU];
                        vb[i] = frame[oV + (g + i) * pV + p * sV];
                    }
#pragma unroll
                for (int i = 0; i < LUM_GROUPS; ++i)
                    if (g + i < g1) {
                        const YuvChroma c = yuv_chroma<true>((int)ub[i], (int)vb[i], coef);
#pragma unroll
                        for (int r = 0; r < 2; ++r) {
                            const int iy = (g + i) * 2 + r;
                            if (iy < y1) {
#pragma unroll
                                for (int e = 0; e < 2; ++e)
                                    if (e == 0 || second) {
                                        uint32_t rgb[3];
                                        yuv_pixel<true>((int)yb[i][r][e], c, coef, rgb);
                                        lum_add<DISC>(acc, tab, a, q, near, 2 * p + e, iy, rgb);
                                    }
                            }
                        }
                    }
            }
        }
    }
}

// rows [y0, y1) of one frame: every other descriptor, three byte loads per pixel through the address rule
template <bool DISC>
__device__ __forceinline__ void lum_band_generic(LumAcc& acc, const uint32_t* tab, const LumArgs& a, const LumCentre& q,
                                                 const uint8_t* __restrict__ frame, const int y0, const int y1) {
    const YuvCoef coef = a.coef;
    const Surf sf = a.sf;
    for (int x = threadIdx.x; x < a.IW; x += LUM_THREADS) {
        const bool near = DISC && lum_near(a, q, x, x);
        for (int iy = y0; iy < y1; iy += LUM_ROWS) {
            uint32_t b[LUM_ROWS][3];
#pragma unroll
            for (int r = 0; r < LUM_ROWS; ++r)
                if (iy + r < y1) surf_components(frame, sf, iy + r, x, b[r]);
#pragma unroll
            for (int r = 0; r < LUM_ROWS; ++r)
                if (iy + r < y1) {
                    uint32_t rgb[3] = {b[r][0], b[r][1], b[r][2]};
                    if (a.yuv) yuv_pixel<true>((int)b[r][0], yuv_chroma<true>((int)b[r][1], (int)b[r][2], coef), coef, rgb);
                    lum_add<DISC>(acc, tab, a, q, near, x, iy + r, rgb);
                }
        }
    }
}

constexpr int LUM_YUV420 = 0, LUM_GENERIC = 1;

__device__ __forceinline__ unsigned long long lum_wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// FORM: LUM_YUV420 (VEC: its vector form) or LUM_GENERIC (the byte form only)
template <int FORM, bool VEC>
__global__ __launch_bounds__(LUM_THREADS) void screen_luminance_kernel(const LumArgs a, const uint8_t* __restrict__ src,
                                                                       const uint16_t* __restrict__ response, const int* __restrict__ lengths,
                                                                       const float* __restrict__ centres,
                                                                       const uint8_t* __restrict__ centre_valid,
                                                                       unsigned long long* __restrict__ sums, int* __restrict__ counts) {
    __shared__ uint32_t tab[3 * 256];                                        // k_c * response[c][v]
    __shared__ unsigned long long red_sum[LUM_THREADS / 64][1 + LUM_MAX_DISCS];
    __shared__ uint32_t red_cnt[LUM_THREADS / 64][LUM_MAX_DISCS];
    const int tid = threadIdx.x;
    for (int i = tid; i < 3 * 256; i += LUM_THREADS)
        tab[i] = (uint32_t)(i < 256 ? a.kr : i < 512 ? a.kg : a.kb) * (uint32_t)response[i];
    __syncthreads();
    for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
        const long long n = item / a.bands;
        const int band = (int)(item - n * a.bands);
        if (lengths) {                                                       // an undelivered frame: its bytes are not read
            const long long b = n / a.T;
            const int f = (int)(n - b * a.T), len = lengths[b];
            if (f >= (len < 0 ? 0 : len > a.T ? a.T : len)) continue;        // (uniform over the workgroup)
        }
        const int y0 = band * LUM_BAND_ROWS, y1 = y0 + LUM_BAND_ROWS < a.IH ? y0 + LUM_BAND_ROWS : a.IH;
        // the frame's centre in half pixels, the overlay's way; no address is computed from it
        LumCentre q = {0, 0};
        bool disc = false;
        if (a.R > 0 && (!centre_valid || centre_valid[n] != 0)) {
            const float fx = rintf(__fmul_rn(__fmul_rn(centres[2 * n], a.sx), 2.f)), fy = rintf(__fmul_rn(__fmul_rn(centres[2 * n + 1], a.sy), 2.f));
            if (fabsf(fx) <= (float)LUM_Q_MAX && fabsf(fy) <= (float)LUM_Q_MAX) {       // (false for a NaN)
                q.qx = (int)fx; q.qy = (int)fy;
                // do the band's rows meet the largest disc's rows?  |2Y + 1 - qy| <= 2 r for some Y in [y0, y1)
                disc = 2 * y0 + 1 - q.qy <= (int)a.two_r_max && q.qy - (2 * y1 - 1) <= (int)a.two_r_max;
            }
        }
        LumAcc acc;
        acc.sum = 0u;
#pragma unroll
        for (int k = 0; k < LUM_MAX_DISCS; ++k) acc.dsum[k] = acc.dcnt[k] = 0u;
        const uint8_t* frame = src + n * a.sf.frame_stride;
        if (disc) {
            if constexpr (FORM == LUM_YUV420) lum_band_yuv420<VEC, true>(acc, tab, a, q, frame, y0, y1);
            else lum_band_generic<true>(acc, tab, a, q, frame, y0, y1);
        } else {
            if constexpr (FORM == LUM_YUV420) lum_band_yuv420<VEC, false>(acc, tab, a, q, frame, y0, y1);
            else lum_band_generic<false>(acc, tab, a, q, frame, y0, y1);
        }
        // widen, reduce across the wave, then across the waves
        const int wave = tid >> 6, lane = tid & 63;
        const unsigned long long s0 = lum_wave_sum(acc.sum);
        if (lane == 0) red_sum[wave][0] = s0;
        if (disc) {
#pragma unroll
            for (int k = 0; k < LUM_MAX_DISCS; ++k) {
                const unsigned long long s = lum_wave_sum(acc.dsum[k]), c = lum_wave_sum(acc.dcnt[k]);
                if (lane == 0) { red_sum[wave][1 + k] = s; red_cnt[wave][k] = (uint32_t)c; }
            }
        }
        __syncthreads();
        if (tid == 0) {
            const long long at = n * (1 + a.R);
            unsigned long long s = 0;
            for (int w = 0; w < LUM_THREADS / 64; ++w) s += red_sum[w][0];
            atomicAdd(sums + at, s);
            atomicAdd(counts + at, a.IW * (y1 - y0));
            if (disc)
                for (int k = 0; k < a.R; ++k) {
                    unsigned long long sk = 0;
                    uint32_t ck = 0u;
                    for (int w = 0; w < LUM_THREADS / 64; ++w) { sk += red_sum[w][1 + k]; ck += red_cnt[w][k]; }
                    if (ck) {
                        atomicAdd(sums + at + 1 + k, sk);
                        atomicAdd(counts + at + 1 + k, (int)ck);
                    }
                }
        }
        __syncthreads();                 // the next item overwrites the partial sums
    }
}

__global__ __launch_bounds__(LUM_THREADS) void screen_luminance_finish_kernel(const long long total, const unsigned long long* __restrict__ sums,
                                                                              const int* __restrict__ counts, float* __restrict__ mean) {
    const long long i = (long long)blockIdx.x * LUM_THREADS + threadIdx.x;
    if (i < total) mean[i] = (float)((double)sums[i] / ((double)counts[i] * 65535.0));      // a zero count: 0 / 0 = NaN
}

__host__ bool lum_positive(const float x) { return x > 0.f && x <= 3.40282346638528859812e38f; }

}  // namespace
}  // namespace eve

using namespace eve;

extern "C" int eve_screen_luminance(const eve_surface* surface, int matrix, long long B, int T, const uint8_t* src, const uint16_t* response,
                                    int kr, int kg, int kb, const int* lengths, int R, const int* radii, const float* centres, float sx,
                                    float sy, const uint8_t* centre_valid, unsigned long long* sums, int* counts, float* mean,
                                    eve_stream_t stream) {
    static const char who[] = "screen_luminance";
    char msg[192];
    const long long LIM = 0x7fffffff;
    const char* why = nullptr;
    if (B < 1 || T < 1) why = "B >= 1 and T >= 1";
    else if (R < 0 || R > LUM_MAX_DISCS) why = "R must lie in 0 .. 4";
    else if (B > LIM / T / (1 + R)) why = "B * T * (1 + R) must fit 31 bits";
    else why = surface_refusal(surface, matrix, B * T);
    if (why) {}
    else if (surface->width > LUM_MAX_SIDE || surface->height > LUM_MAX_SIDE) why = "frame too large (width, height <= 16384)";
    else if (!src || !response || !sums || !counts || !mean) why = "bad arguments";
    else if (kr < 0 || kg < 0 || kb < 0 || (long long)kr + kg + kb != 65536) why = "the weights must be >= 0 and sum to 65536";
    else if ((R > 0) != (radii != nullptr)) why = "radii come with R > 0, and only then";
    else if ((R > 0) != (centres != nullptr)) why = "centres come with R > 0, and only then";
    else if (!lum_positive(sx) || !lum_positive(sy)) why = "sx and sy must be finite numbers > 0";
    else
        for (int k = 0; k < R; ++k)
            if (radii[k] < 1 || radii[k] > LUM_MAX_SIDE || (k && radii[k] <= radii[k - 1])) why = "radii must lie in 1 .. 16384 and increase strictly";
    if (why) {
        snprintf(msg, sizeof(msg), "%s: %s", who, why);
        return set_error_msg(msg);
    }
    const eve_surface& s = *surface;
    const long long N = B * T, total = N * (1 + R);
    LumArgs a;
    a.IH = s.height; a.IW = s.width; a.T = T; a.R = R;
    a.bands = (s.height + LUM_BAND_ROWS - 1) / LUM_BAND_ROWS;
    a.items = N * a.bands;
    a.yuv = s.kind == EVE_SURF_YUV;
    a.coef = YUV_MATRICES[a.yuv ? matrix : 0];
    a.sf = surf_of(s);
    a.kr = kr; a.kg = kg; a.kb = kb;
    a.sx = sx; a.sy = sy;
    a.two_r_max = R ? 2u * (uint32_t)radii[R - 1] : 0u;
    for (int k = 0; k < LUM_MAX_DISCS; ++k) a.four_r2[k] = k < R ? 4u * (uint32_t)radii[k] * (uint32_t)radii[k] : 0u;
    const SurfForm form = surf_form(s, N, src);
    a.planar = form.planar;
    a.skew = form.skew;
    hipError_t e = hipMemsetAsync(sums, 0, (size_t)total * sizeof(unsigned long long), (hipStream_t)stream);
    if (e == hipSuccess) e = hipMemsetAsync(counts, 0, (size_t)total * sizeof(int), (hipStream_t)stream);
    if (e != hipSuccess) return set_error(e, __func__);
    const dim3 grid((unsigned)(a.items < LUM_MAX_BLOCKS ? a.items : LUM_MAX_BLOCKS)), block(LUM_THREADS);
    if (form.yuv420 && form.vec)
        EVE_LAUNCH("screen_luminance_kernel<yuv420,true>", (screen_luminance_kernel<LUM_YUV420, true>), grid, block, 0, (hipStream_t)stream, a,
                   src, response, lengths, centres, centre_valid, sums, counts);
    else if (form.yuv420)
        EVE_LAUNCH("screen_luminance_kernel<yuv420,false>", (screen_luminance_kernel<LUM_YUV420, false>), grid, block, 0, (hipStream_t)stream, a,
                   src, response, lengths, centres, centre_valid, sums, counts);
    else
        EVE_LAUNCH("screen_luminance_kernel<generic,false>", (screen_luminance_kernel<LUM_GENERIC, false>), grid, block, 0, (hipStream_t)stream, a,
                   src, response, lengths, centres, centre_valid, sums, counts);
    const char* form_name = g_last_kernel;
    EVE_LAUNCH("screen_luminance_finish_kernel", screen_luminance_finish_kernel, dim3((unsigned)((total + LUM_THREADS - 1) / LUM_THREADS)), block,
               0, (hipStream_t)stream, total, sums, counts, mean);
    g_last_kernel = form_name;           // eve_last_kernel names the form that read the frames
    EVE_CHECK_LAUNCH();
    return 0;
}
