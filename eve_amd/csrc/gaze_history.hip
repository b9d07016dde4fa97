// The time-decayed gaze history ("where has this person been looking"), on the device: per stream the recurrence
// M_t = decay^(dt_ms) * M_{t-1} + w_t * G_t over a float32 map, G_t the Gaussian around the frame's point of gaze (or the network's own
// heat map).  One read and one write of the map per chunk, however many frames the chunk holds.  The contract -- operation order, the
// exp and the state row included -- is in include/eve_hip.h (eve_gaze_history_plan / _update) and in numpy in tests/gaze_history_ref.py.
//
// Two launches, because no workgroup of the map launch may both read and write the state row (a single launch would race across
// workgroups):
//   gaze_history_plan_kernel     one wavefront per stream, passes of 64 frames: lane t reads frame t's inputs, lane 0 walks the time
//                                chain (no transcendental), lane t forms its frame's decay factor and writes the coefficient row
//                                (d, w, cx, cy) -- d = -1: the frame is ignored; w = -1: it decays and deposits nothing
//   gaze_history_update_kernel   grid (map tiles, B), a 64 x 32 tile per 256-thread workgroup, four consecutive pixels in each of two
//                                rows per thread (16-byte loads and stores where the rows allow).  The pixels stay in registers over all the
//                                frames; per pass of 16 frames the workgroup fills LDS tables of the tile's column and row factors
//                                (64 + 32 exp evaluations per frame), so a pixel costs five float64 operations and a convert per frame.
// Float64 throughout, every operation rounded on its own: the bits do not depend on this structure.
#include "common.h"

#pragma clang fp contract(off)

namespace eve {
namespace {

constexpr int GH_WAVE = 64;
constexpr int GH_STATE = 8;              // doubles per state row: has_prev, t_prev, ticks, 5 reserved
constexpr int GH_TW = 64, GH_TH = 32;    // the update's tile
constexpr int GH_PX = 4;                 // consecutive pixels of a row per thread ...
constexpr int GH_RY = 2;                 // ... in each of this many rows, GH_TH / GH_RY apart
constexpr int GH_THREADS = (GH_TW / GH_PX) * (GH_TH / GH_RY);
constexpr int GH_PASS = 16;              // frames per fill of the LDS tables
constexpr double GH_TINY = 7.888609052210118e-31;      // 2^-100

__device__ __forceinline__ bool gh_finite(const double x) { return fabs(x) <= 1.79769313486231570815e308; }      // false for a NaN

// exp(x) for x <= 0, the contract's own: every operation rounded once, so the host restatement has the same bits
__device__ __forceinline__ double gh_exp(const double x) {
#pragma clang fp contract(off)
    const double xc = x < -104.0 ? -104.0 : x;
    const double k = rint(xc * 1.4426950408889634);
    const double r = (xc - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10;
    double p = 1.6059043836821613e-10;
    p = p * r + 2.08767569878681e-09;
    p = p * r + 2.505210838544172e-08;
    p = p * r + 2.755731922398589e-07;
    p = p * r + 2.7557319223985893e-06;
    p = p * r + 2.48015873015873e-05;
    p = p * r + 0.0001984126984126984;
    p = p * r + 0.001388888888888889;
    p = p * r + 0.008333333333333333;
    p = p * r + 0.041666666666666664;
    p = p * r + 0.16666666666666666;
    p = p * r + 0.5;
    p = p * r + 1.0;
    p = p * r + 1.0;
    const double e = ldexp(p, gh_finite(k) ? (int)k : 0);
    return x < -104.0 ? 0.0 : e;
}

struct GhPlan {
    double fps, ln_decay, max_gap, gain, sx, sy;
    int seconds, has_fps;
};

__global__ __launch_bounds__(GH_WAVE) void gaze_history_plan_kernel(const int T, const float* __restrict__ pog,
                                                                    const double* __restrict__ frame_time, const uint8_t* __restrict__ valid,
                                                                    const uint8_t* __restrict__ valid2, const int* __restrict__ lengths,
                                                                    const int* __restrict__ reset, const GhPlan P, double* __restrict__ state,
                                                                    double* __restrict__ coef, int* __restrict__ clear) {
#pragma clang fp contract(off)
    __shared__ double st[GH_STATE];
    __shared__ double s_tt[GH_WAVE], s_delta[GH_WAVE], s_w[GH_WAVE];
    __shared__ int s_flag[GH_WAVE];                                    // 0 ignored, 1 decays only, 2 deposits
    const int lane = threadIdx.x;
    const long long b = blockIdx.x;
    double* row = state + (size_t)b * GH_STATE;
    if (lane < GH_STATE) st[lane] = row[lane];
    __syncthreads();
    if (lane == 0) {
        const int rs = (reset && reset[b] != 0) ? 1 : 0;
        if (rs)
            for (int i = 0; i < GH_STATE; ++i) st[i] = 0.0;
        clear[b] = rs;
    }
    __syncthreads();
    int len = T;
    if (lengths) len = min(max(lengths[b], 0), T);
    const double ticks0 = st[2];
    for (int base = 0; base < T; base += GH_WAVE) {                    // (T, base: the same in every lane)
        const int f = base + lane;
        const long long n = b * T + f;
        // ---- parallel: the frame's time, point and validity
        int flag = 0;
        double cx = 0.0, cy = 0.0;
        if (f < len) {
            const double tt = frame_time ? frame_time[n] : (ticks0 + (double)f) / P.fps;
            bool usable = (!valid || valid[n] != 0) && (!valid2 || valid2[n] != 0);
            if (pog) {
                const double px = (double)pog[n * 2], py = (double)pog[n * 2 + 1];
                usable = usable && gh_finite(px) && gh_finite(py);
                cx = P.sx * px;
                cy = P.sy * py;
            }
            s_tt[lane] = tt;
            flag = gh_finite(tt) ? (usable ? 2 : 1) : 0;
        }
        s_flag[lane] = flag;
        __syncthreads();
        // ---- serial: the time chain
        if (lane == 0) {
            const int m = min(GH_WAVE, len - base);
            for (int t = 0; t < m; ++t) {
                if (s_flag[t] == 0) continue;
                const double tt = s_tt[t];
                const bool has_prev = st[0] != 0.0;
                if (has_prev && tt < st[1]) {
                    s_flag[t] = 0;
                    continue;
                }
                const double delta = has_prev ? tt - st[1] : 0.0;
                double wb = 1.0;
                if (P.seconds) wb = has_prev ? (P.max_gap < delta ? P.max_gap : delta) : (P.has_fps ? 1.0 / P.fps : 0.0);
                s_delta[t] = delta;
                s_w[t] = P.gain * wb;
                st[0] = 1.0;
                st[1] = tt;
            }
        }
        __syncthreads();
        // ---- parallel: the decay factor, the coefficient row
        if (f < T) {
            flag = s_flag[lane];
            double d = -1.0, w = 0.0;
            if (flag != 0) {
                d = gh_exp((s_delta[lane] * 1000.0) * P.ln_decay);
                w = flag == 2 ? s_w[lane] : -1.0;
            }
            double* c = coef + n * 4;
            c[0] = d;
            c[1] = w;
            c[2] = cx;
            c[3] = cy;
        }
        __syncthreads();
    }
    if (lane == 0) st[2] = ticks0 + (double)len;
    __syncthreads();
    if (lane < GH_STATE) row[lane] = st[lane];
}

template <bool VEC>
__global__ __launch_bounds__(GH_THREADS) void gaze_history_update_kernel(const int T, const int MH, const int MW, const int tiles_x,
                                                                         const double* __restrict__ coef, const int* __restrict__ clear,
                                                                         const float* __restrict__ heat, const double alpha,
                                                                         const double floor_, float* __restrict__ map,
                                                                         float* __restrict__ frames) {
#pragma clang fp contract(off)
    __shared__ double s_ex[GH_PASS][GH_TW], s_ey[GH_PASS][GH_TH], s_d[GH_PASS], s_w[GH_PASS];
    const int tid = threadIdx.x;
    const long long b = blockIdx.y;
    const int tile_x = (int)(blockIdx.x % (unsigned)tiles_x), tile_y = (int)(blockIdx.x / (unsigned)tiles_x);
    const int lx = (tid % (GH_TW / GH_PX)) * GH_PX, ly = tid / (GH_TW / GH_PX);
    const int x0 = tile_x * GH_TW + lx;
    const size_t plane = (size_t)MH * MW;
    bool row_in[GH_RY];                                                // (VEC: MW is a multiple of 4, so x0 < MW covers x0 + 3)
    size_t at[GH_RY];                                                  // used only where row_in
#pragma unroll
    for (int r = 0; r < GH_RY; ++r) {
        const int y = tile_y * GH_TH + ly + r * (GH_TH / GH_RY);
        row_in[r] = y < MH && x0 < MW;
        at[r] = (size_t)y * MW + x0;
    }
    float* mbase = map + (size_t)b * plane;
    const bool cleared = clear[b] != 0;
    if (T == 0 && !cleared) return;                                    // (uniform over the workgroup)
    float m[GH_RY][GH_PX];
#pragma unroll
    for (int r = 0; r < GH_RY; ++r) {
#pragma unroll
        for (int i = 0; i < GH_PX; ++i) m[r][i] = 0.0f;
        if (row_in[r] && !cleared) {
            if (VEC) {
                const float4 q = *reinterpret_cast<const float4*>(mbase + at[r]);
                m[r][0] = q.x, m[r][1] = q.y, m[r][2] = q.z, m[r][3] = q.w;
            } else {
#pragma unroll
                for (int i = 0; i < GH_PX; ++i)
                    if (x0 + i < MW) m[r][i] = mbase[at[r] + i];
            }
        }
    }
    for (int base = 0; base < T; base += GH_PASS) {                    // (T, base: the same in every thread)
        const int np = min(GH_PASS, T - base);
        __syncthreads();                                               // the tables of the pass before have been read
        if (tid < np) {
            const double* c = coef + ((size_t)b * T + base + tid) * 4;
            s_d[tid] = c[0];
            s_w[tid] = c[1];
        }
        if (!heat) {
            for (int idx = tid; idx < np * (GH_TW + GH_TH); idx += GH_THREADS) {
                const int f = idx / (GH_TW + GH_TH), j = idx % (GH_TW + GH_TH);
                const double* c = coef + ((size_t)b * T + base + f) * 4;
                if (c[0] < 0.0 || c[1] < 0.0) continue;                // ignored, or no deposit: the tables are not read
                if (j < GH_TW) {
                    const double dx = (double)(tile_x * GH_TW + j) - c[2];
                    s_ex[f][j] = gh_exp(alpha * (dx * dx));
                } else {
                    const double dy = (double)(tile_y * GH_TH + (j - GH_TW)) - c[3];
                    s_ey[f][j - GH_TW] = gh_exp(alpha * (dy * dy));
                }
            }
        }
        __syncthreads();
        for (int f = 0; f < np; ++f) {
            const double d = s_d[f], w = s_w[f];
            const size_t frame = ((size_t)b * T + base + f) * plane;
#pragma unroll
            for (int r = 0; r < GH_RY; ++r) {
                if (!row_in[r]) continue;
                if (d >= 0.0) {                                        // (d < 0: the frame is ignored, the map as it stands)
                    double g[GH_PX] = {0.0, 0.0, 0.0, 0.0};
                    if (w >= 0.0) {
                        if (heat) {
                            const float* h = heat + frame + at[r];
                            if (VEC) {
                                const float4 q = *reinterpret_cast<const float4*>(h);
                                g[0] = (double)q.x, g[1] = (double)q.y, g[2] = (double)q.z, g[3] = (double)q.w;
                            } else {
#pragma unroll
                                for (int i = 0; i < GH_PX; ++i)
                                    if (x0 + i < MW) g[i] = (double)h[i];
                            }
                        } else {
                            const double ey = s_ey[f][ly + r * (GH_TH / GH_RY)];
#pragma unroll
                            for (int i = 0; i < GH_PX; ++i) g[i] = s_ex[f][lx + i] * ey + floor_;
                        }
                    }
#pragma unroll
                    for (int i = 0; i < GH_PX; ++i) {
                        double v = (double)m[r][i] * d;
                        if (w >= 0.0) v = v + w * g[i];
                        m[r][i] = fabs(v) < GH_TINY ? 0.0f : (float)v;
                    }
                }
                if (frames) {
                    float* o = frames + frame + at[r];
                    if (VEC) {
                        *reinterpret_cast<float4*>(o) = make_float4(m[r][0], m[r][1], m[r][2], m[r][3]);
                    } else {
#pragma unroll
                        for (int i = 0; i < GH_PX; ++i)
                            if (x0 + i < MW) o[i] = m[r][i];
                    }
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < GH_RY; ++r) {
        if (!row_in[r]) continue;
        if (VEC) {
            *reinterpret_cast<float4*>(mbase + at[r]) = make_float4(m[r][0], m[r][1], m[r][2], m[r][3]);
        } else {
#pragma unroll
            for (int i = 0; i < GH_PX; ++i)
                if (x0 + i < MW) mbase[at[r] + i] = m[r][i];
        }
    }
}

__host__ bool gh_positive(const double x) { return x > 0.0 && x <= 1.79769313486231570815e308; }
__host__ bool gh_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace
}  // namespace eve

using namespace eve;

extern "C" int eve_gaze_history_plan(long long B, int T, const float* pog, const double* frame_time, const uint8_t* valid,
                                     const uint8_t* valid_key, const int* lengths, const int* reset, double fps, double ln_decay,
                                     int weight_seconds, double max_gap_s, double gain, int MW, int MH, double screen_w, double screen_h,
                                     double* state, double* coef, int* clear, eve_stream_t stream) {
    const char* why = nullptr;
    if (B <= 0 || T < 0 || !state || !clear) why = "bad arguments";
    else if (T > 0 && !coef) why = "a null coefficient buffer with T > 0";
    else if (T > 0 && B > (long long)0x7fffffff / 4 / T) why = "B * T * 4 must fit 31 bits";
    else if (MW < 1 || MW > 2048 || MH < 1 || MH > 2048) why = "the map's axes must lie in 1 .. 2048";
    else if (!gh_positive(screen_w) || !gh_positive(screen_h)) why = "the screen size must be finite numbers > 0";
    else if (T > 0 && !frame_time && !gh_positive(fps)) why = "without frame_time, fps must be a finite number > 0";
    else if (!(fps >= 0.0 && fps <= 1.79769313486231570815e308)) why = "fps must be 0 (not given) or a finite number > 0";
    else if (!(ln_decay <= 0.0 && ln_decay >= -1.79769313486231570815e308)) why = "ln_decay must be a finite number <= 0";
    else if (!gh_positive(max_gap_s) || !gh_positive(gain)) why = "max_gap_s and gain must be finite numbers > 0";
    if (why) {
        char msg[160];
        snprintf(msg, sizeof(msg), "gaze_history_plan: %s", why);
        return set_error_msg(msg);
    }
    GhPlan P;
    P.has_fps = fps > 0.0 ? 1 : 0;
    P.fps = P.has_fps ? fps : 1.0;
    P.ln_decay = ln_decay;
    P.max_gap = max_gap_s;
    P.gain = gain;
    P.sx = (double)MW / screen_w;
    P.sy = (double)MH / screen_h;
    P.seconds = weight_seconds ? 1 : 0;
    EVE_LAUNCH("gaze_history_plan_kernel", gaze_history_plan_kernel, dim3((unsigned)B), dim3(GH_WAVE), 0, (hipStream_t)stream, T, pog, frame_time,
               valid, valid_key, lengths, reset, P, state, coef, clear);
    EVE_CHECK_LAUNCH();
    return 0;
}

extern "C" int eve_gaze_history_update(long long B, int T, int MH, int MW, const double* coef, const int* clear, const float* heat, double alpha,
                                       double floor, float* map, float* frames, eve_stream_t stream) {
    const char* why = nullptr;
    if (B <= 0 || B > 65535 || T < 0 || !clear || !map) why = "bad arguments (B in 1 .. 65535)";
    else if (T > 0 && !coef) why = "a null coefficient buffer with T > 0";
    else if (MW < 1 || MW > 2048 || MH < 1 || MH > 2048) why = "the map's axes must lie in 1 .. 2048";
    else if (T > 0 && B > (long long)0x7fffffff / 4 / T) why = "B * T * 4 must fit 31 bits";
    else if (!(alpha < 0.0 && alpha >= -1.79769313486231570815e308)) why = "alpha = -0.5 / sigma^2 must be a finite number < 0";
    else if (!(floor >= 0.0 && floor <= 1.79769313486231570815e308)) why = "floor must be a finite number >= 0";
    if (why) {
        char msg[160];
        snprintf(msg, sizeof(msg), "gaze_history_update: %s", why);
        return set_error_msg(msg);
    }
    const int tiles_x = (MW + GH_TW - 1) / GH_TW, tiles_y = (MH + GH_TH - 1) / GH_TH;
    const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)B);
    const bool vec = MW % GH_PX == 0 && gh_aligned16(map) && (!frames || gh_aligned16(frames)) && (!heat || gh_aligned16(heat));
    if (vec)
        EVE_LAUNCH("gaze_history_update_kernel", gaze_history_update_kernel<true>, grid, dim3(GH_THREADS), 0, (hipStream_t)stream, T, MH, MW,
                   tiles_x, coef, clear, heat, alpha, floor, map, frames);
    else
        EVE_LAUNCH("gaze_history_update_kernel", gaze_history_update_kernel<false>, grid, dim3(GH_THREADS), 0, (hipStream_t)stream, T, MH, MW,
                   tiles_x, coef, clear, heat, alpha, floor, map, frames);
    EVE_CHECK_LAUNCH();
    return 0;
}
