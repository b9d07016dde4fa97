// The eye gate: decides per frame and eye whether the eye is usable, on the device, between the pose derivation and the mask plan
// of an EVEStream step, and detects blinks with state carried from call to call.  The contract -- operation order, the state row and
// the store included -- is in include/eve_hip.h (eve_eye_gate) and in numpy in tests/eye_gate_ref.py.
//
// One wavefront (a 64-thread workgroup) per stream; the frames go by in passes of 64, each pass in phases, its intermediates in LDS:
//   0  parallel   lane t reads frame t's pose flag, rms, inlier count and head angles, forms both eyes' stateless reason bits, and
//                 both eyes' eyelid aspect ratio (six points, three distances, one division)
//   1  parallel   the coverage test, one (frame, eye) at a time over the whole wave: lane i + 8j pushes lattice point (ox_i, oy_j)
//                 through the warp; a ballot and a popcount give the inside count, which depends on no summation order
//   2  serial     lane e (0, 1) walks eye e's delivered frames in order: baseline, openness, the closed / open machine, hold-off; a
//                 blink that ends is noted at its frame
//   3  serial     lane 0 appends the pass's ended blinks to the store in (frame, eye) order
//   4  parallel   lane t writes frame t's outputs for both eyes
// Float64 throughout, every operation rounded on its own: the bits do not depend on this structure.  Every branch around a barrier
// or a ballot is uniform over the wave (T, base, the stream's frame count and the null tests are the same in every lane).
#include "common.h"

#pragma clang fp contract(off)

namespace eve {
namespace {

constexpr int EG_WAVE = 64;
constexpr int EG_STATE = 8;              // doubles per (stream, eye) state row (include/eve_hip.h has the layout)
constexpr int EG_ROW = 4;                // doubles per stored blink
enum { EG_HAS_BASE = 0, EG_BASE, EG_CLOSED, EG_RUN, EG_MIN_OPEN, EG_START, EG_HOLD, EG_TICK };
enum { EG_R_POSE = 1, EG_R_REPROJ = 2, EG_R_INLIERS = 4, EG_R_COVERAGE = 8, EG_R_HEAD = 16, EG_R_CLOSED = 32, EG_R_HOLD = 64 };

struct EgParams {
    double max_reproj, pitch_lo, pitch_hi, yaw_lo[2], yaw_hi[2], close_ratio, open_ratio, rate, rise;
    int min_inliers, min_inside, hold_frames, max_closed;
};

__device__ __forceinline__ bool eg_finite(const double x) { return fabs(x) <= 1.79769313486231570815e308; }      // false for a NaN

__device__ __forceinline__ double eg_dist(const double ax, const double ay, const double bx, const double by) {
#pragma clang fp contract(off)
    const double dx = ax - bx, dy = ay - by;
    return sqrt(dx * dx + dy * dy);
}

__global__ __launch_bounds__(EG_WAVE) void eye_gate_kernel(const long long B, const int T, const uint8_t* __restrict__ pose_valid,
                                                           const float* __restrict__ rms, const uint8_t* __restrict__ inliers,
                                                           const float* __restrict__ warp, const float* __restrict__ h,
                                                           const float* __restrict__ contours, const int C, const int* __restrict__ lengths,
                                                           const int* __restrict__ reset, const int IW, const int IH, const int OW, const int OH,
                                                           const EgParams P, double* __restrict__ state, const int F,
                                                           double* __restrict__ store, int* __restrict__ count, int* __restrict__ dropped,
                                                           uint8_t* __restrict__ usable, uint8_t* __restrict__ reason,
                                                           float* __restrict__ openness, uint8_t* __restrict__ blink) {
#pragma clang fp contract(off)
    __shared__ double st[2][EG_STATE];
    __shared__ double s_ear[2][EG_WAVE], s_open[2][EG_WAVE], s_start[2][EG_WAVE], s_min[2][EG_WAVE];
    __shared__ int s_reason[2][EG_WAVE], s_known[2][EG_WAVE], s_blink[2][EG_WAVE], s_ended[2][EG_WAVE];
    const int lane = threadIdx.x;
    const long long b = blockIdx.x;
    double* row = state + (size_t)b * 2 * EG_STATE;
    double* rows = store + (size_t)b * F * EG_ROW;
    int cnt = 0, drop = 0;                                             // lane 0's
    if (lane < 2 * EG_STATE) (&st[0][0])[lane] = (reset && reset[b] != 0) ? 0.0 : row[lane];
    if (lane == 0) {
        cnt = min(max(count[b], 0), F);
        drop = dropped[b];
    }
    __syncthreads();
    int len = T;
    if (lengths) len = min(max(lengths[b], 0), T);
    const int ox = ((2 * (lane & 7) + 1) * OW) >> 4, oy = ((2 * (lane >> 3) + 1) * OH) >> 4;      // this lane's lattice point
    for (int base = 0; base < T; base += EG_WAVE) {                    // (T, base, len: the same in every lane)
        const int f = base + lane;
        const long long n = b * T + f;
        const int m = min(EG_WAVE, len - base);                       // the pass's delivered frames (<= 0: none)
        // ---- phase 0
        if (f < len) {
            int common = 0;
            if (rms && !((double)rms[n] <= P.max_reproj)) common |= EG_R_REPROJ;                  // (a NaN fails)
            if (inliers && !((int)inliers[n] >= P.min_inliers)) common |= EG_R_INLIERS;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                int r = common;
                if (pose_valid && pose_valid[n * 2 + e] == 0) r |= EG_R_POSE;
                if (h) {
                    const long long q = ((long long)e * B * T + n) * 2;
                    const double pitch = (double)h[q], yaw = (double)h[q + 1];
                    if (!(pitch >= P.pitch_lo && pitch <= P.pitch_hi && yaw >= P.yaw_lo[e] && yaw <= P.yaw_hi[e])) r |= EG_R_HEAD;
                }
                s_reason[e][lane] = r;
                double ear = 0.0;
                bool known = false;
                if (contours) {
                    const float* p = contours + ((n * 2 + e) * 6) * C;
                    double x[6], y[6];
                    known = true;
#pragma unroll
                    for (int i = 0; i < 6; ++i) {
                        x[i] = (double)p[i * C];
                        y[i] = (double)p[i * C + 1];
                        known = known && eg_finite(x[i]) && eg_finite(y[i]);
                        if (C == 3) known = known && (double)p[i * C + 2] > 0.0;
                    }
                    const double d14 = eg_dist(x[0], y[0], x[3], y[3]);
                    known = known && d14 != 0.0;
                    if (known) ear = (eg_dist(x[1], y[1], x[5], y[5]) + eg_dist(x[2], y[2], x[4], y[4])) / (2.0 * d14);
                }
                s_ear[e][lane] = ear;
                s_known[e][lane] = known ? 1 : 0;
            }
        }
        __syncthreads();
        // ---- phase 1
        if (warp) {
            for (int t = 0; t < m; ++t) {
                for (int e = 0; e < 2; ++e) {
                    const float* w = warp + ((long long)e * B * T + (b * T + base + t)) * 9;
                    double mm[9];
#pragma unroll
                    for (int i = 0; i < 9; ++i) mm[i] = (double)w[i];
                    const double dx = (double)ox, dy = (double)oy;
                    const double X = (mm[0] * dx + mm[1] * dy) + mm[2];
                    const double Y = (mm[3] * dx + mm[4] * dy) + mm[5];
                    const double Wd = (mm[6] * dx + mm[7] * dy) + mm[8];
                    const double u = X / Wd, v = Y / Wd;
                    const bool inside = Wd > 0.0 && u > -1.0 && u < (double)IW && v > -1.0 && v < (double)IH;
                    const unsigned long long in = __ballot(inside);
                    if (lane == 0 && __popcll(in) < P.min_inside) s_reason[e][t] |= EG_R_COVERAGE;
                }
            }
        }
        __syncthreads();
        // ---- phase 2
        if (lane < 2) {
            double* s = st[lane];
            for (int t = 0; t < m; ++t) {
                int bit = 0, ended = 0, closed_now = 0;
                double open = __builtin_nan("");
                if (contours) {
                    const bool known = s_known[lane][t] != 0;
                    const double ear = s_ear[lane][t];
                    const double tick = s[EG_TICK] + (double)(base + t);
                    if (known && s[EG_HAS_BASE] == 0.0) {
                        s[EG_HAS_BASE] = 1.0;
                        s[EG_BASE] = ear;
                    }
                    if (known) open = ear / s[EG_BASE];
                    if (s[EG_CLOSED] != 0.0) {
                        s[EG_RUN] = s[EG_RUN] + 1.0;
                        if (known && open < s[EG_MIN_OPEN]) s[EG_MIN_OPEN] = open;
                        if (known && open > P.open_ratio) {              // the blink ends: noted here, stored by lane 0 in phase 3
                            ended = 1;
                            s_start[lane][t] = s[EG_START];
                            s_min[lane][t] = s[EG_MIN_OPEN];
                            s[EG_CLOSED] = 0.0;
                            s[EG_RUN] = 0.0;
                            s[EG_HOLD] = (double)P.hold_frames;
                        } else if (s[EG_RUN] > (double)P.max_closed) {   // a wrong baseline: start over from this frame, no blink, no hold-off
                            s[EG_HAS_BASE] = known ? 1.0 : 0.0;
                            s[EG_BASE] = known ? ear : 0.0;
                            s[EG_CLOSED] = 0.0;
                            s[EG_RUN] = 0.0;
                            if (known) open = ear / s[EG_BASE];
                        }
                    } else if (known && open < P.close_ratio) {
                        s[EG_CLOSED] = 1.0;
                        s[EG_RUN] = 1.0;
                        s[EG_MIN_OPEN] = open;
                        s[EG_START] = tick;
                    } else if (known && open >= P.open_ratio) {
                        const double r = ear > s[EG_BASE] ? P.rise : P.rate;
                        s[EG_BASE] = s[EG_BASE] + r * (ear - s[EG_BASE]);
                    }
                    if (s[EG_CLOSED] != 0.0) {
                        bit = EG_R_CLOSED;
                        closed_now = 1;
                    } else if (s[EG_HOLD] > 0.0) {
                        bit = EG_R_HOLD;
                        s[EG_HOLD] = s[EG_HOLD] - 1.0;
                    }
                }
                s_reason[lane][t] |= bit;
                s_open[lane][t] = open;
                s_blink[lane][t] = closed_now;
                s_ended[lane][t] = ended;
            }
        }
        __syncthreads();
        // ---- phase 3
        if (lane == 0 && contours) {
            for (int t = 0; t < m; ++t) {
                for (int e = 0; e < 2; ++e) {
                    if (s_ended[e][t] == 0) continue;
                    if (cnt >= F) {
                        ++drop;
                        continue;
                    }
                    double* dst = rows + (size_t)cnt * EG_ROW;
                    dst[0] = (double)e;
                    dst[1] = s_start[e][t];
                    dst[2] = (st[e][EG_TICK] + (double)(base + t)) - 1.0;
                    dst[3] = s_min[e][t];
                    ++cnt;
                }
            }
        }
        // ---- phase 4
        if (f < T) {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const bool live = f < len;
                const int r = live ? s_reason[e][lane] : 0;
                usable[n * 2 + e] = (uint8_t)((live && r == 0) ? 1 : 0);
                reason[n * 2 + e] = (uint8_t)r;
                openness[n * 2 + e] = live ? (float)s_open[e][lane] : __builtin_nanf("");
                blink[n * 2 + e] = (uint8_t)(live ? s_blink[e][lane] : 0);
            }
        }
        __syncthreads();
    }
    if (lane < 2) st[lane][EG_TICK] = st[lane][EG_TICK] + (double)len;
    if (lane == 0) {
        count[b] = cnt;
        dropped[b] = drop;
    }
    __syncthreads();
    if (lane < 2 * EG_STATE) row[lane] = (&st[0][0])[lane];
}

}  // namespace
}  // namespace eve

using namespace eve;

extern "C" int eve_eye_gate(long long B, int T, const uint8_t* pose_valid, const float* reproj_rms, const uint8_t* inliers, const float* warp,
                            const float* h, const float* contours, int C, const int* lengths, const int* reset, int IW, int IH, int OW, int OH,
                            const eve_eye_gate_params* params, double* state, int capacity, double* blinks, int* count, int* dropped,
                            uint8_t* usable, uint8_t* reason, float* openness, uint8_t* blink, eve_stream_t stream) {
    const char* why = nullptr;
    const auto nan = [](const double x) { return x != x; };
    if (B < 1 || T < 1 || capacity < 1) why = "B, T and the blink capacity must be >= 1";
    else if (!params || !state || !blinks || !count || !dropped || !usable || !reason || !openness || !blink)
        why = "a null parameter block, state, store, counter or output";
    else if (contours && C != 2 && C != 3) why = "contours hold 2 or 3 values per point";
    else if (warp && (IW < 1 || IH < 1 || OW < 1 || OH < 1 || IW > 16384 || IH > 16384 || OW > 16384 || OH > 16384))
        why = "warp needs the frame size IW, IH and the patch size OW, OH in 1 .. 16384";
    else if (B > (long long)0x7fffffff / 36 / T) why = "B * T * 36 must fit 31 bits";
    else if (B > (long long)0x7fffffff / 4 / capacity) why = "B * capacity * 4 must fit 31 bits";
    else if (nan(params->max_reproj_px) || nan(params->pitch_lo) || nan(params->pitch_hi) || nan(params->yaw_lo[0]) || nan(params->yaw_hi[0]) ||
             nan(params->yaw_lo[1]) || nan(params->yaw_hi[1]) || nan(params->close_ratio) || nan(params->open_ratio) ||
             nan(params->baseline_rate) || nan(params->baseline_rise))
        why = "a NaN parameter";
    else if (warp && (params->min_inside < 1 || params->min_inside > 64)) why = "min_inside must lie in 1 .. 64";
    else if (contours && !(params->open_ratio > params->close_ratio)) why = "open_ratio must be above close_ratio";
    else if (contours && (params->hold_frames < 0 || params->max_closed_frames < 1)) why = "hold_frames must be >= 0 and max_closed_frames >= 1";
    if (why) {
        char msg[160];
        snprintf(msg, sizeof(msg), "eye_gate: %s", why);
        return set_error_msg(msg);
    }
    EgParams P;
    P.max_reproj = params->max_reproj_px;
    P.pitch_lo = params->pitch_lo;
    P.pitch_hi = params->pitch_hi;
    for (int e = 0; e < 2; ++e) {
        P.yaw_lo[e] = params->yaw_lo[e];
        P.yaw_hi[e] = params->yaw_hi[e];
    }
    P.close_ratio = params->close_ratio;
    P.open_ratio = params->open_ratio;
    P.rate = params->baseline_rate;
    P.rise = params->baseline_rise;
    P.min_inliers = params->min_inliers;
    P.min_inside = params->min_inside;
    P.hold_frames = params->hold_frames;
    P.max_closed = params->max_closed_frames;
    EVE_LAUNCH("eye_gate_kernel", eye_gate_kernel, dim3((unsigned)B), dim3(EG_WAVE), 0, (hipStream_t)stream, B, T, pose_valid, reproj_rms, inliers,
               warp, h, contours, C, lengths, reset, IW, IH, OW, OH, P, state, capacity, blinks, count, dropped, usable, reason, openness, blink);
    EVE_CHECK_LAUNCH();
    return 0;
}
