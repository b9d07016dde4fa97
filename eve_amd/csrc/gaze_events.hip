// Gaze filtering and fixation / saccade events, on the device: the last stage of a live tracker.  Per stream the point of gaze is
// smoothed by a one-euro filter (Casiez et al. 2012), the angular velocity of the gaze vector between consecutive samples is
// formed, every frame is labelled fixation or saccade by a velocity threshold (I-VT), the running fixation is tracked and completed
// fixations are appended to the stream's store.  The contract -- operation order and the state row included -- is in
// include/eve_hip.h (eve_gaze_events) and in numpy in tests/gaze_events_ref.py.
//
// One wavefront (a 64-thread workgroup) per stream; the frames go by in passes of 64, each pass in phases, its intermediates in LDS:
//   0  parallel   lane t reads frame t's inputs, forms e = T3 o + t and the frame's time, and tests what does not depend on history
//   1  serial     lane 0 walks the pass: the time-order test, the gap rule, the one-euro update (no transcendental)
//   2  parallel   lane t forms its gaze vector, finds its predecessor sample -- the highest set bit below t in the wave's ballot of
//                 the sample flags, the carried vector for the pass's first sample -- and computes the angle (sqrt, atan2) and velocity
//   3  serial     lane 0: the I-VT state machine, the running fixation's sums, the store appends, the per-frame results into LDS
//   4  parallel   lane t writes frame t's seven outputs, and for eve_gaze_events_ex its sample flag, time and gaze vector
// The float64 atan2 is the one long dependency chain, and phase 2 keeps it off the serial path.  Float64 throughout, every operation
// rounded on its own: the bits do not depend on this structure.  Every branch around a barrier or a ballot is uniform over the wave.
#include "common.h"

#pragma clang fp contract(off)

namespace eve {
namespace {

constexpr int GE_WAVE = 64;
constexpr int GE_STATE = 32;             // doubles per state row (include/eve_hip.h has the layout)
constexpr int GE_ROW = 8;                // doubles per stored fixation
enum { GE_TICKS = 0, GE_HAS_PREV, GE_T_PREV, GE_XR_PREV, GE_YR_PREV, GE_XH, GE_YH, GE_DXH, GE_DYH, GE_V0, GE_V1, GE_V2, GE_FIX_OPEN, GE_FIX_ID,
       GE_NEXT_ID, GE_X0, GE_Y0, GE_FIX_N, GE_SDX, GE_SDY, GE_SD2, GE_T_START, GE_T_LAST };

struct GeParams {
    double fps, min_cutoff, beta, d_cutoff, saccade, min_fix, max_gap;
    int raw;
};

__device__ __forceinline__ bool ge_finite(const double x) { return fabs(x) <= 1.79769313486231570815e308; }      // false for a NaN

__device__ __forceinline__ double ge_alpha(const double fc, const double dt) {
#pragma clang fp contract(off)
    return 1.0 / (1.0 + (1.0 / (6.283185307179586 * fc)) / dt);
}

// Closes the open fixation of the state row st (lane 0 only): a row into the store where it lasted long enough.
__device__ __forceinline__ void ge_close(double* st, const double min_fix, double* __restrict__ rows, const int F, int& cnt, int& drop) {
#pragma clang fp contract(off)
    if (st[GE_FIX_OPEN] == 0.0) return;
    st[GE_FIX_OPEN] = 0.0;
    if (!(st[GE_T_LAST] - st[GE_T_START] >= min_fix)) return;
    if (cnt >= F) {
        ++drop;
        return;
    }
    const double n = st[GE_FIX_N], mx = st[GE_SDX] / n, my = st[GE_SDY] / n;
    const double var = st[GE_SD2] / n - (mx * mx + my * my);
    double* dst = rows + (size_t)cnt * GE_ROW;
    dst[0] = st[GE_FIX_ID];
    dst[1] = st[GE_T_START];
    dst[2] = st[GE_T_LAST];
    dst[3] = n;
    dst[4] = st[GE_X0] + mx;
    dst[5] = st[GE_Y0] + my;
    dst[6] = var > 0.0 ? sqrt(var) : 0.0;
    dst[7] = 0.0;
    ++cnt;
}

__global__ __launch_bounds__(GE_WAVE) void gaze_events_kernel(const int T, const float* __restrict__ pog, const float* __restrict__ origin,
                                                              const float* __restrict__ inv_cam, const float* __restrict__ ppm,
                                                              const double* __restrict__ frame_time, const uint8_t* __restrict__ valid,
                                                              const int* __restrict__ lengths, const int* __restrict__ reset,
                                                              const int* __restrict__ flush, const GeParams P, double* __restrict__ state,
                                                              const int F, double* __restrict__ store, int* __restrict__ count,
                                                              int* __restrict__ dropped, float* __restrict__ filtered,
                                                              float* __restrict__ velocity, uint8_t* __restrict__ event,
                                                              int* __restrict__ fixation_id, float* __restrict__ fixation_px,
                                                              float* __restrict__ fixation_ms, uint8_t* __restrict__ fixating,
                                                              uint8_t* __restrict__ sample, double* __restrict__ sample_time,
                                                              double* __restrict__ gaze_vector) {      // the last three: NULL, or _ex's
#pragma clang fp contract(off)
    __shared__ double st[GE_STATE];
    __shared__ double s_x[GE_WAVE], s_y[GE_WAVE], s_sx[GE_WAVE], s_sy[GE_WAVE], s_e[3][GE_WAVE], s_tt[GE_WAVE], s_dt[GE_WAVE];
    __shared__ double s_xh[GE_WAVE], s_yh[GE_WAVE], s_v[3][GE_WAVE], s_vel[GE_WAVE], s_fx[GE_WAVE], s_fy[GE_WAVE], s_ms[GE_WAVE];
    __shared__ int s_flag[GE_WAVE], s_id[GE_WAVE];                      // flag: 0 no sample, 1 a sample that restarts the chain, 2 a chained one
    __shared__ uint8_t s_event[GE_WAVE], s_fixating[GE_WAVE];
    const int lane = threadIdx.x;
    const long long b = blockIdx.x;
    double* row = state + (size_t)b * GE_STATE;
    double* rows = store + (size_t)b * F * GE_ROW;
    int cnt = 0, drop = 0;                                             // lane 0's
    if (lane < GE_STATE) st[lane] = row[lane];
    __syncthreads();
    if (lane == 0) {
        cnt = min(max(count[b], 0), F);
        drop = dropped[b];
        if (reset && reset[b] != 0) {
            ge_close(st, P.min_fix, rows, F, cnt, drop);
            const double keep = st[GE_NEXT_ID];
            for (int i = 0; i < GE_STATE; ++i) st[i] = 0.0;
            st[GE_NEXT_ID] = keep;
        }
    }
    __syncthreads();
    int len = T;
    if (lengths) len = min(max(lengths[b], 0), T);
    const double ticks0 = st[GE_TICKS];
    for (int base = 0; base < T; base += GE_WAVE) {                    // (T, base: the same in every lane)
        const int f = base + lane;
        const long long n = b * T + f;
        // ---- phase 0
        bool ok = false;
        if (f < len) {
            const double tt = frame_time ? frame_time[n] : (ticks0 + (double)f) / P.fps;
            const double x = (double)pog[n * 2], y = (double)pog[n * 2 + 1], sx = (double)ppm[n * 2], sy = (double)ppm[n * 2 + 1];
            double o[3], Tm[12];
            ok = (!valid || valid[n] != 0) && ge_finite(tt) && ge_finite(x) && ge_finite(y) && ge_finite(sx) && ge_finite(sy);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                o[i] = (double)origin[n * 3 + i];
                ok = ok && ge_finite(o[i]);
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const double v = (double)inv_cam[n * 16 + i];
                ok = ok && ge_finite(v);
                if (i < 12) Tm[i] = v;
            }
            double e[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) e[i] = ((Tm[i * 4] * o[0] + Tm[i * 4 + 1] * o[1]) + Tm[i * 4 + 2] * o[2]) + Tm[i * 4 + 3];
            ok = ok && e[2] != 0.0;
            s_x[lane] = x;
            s_y[lane] = y;
            s_sx[lane] = sx;
            s_sy[lane] = sy;
            s_e[0][lane] = e[0];
            s_e[1][lane] = e[1];
            s_e[2][lane] = e[2];
            s_tt[lane] = tt;
        }
        s_flag[lane] = ok ? 1 : 0;
        __syncthreads();
        // ---- phase 1
        if (lane == 0) {
            const int m = min(GE_WAVE, len - base);
            for (int t = 0; t < m; ++t) {
                if (s_flag[t] == 0) continue;
                const double tt = s_tt[t], x = s_x[t], y = s_y[t];
                const bool has_prev = st[GE_HAS_PREV] != 0.0;
                if (has_prev && !(tt > st[GE_T_PREV])) {
                    s_flag[t] = 0;
                    continue;
                }
                const double dt = tt - st[GE_T_PREV];
                const bool restart = !has_prev || dt > P.max_gap;
                double xh = x, yh = y, dxh = 0.0, dyh = 0.0;
                if (!restart) {
                    const double ad = ge_alpha(P.d_cutoff, dt);
                    dxh = ad * ((x - st[GE_XR_PREV]) / dt) + (1.0 - ad) * st[GE_DXH];
                    dyh = ad * ((y - st[GE_YR_PREV]) / dt) + (1.0 - ad) * st[GE_DYH];
                    const double ax = ge_alpha(P.min_cutoff + P.beta * fabs(dxh), dt), ay = ge_alpha(P.min_cutoff + P.beta * fabs(dyh), dt);
                    xh = ax * x + (1.0 - ax) * st[GE_XH];
                    yh = ay * y + (1.0 - ay) * st[GE_YH];
                }
                st[GE_HAS_PREV] = 1.0;
                st[GE_T_PREV] = tt;
                st[GE_XR_PREV] = x;
                st[GE_YR_PREV] = y;
                st[GE_XH] = xh;
                st[GE_YH] = yh;
                st[GE_DXH] = dxh;
                st[GE_DYH] = dyh;
                s_xh[t] = xh;
                s_yh[t] = yh;
                s_dt[t] = dt;
                s_flag[t] = restart ? 1 : 2;
            }
        }
        __syncthreads();
        // ---- phase 2
        const int flag = s_flag[lane];
        const unsigned long long samples = __ballot(flag != 0);
        double v[3] = {0.0, 0.0, 0.0};
        if (flag != 0) {
            const double px = P.raw ? s_x[lane] : s_xh[lane], py = P.raw ? s_y[lane] : s_yh[lane];
            v[0] = px / s_sx[lane] - s_e[0][lane];
            v[1] = py / s_sy[lane] - s_e[1][lane];
            v[2] = -s_e[2][lane];
            s_v[0][lane] = v[0];
            s_v[1][lane] = v[1];
            s_v[2][lane] = v[2];
        }
        __syncthreads();
        if (flag == 2) {
            const unsigned long long below = lane == 0 ? 0ull : samples & (~0ull >> (64 - lane));
            double p[3];
            if (below != 0ull) {
                const int q = 63 - __clzll((long long)below);
                p[0] = s_v[0][q];
                p[1] = s_v[1][q];
                p[2] = s_v[2][q];
            } else {
                p[0] = st[GE_V0];
                p[1] = st[GE_V1];
                p[2] = st[GE_V2];
            }
            const double c0 = p[1] * v[2] - p[2] * v[1], c1 = p[2] * v[0] - p[0] * v[2], c2 = p[0] * v[1] - p[1] * v[0];
            const double angle = atan2(sqrt((c0 * c0 + c1 * c1) + c2 * c2), (p[0] * v[0] + p[1] * v[1]) + p[2] * v[2]);
            s_vel[lane] = angle * 57.29577951308232 / s_dt[lane];
        }
        __syncthreads();
        // ---- phase 3
        if (lane == 0) {
            if (samples != 0ull) {                                     // the carried vector: the pass's last sample's
                const int q = 63 - __clzll((long long)samples);
                st[GE_V0] = s_v[0][q];
                st[GE_V1] = s_v[1][q];
                st[GE_V2] = s_v[2][q];
            }
            const int m = min(GE_WAVE, T - base);
            for (int t = 0; t < m; ++t) {
                const int fl = s_flag[t];
                int ev = 0, id = -1, fixg = 0;
                double fx = 0.0, fy = 0.0, ms = 0.0;
                if (fl == 1) {
                    ge_close(st, P.min_fix, rows, F, cnt, drop);
                } else if (fl == 2) {
                    if (s_vel[t] > P.saccade) {
                        ev = 2;
                        ge_close(st, P.min_fix, rows, F, cnt, drop);
                    } else {
                        ev = 1;
                        const double tt = s_tt[t], x = s_x[t], y = s_y[t];
                        if (st[GE_FIX_OPEN] == 0.0) {
                            st[GE_FIX_OPEN] = 1.0;
                            st[GE_FIX_ID] = st[GE_NEXT_ID];
                            st[GE_NEXT_ID] = st[GE_NEXT_ID] + 1.0;
                            st[GE_X0] = x;
                            st[GE_Y0] = y;
                            st[GE_FIX_N] = 0.0;
                            st[GE_SDX] = 0.0;
                            st[GE_SDY] = 0.0;
                            st[GE_SD2] = 0.0;
                            st[GE_T_START] = tt;
                        }
                        const double ddx = x - st[GE_X0], ddy = y - st[GE_Y0];
                        st[GE_FIX_N] = st[GE_FIX_N] + 1.0;
                        st[GE_SDX] = st[GE_SDX] + ddx;
                        st[GE_SDY] = st[GE_SDY] + ddy;
                        st[GE_SD2] = st[GE_SD2] + (ddx * ddx + ddy * ddy);
                        st[GE_T_LAST] = tt;
                        id = (int)st[GE_FIX_ID];
                        fx = st[GE_X0] + st[GE_SDX] / st[GE_FIX_N];
                        fy = st[GE_Y0] + st[GE_SDY] / st[GE_FIX_N];
                        ms = 1000.0 * (tt - st[GE_T_START]);
                        fixg = (tt - st[GE_T_START] >= P.min_fix) ? 1 : 0;
                    }
                }
                s_event[t] = (uint8_t)ev;
                s_id[t] = id;
                s_fx[t] = fx;
                s_fy[t] = fy;
                s_ms[t] = ms;
                s_fixating[t] = (uint8_t)fixg;
            }
        }
        __syncthreads();
        // ---- phase 4
        if (f < T) {
            if (flag != 0) {
                filtered[n * 2] = (float)s_xh[lane];
                filtered[n * 2 + 1] = (float)s_yh[lane];
            } else {                                                   // not a sample: the source as it came
                filtered[n * 2] = pog[n * 2];
                filtered[n * 2 + 1] = pog[n * 2 + 1];
            }
            velocity[n] = flag == 2 ? (float)s_vel[lane] : __builtin_nanf("");
            event[n] = s_event[lane];
            fixation_id[n] = s_id[lane];
            fixation_px[n * 2] = (float)s_fx[lane];
            fixation_px[n * 2 + 1] = (float)s_fy[lane];
            fixation_ms[n] = (float)s_ms[lane];
            fixating[n] = s_fixating[lane];
            if (sample) sample[n] = (uint8_t)flag;
            if (sample_time) sample_time[n] = flag != 0 ? s_tt[lane] : 0.0;
            if (gaze_vector) {
                gaze_vector[n * 3] = flag != 0 ? s_v[0][lane] : 0.0;
                gaze_vector[n * 3 + 1] = flag != 0 ? s_v[1][lane] : 0.0;
                gaze_vector[n * 3 + 2] = flag != 0 ? s_v[2][lane] : 0.0;
            }
        }
        __syncthreads();
    }
    if (lane == 0) {
        st[GE_TICKS] = ticks0 + (double)len;
        if (flush && flush[b] != 0) ge_close(st, P.min_fix, rows, F, cnt, drop);
        count[b] = cnt;
        dropped[b] = drop;
    }
    __syncthreads();
    if (lane < GE_STATE) row[lane] = st[lane];
}

__host__ bool ge_positive(const double x) { return x > 0.0 && x <= 1.79769313486231570815e308; }

}  // namespace
}  // namespace eve

using namespace eve;

// Both entries: the checks and the one launch.  sample, sample_time and gaze_vector: each NULL or eve_gaze_events_ex's output.
static int ge_launch(long long B, int T, const float* pog, const float* origin, const float* inv_cam, const float* ppm, const double* frame_time,
                     const uint8_t* valid, const int* lengths, const int* reset, const int* flush, double fps, double min_cutoff_hz, double beta,
                     double d_cutoff_hz, int velocity_from_raw, double saccade_deg_s, double min_fixation_s, double max_gap_s, double* state,
                     int F, double* store, int* count, int* dropped, float* filtered, float* velocity, uint8_t* event, int* fixation_id,
                     float* fixation_px, float* fixation_ms, uint8_t* fixating, uint8_t* sample, double* sample_time, double* gaze_vector,
                     eve_stream_t stream) {
    const char* why = nullptr;
    if (B <= 0 || T < 0 || F <= 0 || !state || !store || !count || !dropped) why = "bad arguments";
    else if (T > 0 && (!pog || !origin || !inv_cam || !ppm || !filtered || !velocity || !event || !fixation_id || !fixation_px || !fixation_ms ||
                       !fixating))
        why = "a null frame input or output with T > 0";
    else if (T > 0 && B > (long long)0x7fffffff / 16 / T) why = "B * T * 16 must fit 31 bits";
    else if (B > (long long)0x7fffffff / 8 / F) why = "B * F * 8 must fit 31 bits";
    else if (T > 0 && !frame_time && !ge_positive(fps)) why = "without frame_time, fps must be a finite number > 0";
    else if (!ge_positive(min_cutoff_hz) || !ge_positive(d_cutoff_hz) || !ge_positive(saccade_deg_s) || !ge_positive(min_fixation_s) ||
             !ge_positive(max_gap_s))
        why = "the cutoffs, saccade_deg_s, min_fixation_s and max_gap_s must be finite numbers > 0";
    else if (!(beta >= 0.0 && beta <= 1.79769313486231570815e308)) why = "beta must be a finite number >= 0";
    if (why) {
        char msg[160];
        snprintf(msg, sizeof(msg), "gaze_events: %s", why);
        return set_error_msg(msg);
    }
    GeParams P;
    P.fps = frame_time ? 1.0 : fps;
    P.min_cutoff = min_cutoff_hz;
    P.beta = beta;
    P.d_cutoff = d_cutoff_hz;
    P.saccade = saccade_deg_s;
    P.min_fix = min_fixation_s;
    P.max_gap = max_gap_s;
    P.raw = velocity_from_raw ? 1 : 0;
    EVE_LAUNCH("gaze_events_kernel", gaze_events_kernel, dim3((unsigned)B), dim3(GE_WAVE), 0, (hipStream_t)stream, T, pog, origin, inv_cam, ppm,
               frame_time, valid, lengths, reset, flush, P, state, F, store, count, dropped, filtered, velocity, event, fixation_id, fixation_px,
               fixation_ms, fixating, sample, sample_time, gaze_vector);
    EVE_CHECK_LAUNCH();
    return 0;
}

extern "C" int eve_gaze_events(long long B, int T, const float* pog, const float* origin, const float* inv_cam, const float* ppm,
                               const double* frame_time, const uint8_t* valid, const int* lengths, const int* reset, const int* flush, double fps,
                               double min_cutoff_hz, double beta, double d_cutoff_hz, int velocity_from_raw, double saccade_deg_s,
                               double min_fixation_s, double max_gap_s, double* state, int F, double* store, int* count, int* dropped,
                               float* filtered, float* velocity, uint8_t* event, int* fixation_id, float* fixation_px, float* fixation_ms,
                               uint8_t* fixating, eve_stream_t stream) {
    return ge_launch(B, T, pog, origin, inv_cam, ppm, frame_time, valid, lengths, reset, flush, fps, min_cutoff_hz, beta, d_cutoff_hz,
                     velocity_from_raw, saccade_deg_s, min_fixation_s, max_gap_s, state, F, store, count, dropped, filtered, velocity, event,
                     fixation_id, fixation_px, fixation_ms, fixating, nullptr, nullptr, nullptr, stream);
}

extern "C" int eve_gaze_events_ex(long long B, int T, const float* pog, const float* origin, const float* inv_cam, const float* ppm,
                                  const double* frame_time, const uint8_t* valid, const int* lengths, const int* reset, const int* flush,
                                  double fps, double min_cutoff_hz, double beta, double d_cutoff_hz, int velocity_from_raw,
                                  double saccade_deg_s, double min_fixation_s, double max_gap_s, double* state, int F, double* store,
                                  int* count, int* dropped, float* filtered, float* velocity, uint8_t* event, int* fixation_id,
                                  float* fixation_px, float* fixation_ms, uint8_t* fixating, uint8_t* sample, double* sample_time,
                                  double* gaze_vector, eve_stream_t stream) {
    return ge_launch(B, T, pog, origin, inv_cam, ppm, frame_time, valid, lengths, reset, flush, fps, min_cutoff_hz, beta, d_cutoff_hz,
                     velocity_from_raw, saccade_deg_s, min_fixation_s, max_gap_s, state, F, store, count, dropped, filtered, velocity, event,
                     fixation_id, fixation_px, fixation_ms, fixating, sample, sample_time, gaze_vector, stream);
}
