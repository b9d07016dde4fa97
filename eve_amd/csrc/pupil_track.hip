// Pupillometry on the device: EyeNet's two pupil sizes per frame become one validated, binocularly fused, low-passed, light- and
// baseline-corrected trace per stream, with a table of tallies and a store of dilation / constriction episodes.  The contract --
// operation order, the state row and the table included -- is in include/eve_hip.h (eve_pupil_track) and in numpy in
// tests/pupil_ref.py.
//
// One wavefront (a 64-thread workgroup) per stream; the state row, the table and the light row live in LDS for the launch.  The
// frames go by in passes of 64, each pass in phases:
//   0  parallel   lane t reads frame t's two sizes, time, luminance and flags
//   1  serial     lane 0 walks the pass: acceptance, fusion, the filters, the baseline, the episodes, the table
//   2  parallel   lane t writes frame t's nine outputs
// Float64 throughout, + - * / , fabs and comparisons only, every operation rounded on its own: the bits do not depend on this
// structure.  Every branch around a barrier is uniform over the wave.  A value at a withheld eye is never used in arithmetic.
#include "common.h"

#pragma clang fp contract(off)

namespace eve {
namespace {

constexpr int PT_WAVE = 64;
constexpr int PT_STATE = 32;             // doubles per state row (include/eve_hip.h has the layout)
constexpr int PT_TABLE = 24;             // doubles per table row
constexpr int PT_LIGHT = 4;
constexpr int PT_ROW = 8;                // doubles per stored episode
enum { PT_TICKS = 0, PT_HAS_PREV, PT_T_PREV, PT_DF, PT_LAST_IDX, PT_HAS_L, PT_T_L, PT_V_L, PT_HAS_R, PT_T_R, PT_V_R, PT_HAS_OFF, PT_OFF,
       PT_HAS_LUM, PT_T_LUM, PT_LF, PT_HAS_BASE, PT_BASE, PT_B_N, PT_B_D0, PT_B_SUM, PT_PREV_MARK, PT_EP_OPEN, PT_EP_PHASE, PT_EP_T_START,
       PT_EP_T_END, PT_EP_D_START, PT_EP_D_END, PT_EP_PEAK, PT_EP_SAMPLES, PT_EP_LF, PT_EP_COUNT };
enum { PT_COVERED = 0, PT_LOST, PT_BOTH, PT_LEFT, PT_RIGHT, PT_REJ = 5 /* [eye][not finite, range, speed] */, PT_D0 = 11, PT_S1, PT_S2, PT_MIN,
       PT_MAX, PT_N, PT_X0, PT_Y0, PT_SX, PT_SY, PT_SXX, PT_SXY, PT_SYY };
enum { PT_F_EYE_L = 1, PT_F_EYE_R = 2, PT_F_MARK = 4 };

struct PupilParams {
    double fps, min_mm, max_mm, max_speed, max_gap, offset_rate, cutoff_hz, light_tau, baseline_tau, dilate, constrict, min_amplitude;
};

__device__ __forceinline__ bool pt_finite(const double x) { return fabs(x) <= 1.79769313486231570815e308; }      // false for a NaN

// Closes the open episode of the state row st (lane 0 only): a row into the store where its amplitude counts, or a drop where the
// store is full.  cd (in LDS, so that nothing lives in scratch): the stream's count and dropped.
__device__ __forceinline__ void pt_close(double* st, double* __restrict__ rows, const int V, int* cd, const double min_amplitude) {
#pragma clang fp contract(off)
    if (st[PT_EP_OPEN] == 0.0) return;
    st[PT_EP_OPEN] = 0.0;
    if (!(fabs(st[PT_EP_D_END] - st[PT_EP_D_START]) >= min_amplitude)) return;
    st[PT_EP_COUNT] = st[PT_EP_COUNT] + 1.0;
    const int cnt = cd[0];
    if (cnt >= V) {
        cd[1] = cd[1] + 1;
        return;
    }
    double* dst = rows + (size_t)cnt * PT_ROW;
    dst[0] = st[PT_EP_PHASE];
    dst[1] = st[PT_EP_T_START];
    dst[2] = st[PT_EP_T_END];
    dst[3] = st[PT_EP_D_START];
    dst[4] = st[PT_EP_D_END];
    dst[5] = st[PT_EP_PEAK];
    dst[6] = st[PT_EP_SAMPLES];
    dst[7] = st[PT_EP_LF];
    cd[0] = cnt + 1;
}

__global__ __launch_bounds__(PT_WAVE) void pupil_track_kernel(const int T, const float* __restrict__ size, const long long side,
                                                              const uint8_t* __restrict__ eye_valid, const double* __restrict__ frame_time,
                                                              const int* __restrict__ lengths, const int* __restrict__ reset,
                                                              const int* __restrict__ flush, const float* __restrict__ luminance,
                                                              const uint8_t* __restrict__ baseline_mark, const PupilParams P,
                                                              double* __restrict__ state, double* __restrict__ table, double* __restrict__ light,
                                                              const int V, double* __restrict__ store, int* __restrict__ count,
                                                              int* __restrict__ dropped, float* __restrict__ out_mm, float* __restrict__ out_raw,
                                                              float* __restrict__ out_velocity, float* __restrict__ out_change_mm,
                                                              float* __restrict__ out_change_pct, uint8_t* __restrict__ out_valid,
                                                              uint8_t* __restrict__ out_used, uint8_t* __restrict__ out_reason,
                                                              uint8_t* __restrict__ out_event) {
#pragma clang fp contract(off)
    __shared__ double st[PT_STATE];
    __shared__ double tab[PT_TABLE];
    __shared__ double lt[PT_LIGHT];
    __shared__ double s_size[2][PT_WAVE], s_tt[PT_WAVE], s_lum[PT_WAVE];
    __shared__ double s_out[5][PT_WAVE];                               // mm, raw_mm, velocity, change_mm, change_pct
    __shared__ int s_flag[PT_WAVE];                                    // in: PT_F_*; out: valid | used << 1 | reason << 3 | event << 11
    __shared__ int s_cd[2];                                            // the stream's count and dropped (lane 0's)
    const int lane = threadIdx.x;
    const long long b = blockIdx.x;
    double* row = state + (size_t)b * PT_STATE;
    double* trow = table + (size_t)b * PT_TABLE;
    double* rows = store + (size_t)b * V * PT_ROW;
    if (lane < PT_STATE) st[lane] = row[lane];
    if (lane < PT_TABLE) tab[lane] = trow[lane];
    if (lane < PT_LIGHT) lt[lane] = light[(size_t)b * PT_LIGHT + lane];
    __syncthreads();
    if (lane == 0) {
        s_cd[0] = min(max(count[b], 0), V);
        s_cd[1] = dropped[b];
        if (reset && reset[b] != 0) {
            pt_close(st, rows, V, s_cd, P.min_amplitude);
            const double keep = st[PT_EP_COUNT];
            for (int i = 0; i < PT_STATE; ++i) st[i] = 0.0;
            st[PT_EP_COUNT] = keep;
        }
    }
    __syncthreads();
    int len = T;
    if (lengths) len = min(max(lengths[b], 0), T);
    const double ticks0 = st[PT_TICKS];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int base = 0; base < T; base += PT_WAVE) {                    // (T, base, len: the same in every lane)
        const int f = base + lane;
        const long long n = b * T + f;
        // ---- phase 0
        if (f < len) {
            int flag = 0;
            if (!eye_valid || eye_valid[n * 2] != 0) flag |= PT_F_EYE_L;
            if (!eye_valid || eye_valid[n * 2 + 1] != 0) flag |= PT_F_EYE_R;
            if (baseline_mark && baseline_mark[n] != 0) flag |= PT_F_MARK;
            s_flag[lane] = flag;
            s_size[0][lane] = (double)size[n];
            s_size[1][lane] = (double)size[side + n];
            s_tt[lane] = frame_time ? frame_time[n] : (ticks0 + (double)f) / P.fps;
            s_lum[lane] = luminance ? (double)luminance[n] : nan;
        }
        __syncthreads();
        // ---- phase 1
        if (lane == 0) {
            const int mt = min(PT_WAVE, T - base);
            const int m = min(PT_WAVE, len - base);                    // the pass's delivered frames (<= 0: none)
            for (int t = 0; t < mt; ++t) {
                double o_mm = nan, o_raw = nan, o_vel = nan, o_cmm = nan, o_cpct = nan;
                int code = 0;
                const bool timed = t < m && pt_finite(s_tt[t]) && (st[PT_HAS_PREV] == 0.0 || s_tt[t] > st[PT_T_PREV]);
                if (timed) {
                    const double tt = s_tt[t];
                    const int flag = s_flag[t];
                    // the light covariate's own low pass: every frame with a finite luminance, sample or not
                    if (luminance) {
                        const double lum = s_lum[t];
                        if (pt_finite(lum) && (st[PT_HAS_LUM] == 0.0 || tt > st[PT_T_LUM])) {
                            const double dtl = tt - st[PT_T_LUM];
                            if (st[PT_HAS_LUM] == 0.0 || dtl > P.max_gap) {
                                st[PT_LF] = lum;
                            } else {
                                const double al = 1.0 / (1.0 + P.light_tau / dtl);
                                st[PT_LF] = al * lum + (1.0 - al) * st[PT_LF];
                            }
                            st[PT_HAS_LUM] = 1.0;
                            st[PT_T_LUM] = tt;
                        }
                    }
                    // per-eye acceptance
                    bool acc[2];
                    double val[2];
                    int reason = 0;
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const int se = PT_HAS_L + 3 * e;               // (has, t, value) of the eye's last accepted size
                        int why = 0;
                        double v = 0.0;
                        if ((flag & (PT_F_EYE_L << e)) == 0) {
                            why = 1;
                        } else {
                            v = s_size[e][t];
                            if (!pt_finite(v)) {
                                why = 2;
                            } else if (!(P.min_mm <= v && v <= P.max_mm)) {
                                why = 4;
                            } else if (st[se] != 0.0 && tt - st[se + 1] <= P.max_gap) {
                                if (!(fabs(v - st[se + 2]) / (tt - st[se + 1]) <= P.max_speed)) why = 8;
                            }
                        }
                        acc[e] = why == 0;
                        val[e] = acc[e] ? v : 0.0;                     // (selected, never multiplied)
                        if (why == 2) tab[PT_REJ + 3 * e] = tab[PT_REJ + 3 * e] + 1.0;
                        if (why == 4) tab[PT_REJ + 3 * e + 1] = tab[PT_REJ + 3 * e + 1] + 1.0;
                        if (why == 8) tab[PT_REJ + 3 * e + 2] = tab[PT_REJ + 3 * e + 2] + 1.0;
                        reason |= why << (4 * e);
                    }
                    code = reason << 3;
                    if (acc[0] || acc[1]) {
                        // binocular fusion with the running offset
                        const double l = val[0], r = val[1];
                        double d;
                        if (acc[0] && acc[1]) {
                            const double diff = l - r;
                            st[PT_OFF] = st[PT_HAS_OFF] != 0.0 ? st[PT_OFF] + P.offset_rate * (diff - st[PT_OFF]) : diff;
                            st[PT_HAS_OFF] = 1.0;
                            d = 0.5 * (l + r);
                            tab[PT_BOTH] = tab[PT_BOTH] + 1.0;
                        } else if (acc[0]) {
                            d = st[PT_HAS_OFF] != 0.0 ? l - 0.5 * st[PT_OFF] : l;
                            tab[PT_LEFT] = tab[PT_LEFT] + 1.0;
                        } else {
                            d = st[PT_HAS_OFF] != 0.0 ? r + 0.5 * st[PT_OFF] : r;
                            tab[PT_RIGHT] = tab[PT_RIGHT] + 1.0;
                        }
                        // the filter
                        const double dt = tt - st[PT_T_PREV];
                        const bool restart = st[PT_HAS_PREV] == 0.0 || dt > P.max_gap;
                        const double idx = ticks0 + (double)(base + t);
                        double df, vel = nan;
                        if (restart) {
                            df = d;
                            pt_close(st, rows, V, s_cd, P.min_amplitude);
                        } else {
                            const double a = 1.0 / (1.0 + (1.0 / (6.283185307179586 * P.cutoff_hz)) / dt);
                            df = a * d + (1.0 - a) * st[PT_DF];
                            vel = (df - st[PT_DF]) / dt;
                            tab[PT_COVERED] = tab[PT_COVERED] + dt;
                            if (idx - st[PT_LAST_IDX] != 1.0) tab[PT_LOST] = tab[PT_LOST] + dt;
                        }
                        // the light covariate
                        double dc = df;
                        const bool lit = luminance && st[PT_HAS_LUM] != 0.0;
                        if (lit) {
                            if (tab[PT_N] == 0.0) {
                                tab[PT_X0] = st[PT_LF];
                                tab[PT_Y0] = df;
                            }
                            const double dx = st[PT_LF] - tab[PT_X0], dy = df - tab[PT_Y0];
                            tab[PT_N] = tab[PT_N] + 1.0;
                            tab[PT_SX] = tab[PT_SX] + dx;
                            tab[PT_SY] = tab[PT_SY] + dy;
                            tab[PT_SXX] = tab[PT_SXX] + dx * dx;
                            tab[PT_SXY] = tab[PT_SXY] + dx * dy;
                            tab[PT_SYY] = tab[PT_SYY] + dy * dy;
                            if (lt[0] != 0.0) dc = df - lt[1] * (st[PT_LF] - lt[2]);
                        }
                        // the baseline
                        if (baseline_mark) {
                            if ((flag & PT_F_MARK) != 0) {
                                if (st[PT_PREV_MARK] == 0.0) {
                                    st[PT_B_D0] = dc;
                                    st[PT_B_N] = 0.0;
                                    st[PT_B_SUM] = 0.0;
                                }
                                st[PT_B_N] = st[PT_B_N] + 1.0;
                                st[PT_B_SUM] = st[PT_B_SUM] + (dc - st[PT_B_D0]);
                                st[PT_BASE] = st[PT_B_D0] + st[PT_B_SUM] / st[PT_B_N];
                                st[PT_HAS_BASE] = 1.0;
                            }
                        } else if (P.baseline_tau > 0.0) {
                            if (st[PT_HAS_BASE] == 0.0 || st[PT_HAS_PREV] == 0.0) st[PT_BASE] = dc;
                            else st[PT_BASE] = st[PT_BASE] + (1.0 / (1.0 + P.baseline_tau / dt)) * (dc - st[PT_BASE]);
                            st[PT_HAS_BASE] = 1.0;
                        }
                        if ((baseline_mark || P.baseline_tau > 0.0) && st[PT_HAS_BASE] != 0.0) {
                            o_cmm = dc - st[PT_BASE];
                            o_cpct = 100.0 * (dc - st[PT_BASE]) / st[PT_BASE];
                        }
                        // the episodes
                        const int phase = vel > P.dilate ? 1 : (vel < -P.constrict ? -1 : 0);
                        if (st[PT_EP_OPEN] != 0.0 && (double)phase != st[PT_EP_PHASE]) pt_close(st, rows, V, s_cd, P.min_amplitude);
                        if (phase != 0) {
                            if (st[PT_EP_OPEN] == 0.0) {
                                st[PT_EP_OPEN] = 1.0;
                                st[PT_EP_PHASE] = (double)phase;
                                st[PT_EP_T_START] = st[PT_T_PREV];
                                st[PT_EP_D_START] = st[PT_DF];
                                st[PT_EP_PEAK] = 0.0;
                                st[PT_EP_SAMPLES] = 0.0;
                                st[PT_EP_LF] = lit ? st[PT_LF] : 0.0;
                            }
                            st[PT_EP_T_END] = tt;
                            st[PT_EP_D_END] = df;
                            if (fabs(vel) > st[PT_EP_PEAK]) st[PT_EP_PEAK] = fabs(vel);
                            st[PT_EP_SAMPLES] = st[PT_EP_SAMPLES] + 1.0;
                        }
                        // the table's statistics of the trace
                        if (tab[PT_BOTH] + tab[PT_LEFT] + tab[PT_RIGHT] == 1.0) {
                            tab[PT_D0] = dc;
                            tab[PT_MIN] = dc;
                            tab[PT_MAX] = dc;
                        }
                        const double dd = dc - tab[PT_D0];
                        tab[PT_S1] = tab[PT_S1] + dd;
                        tab[PT_S2] = tab[PT_S2] + dd * dd;
                        if (dc < tab[PT_MIN]) tab[PT_MIN] = dc;
                        if (dc > tab[PT_MAX]) tab[PT_MAX] = dc;
                        // hand over
                        if (acc[0]) {
                            st[PT_HAS_L] = 1.0;
                            st[PT_T_L] = tt;
                            st[PT_V_L] = l;
                        }
                        if (acc[1]) {
                            st[PT_HAS_R] = 1.0;
                            st[PT_T_R] = tt;
                            st[PT_V_R] = r;
                        }
                        st[PT_HAS_PREV] = 1.0;
                        st[PT_T_PREV] = tt;
                        st[PT_DF] = df;
                        st[PT_LAST_IDX] = idx;
                        o_mm = dc;
                        o_raw = d;
                        o_vel = vel;
                        code |= 1 | (acc[0] ? 2 : 0) | (acc[1] ? 4 : 0) | ((phase == 1 ? 1 : (phase == -1 ? 2 : 0)) << 11);
                    }
                    if (baseline_mark) st[PT_PREV_MARK] = (flag & PT_F_MARK) != 0 ? 1.0 : 0.0;
                }
                s_out[0][t] = o_mm;
                s_out[1][t] = o_raw;
                s_out[2][t] = o_vel;
                s_out[3][t] = o_cmm;
                s_out[4][t] = o_cpct;
                s_flag[t] = code;
            }
        }
        __syncthreads();
        // ---- phase 2
        if (f < T) {
            const int code = s_flag[lane];
            out_mm[n] = (float)s_out[0][lane];
            out_raw[n] = (float)s_out[1][lane];
            out_velocity[n] = (float)s_out[2][lane];
            out_change_mm[n] = (float)s_out[3][lane];
            out_change_pct[n] = (float)s_out[4][lane];
            out_valid[n] = (uint8_t)(code & 1);
            out_used[n * 2] = (uint8_t)((code >> 1) & 1);
            out_used[n * 2 + 1] = (uint8_t)((code >> 2) & 1);
            out_reason[n * 2] = (uint8_t)((code >> 3) & 15);
            out_reason[n * 2 + 1] = (uint8_t)((code >> 7) & 15);
            out_event[n] = (uint8_t)((code >> 11) & 3);
        }
        __syncthreads();
    }
    if (lane == 0) {
        st[PT_TICKS] = ticks0 + (double)len;
        if (flush && flush[b] != 0) pt_close(st, rows, V, s_cd, P.min_amplitude);
        count[b] = s_cd[0];
        dropped[b] = s_cd[1];
    }
    __syncthreads();
    if (lane < PT_STATE) row[lane] = st[lane];
    if (lane < PT_TABLE) trow[lane] = tab[lane];
}

__host__ bool pt_positive(const double x) { return x > 0.0 && x <= 1.79769313486231570815e308; }
__host__ bool pt_not_negative(const double x) { return x >= 0.0 && x <= 1.79769313486231570815e308; }

}  // namespace
}  // namespace eve

using namespace eve;

extern "C" int eve_pupil_track(long long B, int T, const float* size, const uint8_t* eye_valid, const double* frame_time, const int* lengths,
                               const int* reset, const int* flush, const float* luminance, const uint8_t* baseline_mark, double fps,
                               double min_mm, double max_mm, double max_speed_mm_s, double max_gap_s, double offset_rate, double cutoff_hz,
                               double light_tau_s, double baseline_tau_s, double dilate_mm_s, double constrict_mm_s, double min_amplitude_mm,
                               double* state, double* table, double* light, int capacity, double* store, int* count, int* dropped, float* mm,
                               float* raw_mm, float* velocity, float* change_mm, float* change_pct, uint8_t* valid, uint8_t* eye_used,
                               uint8_t* eye_reason, uint8_t* event, eve_stream_t stream) {
    const char* why = nullptr;
    const long long LIM = 0x7fffffff;
    if (!state || !table || !light || !store || !count || !dropped) why = "a null carried buffer";
    else if (B < 1 || T < 0 || capacity < 1) why = "B >= 1, T >= 0 and capacity >= 1";
    else if (T > 0 && (!size || !mm || !raw_mm || !velocity || !change_mm || !change_pct || !valid || !eye_used || !eye_reason || !event))
        why = "a null frame input or output with T > 0";
    else if (B > LIM / PT_STATE) why = "B * 32 must fit 31 bits";
    else if (B > LIM / PT_ROW / capacity) why = "B * capacity * 8 must fit 31 bits";
    else if (T > 0 && B > LIM / 2 / T) why = "B * T * 2 must fit 31 bits";
    else if (!(pt_positive(min_mm) && pt_positive(max_mm) && min_mm < max_mm)) why = "min_mm and max_mm must be finite numbers > 0 with min_mm < max_mm";
    else if (!pt_positive(max_speed_mm_s)) why = "max_speed_mm_s must be a finite number > 0";
    else if (!pt_positive(max_gap_s)) why = "max_gap_s must be a finite number > 0";
    else if (!(offset_rate > 0.0 && offset_rate <= 1.0)) why = "offset_rate must lie in (0, 1]";
    else if (!pt_positive(cutoff_hz)) why = "cutoff_hz must be a finite number > 0";
    else if (!pt_positive(light_tau_s)) why = "light_tau_s must be a finite number > 0";
    else if (!pt_not_negative(baseline_tau_s)) why = "baseline_tau_s must be a finite number >= 0 (0: no follower)";
    else if (!pt_positive(dilate_mm_s)) why = "dilate_mm_s must be a finite number > 0";
    else if (!pt_positive(constrict_mm_s)) why = "constrict_mm_s must be a finite number > 0";
    else if (!pt_not_negative(min_amplitude_mm)) why = "min_amplitude_mm must be a finite number >= 0";
    else if (T > 0 && !frame_time && !pt_positive(fps)) why = "without frame_time, fps must be a finite number > 0";
    if (why) {
        char msg[160];
        snprintf(msg, sizeof(msg), "pupil_track: %s", why);
        return set_error_msg(msg);
    }
    const PupilParams P = {frame_time ? 1.0 : fps, min_mm, max_mm, max_speed_mm_s, max_gap_s, offset_rate, cutoff_hz, light_tau_s,
                           baseline_tau_s, dilate_mm_s, constrict_mm_s, min_amplitude_mm};
    EVE_LAUNCH("pupil_track_kernel", pupil_track_kernel, dim3((unsigned)B), dim3(PT_WAVE), 0, (hipStream_t)stream, T, size, B * T, eye_valid,
               frame_time, lengths, reset, flush, luminance, baseline_mark, P, state, table, light, capacity, store, count, dropped, mm, raw_mm,
               velocity, change_mm, change_pct, valid, eye_used, eye_reason, event);
    EVE_CHECK_LAUNCH();
    return 0;
}
