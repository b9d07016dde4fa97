// Saccades as events, on the device: the other half of the fixation / saccade detector.  eve_gaze_events labels every frame; this
// stage cuts the runs of saccade frames into events with amplitude, duration, peak and mean velocity and the fixations before and
// after them, keeps a table of tallies (the sums behind the main sequence) and appends accepted saccades to the stream's store.  Its
// inputs are what eve_gaze_events_ex hands out -- the sample flags, the sample times and the gaze vectors -- and the events' own
// labels, velocities and fixation ids.  The contract -- the rules, the state row, the table and the store row -- is in
// include/eve_hip.h (eve_gaze_saccades) and in numpy in tests/saccade_ref.py.
//
// One wavefront (a 64-thread workgroup) per stream; the frames go by in passes of 64, each pass in phases, its intermediates in LDS:
//   0  parallel   lane t reads frame t's inputs into LDS
//   1  serial     lane 0 walks the state machine (no transcendental), writes the per-frame results into LDS and lists the saccades
//                 that close in this pass: at most one per frame, so at most 64
//   2  parallel   lane j computes closing j's amplitude (sqrt, atan2: the one long dependency chain)
//   3  serial     lane 0 judges, tallies and appends the closings in order
//   4  parallel   lane t writes frame t's two outputs
// Float64 throughout, every operation rounded on its own: the bits do not depend on this structure.  Every branch around a barrier
// is uniform over the wave.
#include "common.h"

#pragma clang fp contract(off)

namespace eve {
namespace {

constexpr int GS_WAVE = 64;
constexpr int GS_STATE = 32;             // doubles per state row (include/eve_hip.h has the layout)
constexpr int GS_ROW = 16;               // doubles per table row and per stored saccade
enum { GS_HAS_PREV = 0, GS_T_PREV, GS_PV0, GS_PV1, GS_PV2, GS_PX, GS_PY, GS_P_EVENT, GS_P_FIX, GS_OPEN, GS_ID, GS_NEXT_ID, GS_T_ONSET, GS_OV0,
       GS_OV1, GS_OV2, GS_X0, GS_Y0, GS_N, GS_PEAK, GS_MISSING, GS_PREV_FIX };
enum { GS_ACCEPTED = 0, GS_SUM_A, GS_SUM_AA, GS_SUM_P, GS_SUM_AP, GS_SUM_D, GS_SUM_AD, GS_MAX_A, GS_MAX_P, GS_ABORTED, GS_SMALL, GS_SHORT,
       GS_LONG, GS_INTERRUPTED };
// a closing's record (s_c[k][j]): what phase 1 lists, phase 2 completes and phase 3 judges
enum { GC_ID = 0, GC_T0, GC_T1, GC_N, GC_X0, GC_Y0, GC_X1, GC_Y1, GC_AMP, GC_PEAK, GC_PREV_FIX, GC_NEXT_FIX, GC_MISSING, GC_OV0, GC_OV1, GC_OV2,
       GC_LV0, GC_LV1, GC_LV2, GC_FIELDS };

struct GsParams {
    double min_amp, min_dur, max_dur;
    int max_missing;
};

// Aborts the open saccade of the state row st (lane 0 only): a tally, nothing stored.
__device__ __forceinline__ void gs_abort(double* st, double* tab) {
    if (st[GS_OPEN] == 0.0) return;
    st[GS_OPEN] = 0.0;
    tab[GS_ABORTED] = tab[GS_ABORTED] + 1.0;
}

__global__ __launch_bounds__(GS_WAVE) void gaze_saccades_kernel(const int T, const uint8_t* __restrict__ sample,
                                                                const double* __restrict__ sample_time,
                                                                const double* __restrict__ gaze_vector, const float* __restrict__ point,
                                                                const uint8_t* __restrict__ event, const float* __restrict__ velocity,
                                                                const int* __restrict__ fixation_id, const int* __restrict__ lengths,
                                                                const int* __restrict__ reset, const GsParams P, double* __restrict__ state,
                                                                double* __restrict__ table, const int S, double* __restrict__ store,
                                                                int* __restrict__ count, int* __restrict__ dropped,
                                                                int* __restrict__ saccade_id, float* __restrict__ saccade_ms) {
#pragma clang fp contract(off)
    __shared__ double st[GS_STATE], s_tab[GS_ROW];
    __shared__ double s_tt[GS_WAVE], s_v[3][GS_WAVE], s_px[GS_WAVE], s_py[GS_WAVE], s_vel[GS_WAVE], s_ms[GS_WAVE];
    __shared__ double s_c[GC_FIELDS][GS_WAVE];
    __shared__ int s_flag[GS_WAVE], s_event[GS_WAVE], s_fix[GS_WAVE], s_id[GS_WAVE];
    __shared__ int s_cd[2], s_nc;                                      // the stream's count and dropped, the pass's closings (lane 0's)
    const int lane = threadIdx.x;
    const long long b = blockIdx.x;
    double* row = state + (size_t)b * GS_STATE;
    double* tab = table + (size_t)b * GS_ROW;
    double* rows = store + (size_t)b * S * GS_ROW;
    if (lane < GS_STATE) st[lane] = row[lane];
    if (lane < GS_ROW) s_tab[lane] = tab[lane];
    __syncthreads();
    if (lane == 0) {
        s_cd[0] = min(max(count[b], 0), S);
        s_cd[1] = dropped[b];
        if (reset && reset[b] != 0) {
            gs_abort(st, s_tab);
            const double keep = st[GS_NEXT_ID];
            for (int i = 0; i < GS_STATE; ++i) st[i] = 0.0;
            st[GS_NEXT_ID] = keep;
        }
    }
    __syncthreads();
    int len = T;
    if (lengths) len = min(max(lengths[b], 0), T);
    for (int base = 0; base < T; base += GS_WAVE) {                    // (T, base, len: the same in every lane)
        const int f = base + lane;
        const long long n = b * T + f;
        // ---- phase 0
        int flag = 0;
        if (f < len) {
            flag = (int)sample[n];
            s_tt[lane] = sample_time[n];
            s_v[0][lane] = gaze_vector[n * 3];
            s_v[1][lane] = gaze_vector[n * 3 + 1];
            s_v[2][lane] = gaze_vector[n * 3 + 2];
            s_px[lane] = (double)point[n * 2];
            s_py[lane] = (double)point[n * 2 + 1];
            s_vel[lane] = (double)velocity[n];
            s_event[lane] = (int)event[n];
            s_fix[lane] = fixation_id[n];
        }
        s_flag[lane] = flag;
        __syncthreads();
        // ---- phase 1
        if (lane == 0) {
            int nc = 0;
            const int m = min(GS_WAVE, T - base), ml = min(GS_WAVE, len - base);
            for (int t = 0; t < m; ++t) {
                int id = -1;
                double ms = 0.0;
                const int fl = t < ml ? s_flag[t] : 0;
                if (fl == 0) {
                    if (t < ml && st[GS_OPEN] != 0.0) st[GS_MISSING] = st[GS_MISSING] + 1.0;
                } else {
                    const double tt = s_tt[t];
                    const int ev = fl == 2 ? s_event[t] : 0;           // (a restarting sample carries no label)
                    if (fl != 2 || (ev != 1 && ev != 2)) {
                        gs_abort(st, s_tab);
                    } else if (ev == 2) {
                        if (st[GS_OPEN] == 0.0 && st[GS_HAS_PREV] != 0.0 && st[GS_P_EVENT] != 2.0) {
                            st[GS_OPEN] = 1.0;
                            st[GS_ID] = st[GS_NEXT_ID];
                            st[GS_NEXT_ID] = st[GS_NEXT_ID] + 1.0;
                            st[GS_T_ONSET] = st[GS_T_PREV];
                            st[GS_OV0] = st[GS_PV0];
                            st[GS_OV1] = st[GS_PV1];
                            st[GS_OV2] = st[GS_PV2];
                            st[GS_X0] = st[GS_PX];
                            st[GS_Y0] = st[GS_PY];
                            st[GS_N] = 0.0;
                            st[GS_PEAK] = 0.0;
                            st[GS_MISSING] = 0.0;
                            st[GS_PREV_FIX] = st[GS_P_EVENT] == 1.0 ? st[GS_P_FIX] : -1.0;
                        }
                        if (st[GS_OPEN] != 0.0) {
                            st[GS_N] = st[GS_N] + 1.0;
                            if (s_vel[t] > st[GS_PEAK]) st[GS_PEAK] = s_vel[t];
                            id = (int)st[GS_ID];
                            ms = 1000.0 * (tt - st[GS_T_ONSET]);
                        }
                    } else if (st[GS_OPEN] != 0.0) {                   // a fixation frame: the saccade lands at the previous sample
                        st[GS_OPEN] = 0.0;
                        s_c[GC_ID][nc] = st[GS_ID];
                        s_c[GC_T0][nc] = st[GS_T_ONSET];
                        s_c[GC_T1][nc] = st[GS_T_PREV];
                        s_c[GC_N][nc] = st[GS_N];
                        s_c[GC_X0][nc] = st[GS_X0];
                        s_c[GC_Y0][nc] = st[GS_Y0];
                        s_c[GC_X1][nc] = st[GS_PX];
                        s_c[GC_Y1][nc] = st[GS_PY];
                        s_c[GC_PEAK][nc] = st[GS_PEAK];
                        s_c[GC_PREV_FIX][nc] = st[GS_PREV_FIX];
                        s_c[GC_NEXT_FIX][nc] = (double)s_fix[t];
                        s_c[GC_MISSING][nc] = st[GS_MISSING];
                        s_c[GC_OV0][nc] = st[GS_OV0];
                        s_c[GC_OV1][nc] = st[GS_OV1];
                        s_c[GC_OV2][nc] = st[GS_OV2];
                        s_c[GC_LV0][nc] = st[GS_PV0];
                        s_c[GC_LV1][nc] = st[GS_PV1];
                        s_c[GC_LV2][nc] = st[GS_PV2];
                        ++nc;
                    }
                    st[GS_HAS_PREV] = 1.0;
                    st[GS_T_PREV] = tt;
                    st[GS_PV0] = s_v[0][t];
                    st[GS_PV1] = s_v[1][t];
                    st[GS_PV2] = s_v[2][t];
                    st[GS_PX] = s_px[t];
                    st[GS_PY] = s_py[t];
                    st[GS_P_EVENT] = (double)ev;
                    st[GS_P_FIX] = (double)s_fix[t];
                }
                s_id[t] = id;
                s_ms[t] = ms;
            }
            s_nc = nc;
        }
        __syncthreads();
        // ---- phase 2
        const int nc = s_nc;                                           // (the same in every lane)
        if (lane < nc) {
            const double p0 = s_c[GC_OV0][lane], p1 = s_c[GC_OV1][lane], p2 = s_c[GC_OV2][lane];
            const double v0 = s_c[GC_LV0][lane], v1 = s_c[GC_LV1][lane], v2 = s_c[GC_LV2][lane];
            const double c0 = p1 * v2 - p2 * v1, c1 = p2 * v0 - p0 * v2, c2 = p0 * v1 - p1 * v0;
            const double angle = atan2(sqrt((c0 * c0 + c1 * c1) + c2 * c2), (p0 * v0 + p1 * v1) + p2 * v2);
            s_c[GC_AMP][lane] = angle * 57.29577951308232;
        }
        __syncthreads();
        // ---- phase 3
        if (lane == 0) {
            for (int j = 0; j < nc; ++j) {
                const double amp = s_c[GC_AMP][j], dur = s_c[GC_T1][j] - s_c[GC_T0][j], peak = s_c[GC_PEAK][j], missing = s_c[GC_MISSING][j];
                if (missing > (double)P.max_missing) s_tab[GS_INTERRUPTED] = s_tab[GS_INTERRUPTED] + 1.0;
                else if (dur > P.max_dur) s_tab[GS_LONG] = s_tab[GS_LONG] + 1.0;
                else if (dur < P.min_dur) s_tab[GS_SHORT] = s_tab[GS_SHORT] + 1.0;
                else if (!(amp >= P.min_amp)) s_tab[GS_SMALL] = s_tab[GS_SMALL] + 1.0;
                else {
                    s_tab[GS_ACCEPTED] = s_tab[GS_ACCEPTED] + 1.0;
                    s_tab[GS_SUM_A] = s_tab[GS_SUM_A] + amp;
                    s_tab[GS_SUM_AA] = s_tab[GS_SUM_AA] + amp * amp;
                    s_tab[GS_SUM_P] = s_tab[GS_SUM_P] + peak;
                    s_tab[GS_SUM_AP] = s_tab[GS_SUM_AP] + amp * peak;
                    s_tab[GS_SUM_D] = s_tab[GS_SUM_D] + dur;
                    s_tab[GS_SUM_AD] = s_tab[GS_SUM_AD] + amp * dur;
                    if (amp > s_tab[GS_MAX_A]) s_tab[GS_MAX_A] = amp;
                    if (peak > s_tab[GS_MAX_P]) s_tab[GS_MAX_P] = peak;
                    const int cnt = s_cd[0];
                    if (cnt >= S) {
                        s_cd[1] = s_cd[1] + 1;
                    } else {
                        double* dst = rows + (size_t)cnt * GS_ROW;
                        dst[0] = s_c[GC_ID][j];
                        dst[1] = s_c[GC_T0][j];
                        dst[2] = s_c[GC_T1][j];
                        dst[3] = s_c[GC_N][j];
                        dst[4] = s_c[GC_X0][j];
                        dst[5] = s_c[GC_Y0][j];
                        dst[6] = s_c[GC_X1][j];
                        dst[7] = s_c[GC_Y1][j];
                        dst[8] = amp;
                        dst[9] = peak;
                        dst[10] = amp / dur;
                        dst[11] = s_c[GC_PREV_FIX][j];
                        dst[12] = s_c[GC_NEXT_FIX][j];
                        dst[13] = missing;
                        dst[14] = 0.0;
                        dst[15] = 0.0;
                        s_cd[0] = cnt + 1;
                    }
                }
            }
        }
        // ---- phase 4 (s_id and s_ms were written in phase 1, two barriers ago)
        if (f < T) {
            saccade_id[n] = s_id[lane];
            saccade_ms[n] = (float)s_ms[lane];
        }
        __syncthreads();
    }
    if (lane == 0) {
        count[b] = s_cd[0];
        dropped[b] = s_cd[1];
    }
    __syncthreads();
    if (lane < GS_STATE) row[lane] = st[lane];
    if (lane < GS_ROW) tab[lane] = s_tab[lane];
}

__host__ bool gs_finite(const double x) { return x >= -1.79769313486231570815e308 && x <= 1.79769313486231570815e308; }      // false for a NaN

}  // namespace
}  // namespace eve

using namespace eve;

extern "C" int eve_gaze_saccades(long long B, int T, const uint8_t* sample, const double* sample_time, const double* gaze_vector,
                                 const float* point, const uint8_t* event, const float* velocity, const int* fixation_id, const int* lengths,
                                 const int* reset, double min_amplitude_deg, double min_duration_s, double max_duration_s, int max_missing,
                                 double* state, double* table, int S, double* store, int* count, int* dropped, int* saccade_id,
                                 float* saccade_ms, eve_stream_t stream) {
    const char* why = nullptr;
    const long long LIM = 0x7fffffff;
    if (!state || !table || !store || !count || !dropped) why = "a null carried buffer";
    else if (B < 1 || T < 0 || S <= 0) why = "B >= 1, T >= 0 and a store capacity S >= 1";
    else if (T > 0 && (!sample || !sample_time || !gaze_vector || !point || !event || !velocity || !fixation_id || !saccade_id || !saccade_ms))
        why = "a null frame input or output with T > 0";
    else if (B > LIM / GS_STATE) why = "B * 32 must fit 31 bits";
    else if (B > LIM / GS_ROW / S) why = "B * S * 16 must fit 31 bits";
    else if (T > 0 && B > LIM / 3 / T) why = "B * T * 3 must fit 31 bits";
    else if (!gs_finite(min_amplitude_deg) || !gs_finite(min_duration_s) || !gs_finite(max_duration_s)) why = "the thresholds must be finite";
    else if (min_amplitude_deg < 0.0) why = "min_amplitude_deg must be >= 0";
    else if (max_duration_s <= 0.0) why = "max_duration_s must be > 0";
    else if (min_duration_s < 0.0) why = "min_duration_s must be >= 0";
    else if (max_missing < 0) why = "max_missing must be >= 0";
    if (why) {
        char msg[160];
        snprintf(msg, sizeof(msg), "gaze_saccades: %s", why);
        return set_error_msg(msg);
    }
    GsParams P;
    P.min_amp = min_amplitude_deg;
    P.min_dur = min_duration_s;
    P.max_dur = max_duration_s;
    P.max_missing = max_missing;
    EVE_LAUNCH("gaze_saccades_kernel", gaze_saccades_kernel, dim3((unsigned)B), dim3(GS_WAVE), 0, (hipStream_t)stream, T, sample, sample_time,
               gaze_vector, point, event, velocity, fixation_id, lengths, reset, P, state, table, S, store, count, dropped, saccade_id, saccade_ms);
    EVE_CHECK_LAUNCH();
    return 0;
}
