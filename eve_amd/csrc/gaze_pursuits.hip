// Smooth pursuit, on the device: the third gaze class beside the fixations and saccades of eve_gaze_events.  On a moving target the
// eye moves at a few degrees per second, far below the saccade threshold, so the events stage labels those frames fixations.  This
// stage looks at each fixation-labelled sample over a window of the chained samples before it -- how far the gaze vector turned in
// the window, and how straight it went -- promotes the frames of steady, straight motion to the pursuit class, cuts them into
// episodes with amplitude, direction, mean and peak velocity, path length and, where the pursued object's position is given, gain and
// position error, keeps a table of tallies and appends accepted episodes to the stream's store.  Its inputs are those of
// eve_gaze_saccades plus the optional target.  The contract -- the rules, the state row, the table and the store row -- is in
// include/eve_hip.h (eve_gaze_pursuits) and in numpy in tests/pursuit_ref.py.
//
// One wavefront (a 64-thread workgroup) per stream; the frames go by in passes of 64, each pass in phases, its intermediates in LDS.
// The samples live in 96 slots -- 0 .. 31 the carried ring, 32 + t frame t of the pass -- and the pass's timeline lists the slots of
// the admitted samples in order:
//   0  parallel   lane t reads frame t's inputs into slot 32 + t
//   1  serial     lane 0 admits samples to the timeline (restarts, saccades, the settling time, the running path length: no
//                 transcendental) and gives each run sample its timeline index and its run's first index
//   2  parallel   lane t searches back at most 31 entries for its window's oldest entry and computes the window's angle (sqrt, atan2:
//                 the one long dependency chain, once PER SAMPLE), velocity, straightness, gain and the candidate flag
//   3  serial     lane 0 walks the episode state machine over the flags and lists the episodes that close in this pass
//   4  parallel   lane j computes closing j's amplitude and direction (two atan2)
//   5  serial     lane 0 judges, tallies and appends the closings in order
//   6  parallel   lane t writes frame t's six outputs; the run's last <= 32 timeline entries move to slots 0 .. 31
// Float64 throughout, every operation rounded on its own: the bits do not depend on this structure.  Every branch around a barrier
// is uniform over the wave.
#include "common.h"

#pragma clang fp contract(off)

namespace eve {
namespace {

constexpr int GP_WAVE = 64;
constexpr int GP_SCALARS = 32;           // the state row: 32 scalars, then 32 ring entries of 9 doubles (include/eve_hip.h has the layout)
constexpr int GP_RING = 32;
constexpr int GP_ENTRY = 9;
constexpr int GP_STATE = GP_SCALARS + GP_RING * GP_ENTRY;
constexpr int GP_SLOTS = GP_RING + GP_WAVE;
constexpr int GP_TABLE = 16;             // doubles per table row
constexpr int GP_ROW = 20;               // doubles per stored episode
enum { GP_RING_N = 0, GP_SEEN_SACCADE, GP_T_SACCADE, GP_OPEN, GP_ID, GP_NEXT_ID, GP_T_ONSET, GP_OV0, GP_OV1, GP_OV2, GP_X0, GP_Y0, GP_CUM_ONSET,
       GP_N, GP_PEAK, GP_MISSING, GP_FIX, GP_T_LAST, GP_LV0, GP_LV1, GP_LV2, GP_X1, GP_Y1, GP_CUM_LAST, GP_GAIN_SUM, GP_GAIN_N, GP_ERR_SUM,
       GP_HAS_END, GP_T_END };
enum { GE_T = 0, GE_V0, GE_V1, GE_V2, GE_CUM, GE_X, GE_Y, GE_TX, GE_TY };
enum { GP_ACCEPTED = 0, GP_SUM_DUR, GP_SUM_AMP, GP_SUM_PATH, GP_SUM_MEAN_V, GP_MAX_PEAK, GP_SUM_GAIN, GP_TAB_GAIN_N, GP_ABORTED, GP_SMALL,
       GP_SHORT, GP_INTERRUPTED };
// what phase 1 makes of a frame
enum { GK_PAD = 0, GK_NONE, GK_RESTART, GK_SACCADE, GK_SETTLE, GK_RUN };
// a closing's record (s_c[k][j]): what phase 3 lists, phase 4 completes and phase 5 judges
enum { GC_ID = 0, GC_T0, GC_T1, GC_N, GC_X0, GC_Y0, GC_X1, GC_Y1, GC_AMP, GC_DIR, GC_PEAK, GC_PATH, GC_FIX, GC_MISSING, GC_GAIN_N, GC_GAIN_SUM,
       GC_ERR_SUM, GC_OV0, GC_OV1, GC_OV2, GC_LV0, GC_LV1, GC_LV2, GC_FIELDS };
constexpr int GP_MAX_CLOSINGS = 33;      // a closing needs a candidate frame since the one before: at most every other frame

struct GpParams {
    double window, min_window, pursuit, straight, settle, min_dur, min_amp;
    int max_missing;
};

__device__ __forceinline__ bool gp_finite(const double x) { return fabs(x) <= 1.79769313486231570815e308; }      // false for a NaN

// the angle between two gaze vectors in degrees: the events stage's expression
__device__ __forceinline__ double gp_angle(const double p0, const double p1, const double p2, const double v0, const double v1, const double v2) {
#pragma clang fp contract(off)
    const double c0 = p1 * v2 - p2 * v1, c1 = p2 * v0 - p0 * v2, c2 = p0 * v1 - p1 * v0;
    return atan2(sqrt((c0 * c0 + c1 * c1) + c2 * c2), (p0 * v0 + p1 * v1) + p2 * v2) * 57.29577951308232;
}

// Aborts the open episode of the state row st (lane 0 only): a tally, nothing stored.
__device__ __forceinline__ void gp_abort(double* st, double* tab) {
    if (st[GP_OPEN] == 0.0) return;
    st[GP_OPEN] = 0.0;
    tab[GP_ABORTED] = tab[GP_ABORTED] + 1.0;
}

__global__ __launch_bounds__(GP_WAVE) void gaze_pursuits_kernel(
    const int T, const uint8_t* __restrict__ sample, const double* __restrict__ sample_time, const double* __restrict__ gaze_vector,
    const float* __restrict__ point, const uint8_t* __restrict__ event, const float* __restrict__ velocity, const int* __restrict__ fixation_id,
    const float* __restrict__ target, const int* __restrict__ lengths, const int* __restrict__ reset, const GpParams P,
    double* __restrict__ state, double* __restrict__ table, const int S, double* __restrict__ store, int* __restrict__ count,
    int* __restrict__ dropped, uint8_t* __restrict__ gaze_class, int* __restrict__ pursuit_id, float* __restrict__ pursuit_ms,
    float* __restrict__ windowed, float* __restrict__ straightness, float* __restrict__ pursuit_gain) {
#pragma clang fp contract(off)
    __shared__ double st[GP_SCALARS], s_tab[GP_TABLE];
    __shared__ double s_e[GP_ENTRY][GP_SLOTS];                         // the samples' slots
    __shared__ double s_vel[GP_WAVE], s_w[GP_WAVE], s_s[GP_WAVE], s_gain[GP_WAVE], s_err[GP_WAVE], s_ms[GP_WAVE];
    __shared__ double s_c[GC_FIELDS][GP_MAX_CLOSINGS];
    __shared__ int s_tl[GP_SLOTS];                                     // the timeline: the admitted samples' slots, in order
    __shared__ int s_flag[GP_WAVE], s_event[GP_WAVE], s_fix[GP_WAVE], s_kind[GP_WAVE], s_idx[GP_WAVE], s_first[GP_WAVE], s_j[GP_WAVE];
    __shared__ int s_has[GP_WAVE], s_gdef[GP_WAVE], s_cand[GP_WAVE], s_cls[GP_WAVE], s_id[GP_WAVE];
    __shared__ int s_cd[2], s_nc, s_ntl, s_rf;                         // count and dropped, the pass's closings, the timeline's length and its run's first index
    const int lane = threadIdx.x;
    const long long b = blockIdx.x;
    double* row = state + (size_t)b * GP_STATE;
    double* tab = table + (size_t)b * GP_TABLE;
    double* rows = store + (size_t)b * S * GP_ROW;
    if (lane < GP_SCALARS) st[lane] = row[lane];
    if (lane < GP_TABLE) s_tab[lane] = tab[lane];
    for (int i = lane; i < GP_RING * GP_ENTRY; i += GP_WAVE) s_e[i % GP_ENTRY][i / GP_ENTRY] = row[GP_SCALARS + i];
    for (int i = lane; i < GP_SLOTS; i += GP_WAVE) s_tl[i] = i;
    __syncthreads();
    if (lane == 0) {
        s_cd[0] = min(max(count[b], 0), S);
        s_cd[1] = dropped[b];
        if (reset && reset[b] != 0) {
            gp_abort(st, s_tab);
            const double keep = st[GP_NEXT_ID];
            for (int i = 0; i < GP_SCALARS; ++i) st[i] = 0.0;          // (ring_n = 0: the ring is empty)
            st[GP_NEXT_ID] = keep;
        }
        const double rn = st[GP_RING_N];
        s_ntl = rn >= 1.0 ? (rn <= (double)GP_RING ? (int)rn : GP_RING) : 0;
        s_rf = 0;
    }
    __syncthreads();
    int len = T;
    if (lengths) len = min(max(lengths[b], 0), T);
    for (int base = 0; base < T; base += GP_WAVE) {                    // (T, base, len: the same in every lane)
        const int f = base + lane;
        const long long n = b * T + f;
        const int mine = GP_RING + lane;
        // ---- phase 0
        int flag = 0;
        if (f < len) {
            flag = (int)sample[n];
            s_e[GE_T][mine] = sample_time[n];
            s_e[GE_V0][mine] = gaze_vector[n * 3];
            s_e[GE_V1][mine] = gaze_vector[n * 3 + 1];
            s_e[GE_V2][mine] = gaze_vector[n * 3 + 2];
            s_e[GE_X][mine] = (double)point[n * 2];
            s_e[GE_Y][mine] = (double)point[n * 2 + 1];
            s_e[GE_TX][mine] = target ? (double)target[n * 2] : __builtin_nan("");
            s_e[GE_TY][mine] = target ? (double)target[n * 2 + 1] : __builtin_nan("");
            s_vel[lane] = (double)velocity[n];
            s_event[lane] = (int)event[n];
            s_fix[lane] = fixation_id[n];
        }
        s_flag[lane] = flag;
        __syncthreads();
        const int m = min(GP_WAVE, T - base), ml = min(GP_WAVE, len - base);      // the pass's frames, and those below lengths[b]
        // ---- phase 1
        if (lane == 0) {
            int ntl = s_ntl, rf = s_rf;
            for (int t = 0; t < m; ++t) {
                int kind = GK_PAD;
                if (t < ml) {
                    const int fl = s_flag[t], slot = GP_RING + t;
                    const double tt = s_e[GE_T][slot];
                    const int ev = fl == 2 ? s_event[t] : 0;           // (a restarting sample carries no label)
                    if (fl == 0) {
                        kind = GK_NONE;
                    } else if (fl != 2 || (ev != 1 && ev != 2)) {      // the run is emptied, and this sample is its first entry
                        kind = GK_RESTART;
                        st[GP_SEEN_SACCADE] = 0.0;
                        rf = ntl;
                        s_e[GE_CUM][slot] = 0.0;
                        s_tl[ntl++] = slot;
                    } else if (ev == 2) {                              // the run is emptied
                        kind = GK_SACCADE;
                        rf = ntl;
                        st[GP_SEEN_SACCADE] = 1.0;
                        st[GP_T_SACCADE] = tt;
                    } else if (st[GP_SEEN_SACCADE] != 0.0 && tt - st[GP_T_SACCADE] < P.settle) {
                        kind = GK_SETTLE;
                    } else {
                        kind = GK_RUN;
                        double cum = 0.0;
                        if (ntl > rf) {
                            const int last = s_tl[ntl - 1];
                            cum = s_e[GE_CUM][last] + s_vel[t] * (tt - s_e[GE_T][last]);
                        }
                        s_e[GE_CUM][slot] = cum;
                        s_idx[t] = ntl;
                        s_first[t] = rf;
                        s_tl[ntl++] = slot;
                    }
                }
                s_kind[t] = kind;
            }
            s_ntl = ntl;
            s_rf = rf;
        }
        __syncthreads();
        // ---- phase 2
        {
            int has = 0, gdef = 0, cand = 0, j = 0;
            double w = 0.0, s = 0.0, gain = 0.0, err = 0.0;
            if (lane < m && s_kind[lane] == GK_RUN) {
                const int i = s_idx[lane], lo = max(s_first[lane], i - (GP_RING - 1));
                const double tt = s_e[GE_T][mine];
                j = i;
                while (j > lo && tt - s_e[GE_T][s_tl[j - 1]] <= P.window) --j;
                const int e = s_tl[j];
                const double span = tt - s_e[GE_T][e];
                if (!(span < P.min_window)) {
                    has = 1;
                    const double a = gp_angle(s_e[GE_V0][e], s_e[GE_V1][e], s_e[GE_V2][e], s_e[GE_V0][mine], s_e[GE_V1][mine], s_e[GE_V2][mine]);
                    w = a / span;
                    const double path = s_e[GE_CUM][mine] - s_e[GE_CUM][e];
                    s = path > 0.0 ? a / path : 0.0;
                    cand = (w >= P.pursuit && s >= P.straight) ? 1 : 0;
                    const double x = s_e[GE_X][mine], y = s_e[GE_Y][mine], tx = s_e[GE_TX][mine], ty = s_e[GE_TY][mine];
                    const double txj = s_e[GE_TX][e], tyj = s_e[GE_TY][e];
                    if (gp_finite(tx) && gp_finite(ty) && gp_finite(txj) && gp_finite(tyj)) {
                        const double dtx = tx - txj, dty = ty - tyj, dgx = x - s_e[GE_X][e], dgy = y - s_e[GE_Y][e];
                        const double den = dtx * dtx + dty * dty;
                        if (den > 0.0) {
                            gdef = 1;
                            gain = (dgx * dtx + dgy * dty) / den;
                            err = sqrt((x - tx) * (x - tx) + (y - ty) * (y - ty));
                        }
                    }
                }
            }
            s_has[lane] = has;
            s_gdef[lane] = gdef;
            s_cand[lane] = cand;
            s_j[lane] = j;
            s_w[lane] = w;
            s_s[lane] = s;
            s_gain[lane] = gain;
            s_err[lane] = err;
        }
        __syncthreads();
        // ---- phase 3
        if (lane == 0) {
            int nc = 0;
            for (int t = 0; t < m; ++t) {
                const int kind = s_kind[t], slot = GP_RING + t;
                int cls = 0, id = -1;
                double ms = 0.0;
                bool closes = false;
                if (kind == GK_NONE) {
                    if (st[GP_OPEN] != 0.0) st[GP_MISSING] = st[GP_MISSING] + 1.0;
                } else if (kind == GK_RESTART) {
                    gp_abort(st, s_tab);
                    st[GP_HAS_END] = 0.0;
                } else if (kind == GK_SACCADE) {
                    cls = 2;
                    closes = st[GP_OPEN] != 0.0;
                } else if (kind == GK_SETTLE) {
                    cls = 1;
                } else if (kind == GK_RUN) {
                    cls = 1;
                    if (s_cand[t] != 0) {
                        const double tt = s_e[GE_T][slot];
                        if (st[GP_OPEN] == 0.0) {
                            int k = s_j[t];
                            if (st[GP_HAS_END] != 0.0) {               // episodes never overlap: the onset lies after the last closed one's end
                                while (k < s_idx[t] && !(s_e[GE_T][s_tl[k]] > st[GP_T_END])) ++k;
                            }
                            const int o = s_tl[k];
                            st[GP_OPEN] = 1.0;
                            st[GP_ID] = st[GP_NEXT_ID];
                            st[GP_NEXT_ID] = st[GP_NEXT_ID] + 1.0;
                            st[GP_T_ONSET] = s_e[GE_T][o];
                            st[GP_OV0] = s_e[GE_V0][o];
                            st[GP_OV1] = s_e[GE_V1][o];
                            st[GP_OV2] = s_e[GE_V2][o];
                            st[GP_X0] = s_e[GE_X][o];
                            st[GP_Y0] = s_e[GE_Y][o];
                            st[GP_CUM_ONSET] = s_e[GE_CUM][o];
                            st[GP_N] = 0.0;
                            st[GP_PEAK] = 0.0;
                            st[GP_MISSING] = 0.0;
                            st[GP_GAIN_SUM] = 0.0;
                            st[GP_GAIN_N] = 0.0;
                            st[GP_ERR_SUM] = 0.0;
                            st[GP_FIX] = (double)s_fix[t];
                        }
                        st[GP_N] = st[GP_N] + 1.0;
                        if (s_w[t] > st[GP_PEAK]) st[GP_PEAK] = s_w[t];
                        st[GP_T_LAST] = tt;
                        st[GP_LV0] = s_e[GE_V0][slot];
                        st[GP_LV1] = s_e[GE_V1][slot];
                        st[GP_LV2] = s_e[GE_V2][slot];
                        st[GP_X1] = s_e[GE_X][slot];
                        st[GP_Y1] = s_e[GE_Y][slot];
                        st[GP_CUM_LAST] = s_e[GE_CUM][slot];
                        if (s_gdef[t] != 0) {
                            st[GP_GAIN_SUM] = st[GP_GAIN_SUM] + s_gain[t];
                            st[GP_ERR_SUM] = st[GP_ERR_SUM] + s_err[t];
                            st[GP_GAIN_N] = st[GP_GAIN_N] + 1.0;
                        }
                        cls = 3;
                        id = (int)st[GP_ID];
                        ms = 1000.0 * (tt - st[GP_T_ONSET]);
                    } else {
                        closes = st[GP_OPEN] != 0.0;
                    }
                }
                if (closes && nc < GP_MAX_CLOSINGS) {                  // the episode ends at its last sample
                    st[GP_OPEN] = 0.0;
                    st[GP_HAS_END] = 1.0;
                    st[GP_T_END] = st[GP_T_LAST];
                    s_c[GC_ID][nc] = st[GP_ID];
                    s_c[GC_T0][nc] = st[GP_T_ONSET];
                    s_c[GC_T1][nc] = st[GP_T_LAST];
                    s_c[GC_N][nc] = st[GP_N];
                    s_c[GC_X0][nc] = st[GP_X0];
                    s_c[GC_Y0][nc] = st[GP_Y0];
                    s_c[GC_X1][nc] = st[GP_X1];
                    s_c[GC_Y1][nc] = st[GP_Y1];
                    s_c[GC_PEAK][nc] = st[GP_PEAK];
                    s_c[GC_PATH][nc] = st[GP_CUM_LAST] - st[GP_CUM_ONSET];
                    s_c[GC_FIX][nc] = st[GP_FIX];
                    s_c[GC_MISSING][nc] = st[GP_MISSING];
                    s_c[GC_GAIN_N][nc] = st[GP_GAIN_N];
                    s_c[GC_GAIN_SUM][nc] = st[GP_GAIN_SUM];
                    s_c[GC_ERR_SUM][nc] = st[GP_ERR_SUM];
                    s_c[GC_OV0][nc] = st[GP_OV0];
                    s_c[GC_OV1][nc] = st[GP_OV1];
                    s_c[GC_OV2][nc] = st[GP_OV2];
                    s_c[GC_LV0][nc] = st[GP_LV0];
                    s_c[GC_LV1][nc] = st[GP_LV1];
                    s_c[GC_LV2][nc] = st[GP_LV2];
                    ++nc;
                }
                if (kind == GK_SACCADE) st[GP_HAS_END] = 0.0;          // (the run is emptied: nothing of it can overlap a later one)
                s_cls[t] = cls;
                s_id[t] = id;
                s_ms[t] = ms;
            }
            s_nc = nc;
        }
        __syncthreads();
        // ---- phase 4
        const int nc = s_nc;                                           // (the same in every lane)
        if (lane < nc) {
            s_c[GC_AMP][lane] = gp_angle(s_c[GC_OV0][lane], s_c[GC_OV1][lane], s_c[GC_OV2][lane], s_c[GC_LV0][lane], s_c[GC_LV1][lane],
                                         s_c[GC_LV2][lane]);
            s_c[GC_DIR][lane] = atan2(s_c[GC_Y1][lane] - s_c[GC_Y0][lane], s_c[GC_X1][lane] - s_c[GC_X0][lane]) * 57.29577951308232;
        }
        __syncthreads();
        // ---- phase 5
        if (lane == 0) {
            for (int j = 0; j < nc; ++j) {
                const double amp = s_c[GC_AMP][j], dur = s_c[GC_T1][j] - s_c[GC_T0][j], peak = s_c[GC_PEAK][j], missing = s_c[GC_MISSING][j];
                if (missing > (double)P.max_missing) s_tab[GP_INTERRUPTED] = s_tab[GP_INTERRUPTED] + 1.0;
                else if (dur < P.min_dur) s_tab[GP_SHORT] = s_tab[GP_SHORT] + 1.0;
                else if (!(amp >= P.min_amp)) s_tab[GP_SMALL] = s_tab[GP_SMALL] + 1.0;
                else {
                    const double mean_v = amp / dur, gain_n = s_c[GC_GAIN_N][j];
                    s_tab[GP_ACCEPTED] = s_tab[GP_ACCEPTED] + 1.0;
                    s_tab[GP_SUM_DUR] = s_tab[GP_SUM_DUR] + dur;
                    s_tab[GP_SUM_AMP] = s_tab[GP_SUM_AMP] + amp;
                    s_tab[GP_SUM_PATH] = s_tab[GP_SUM_PATH] + s_c[GC_PATH][j];
                    s_tab[GP_SUM_MEAN_V] = s_tab[GP_SUM_MEAN_V] + mean_v;
                    if (peak > s_tab[GP_MAX_PEAK]) s_tab[GP_MAX_PEAK] = peak;
                    s_tab[GP_SUM_GAIN] = s_tab[GP_SUM_GAIN] + s_c[GC_GAIN_SUM][j];
                    s_tab[GP_TAB_GAIN_N] = s_tab[GP_TAB_GAIN_N] + gain_n;
                    const int cnt = s_cd[0];
                    if (cnt >= S) {
                        s_cd[1] = s_cd[1] + 1;
                    } else {
                        double* dst = rows + (size_t)cnt * GP_ROW;
                        dst[0] = s_c[GC_ID][j];
                        dst[1] = s_c[GC_T0][j];
                        dst[2] = s_c[GC_T1][j];
                        dst[3] = s_c[GC_N][j];
                        dst[4] = s_c[GC_X0][j];
                        dst[5] = s_c[GC_Y0][j];
                        dst[6] = s_c[GC_X1][j];
                        dst[7] = s_c[GC_Y1][j];
                        dst[8] = amp;
                        dst[9] = s_c[GC_DIR][j];
                        dst[10] = mean_v;
                        dst[11] = peak;
                        dst[12] = s_c[GC_PATH][j];
                        dst[13] = s_c[GC_FIX][j];
                        dst[14] = missing;
                        dst[15] = gain_n;
                        dst[16] = gain_n > 0.0 ? s_c[GC_GAIN_SUM][j] / gain_n : __builtin_nan("");
                        dst[17] = gain_n > 0.0 ? s_c[GC_ERR_SUM][j] / gain_n : __builtin_nan("");
                        dst[18] = 0.0;
                        dst[19] = 0.0;
                        s_cd[0] = cnt + 1;
                    }
                }
            }
        }
        // ---- phase 6 (what it reads was written in phases 2 and 3, at least one barrier ago; phase 5 touches none of it)
        if (f < T) {
            const float none = __builtin_nanf("");
            gaze_class[n] = (uint8_t)s_cls[lane];
            pursuit_id[n] = s_id[lane];
            pursuit_ms[n] = (float)s_ms[lane];
            windowed[n] = s_has[lane] ? (float)s_w[lane] : none;
            straightness[n] = s_has[lane] ? (float)s_s[lane] : none;
            pursuit_gain[n] = s_gdef[lane] ? (float)s_gain[lane] : none;
        }
        // the run's last <= 32 timeline entries become slots 0 .. 31 (s_ntl and s_rf: phase 1's, the same in every lane)
        const int ntl = s_ntl, keep = min(GP_RING, ntl - s_rf);
        double mv[GP_ENTRY];
        if (lane < keep) {
            const int src = s_tl[ntl - keep + lane];
#pragma unroll
            for (int c = 0; c < GP_ENTRY; ++c) mv[c] = s_e[c][src];
        }
        __syncthreads();
        if (lane < keep) {
#pragma unroll
            for (int c = 0; c < GP_ENTRY; ++c) s_e[c][lane] = mv[c];
        }
        for (int i = lane; i < GP_SLOTS; i += GP_WAVE) s_tl[i] = i;
        if (lane == 0) {
            s_ntl = keep;
            s_rf = 0;
        }
        __syncthreads();
    }
    if (lane == 0) {
        count[b] = s_cd[0];
        dropped[b] = s_cd[1];
        st[GP_RING_N] = (double)s_ntl;
    }
    __syncthreads();
    const int kept = s_ntl;
    if (lane < GP_SCALARS) row[lane] = st[lane];
    if (lane < GP_TABLE) tab[lane] = s_tab[lane];
    for (int i = lane; i < GP_RING * GP_ENTRY; i += GP_WAVE) row[GP_SCALARS + i] = i / GP_ENTRY < kept ? s_e[i % GP_ENTRY][i / GP_ENTRY] : 0.0;
}

__host__ bool gp_host_finite(const double x) { return x >= -1.79769313486231570815e308 && x <= 1.79769313486231570815e308; }      // false for a NaN

}  // namespace
}  // namespace eve

using namespace eve;

extern "C" int eve_gaze_pursuits(long long B, int T, const uint8_t* sample, const double* sample_time, const double* gaze_vector,
                                 const float* point, const uint8_t* event, const float* velocity, const int* fixation_id, const float* target,
                                 const int* lengths, const int* reset, double window_s, double min_window_s, double pursuit_deg_s,
                                 double min_straightness, double settle_s, double min_duration_s, double min_amplitude_deg, int max_missing,
                                 double* state, double* table, int S, double* store, int* count, int* dropped, uint8_t* gaze_class,
                                 int* pursuit_id, float* pursuit_ms, float* gaze_velocity_windowed, float* gaze_straightness,
                                 float* pursuit_gain, eve_stream_t stream) {
    const char* why = nullptr;
    const long long LIM = 0x7fffffff;
    if (!state || !table || !store || !count || !dropped) why = "a null carried buffer";
    else if (B < 1 || T < 0 || S <= 0) why = "B >= 1, T >= 0 and a store capacity S >= 1";
    else if (T > 0 && (!sample || !sample_time || !gaze_vector || !point || !event || !velocity || !fixation_id || !gaze_class || !pursuit_id ||
                       !pursuit_ms || !gaze_velocity_windowed || !gaze_straightness || !pursuit_gain))
        why = "a null frame input or output with T > 0";
    else if (B > LIM / GP_STATE) why = "B * 320 must fit 31 bits";
    else if (B > LIM / GP_ROW / S) why = "B * S * 20 must fit 31 bits";
    else if (T > 0 && B > LIM / 3 / T) why = "B * T * 3 must fit 31 bits";
    else if (!gp_host_finite(window_s) || !gp_host_finite(min_window_s) || !gp_host_finite(pursuit_deg_s) || !gp_host_finite(min_straightness) ||
             !gp_host_finite(settle_s) || !gp_host_finite(min_duration_s) || !gp_host_finite(min_amplitude_deg))
        why = "the parameters must be finite";
    else if (window_s <= 0.0) why = "window_s must be > 0";
    else if (min_window_s <= 0.0 || min_window_s > window_s) why = "min_window_s must be > 0 and <= window_s";
    else if (pursuit_deg_s <= 0.0) why = "pursuit_deg_s must be > 0";
    else if (min_straightness <= 0.0 || min_straightness > 1.0) why = "min_straightness must lie in (0, 1]";
    else if (settle_s < 0.0) why = "settle_s must be >= 0";
    else if (min_duration_s < 0.0) why = "min_duration_s must be >= 0";
    else if (min_amplitude_deg < 0.0) why = "min_amplitude_deg must be >= 0";
    else if (max_missing < 0) why = "max_missing must be >= 0";
    if (why) {
        char msg[160];
        snprintf(msg, sizeof(msg), "gaze_pursuits: %s", why);
        return set_error_msg(msg);
    }
    GpParams P;
    P.window = window_s;
    P.min_window = min_window_s;
    P.pursuit = pursuit_deg_s;
    P.straight = min_straightness;
    P.settle = settle_s;
    P.min_dur = min_duration_s;
    P.min_amp = min_amplitude_deg;
    P.max_missing = max_missing;
    EVE_LAUNCH("gaze_pursuits_kernel", gaze_pursuits_kernel, dim3((unsigned)B), dim3(GP_WAVE), 0, (hipStream_t)stream, T, sample, sample_time,
               gaze_vector, point, event, velocity, fixation_id, target, lengths, reset, P, state, table, S, store, count, dropped, gaze_class,
               pursuit_id, pursuit_ms, gaze_velocity_windowed, gaze_straightness, pursuit_gain);
    EVE_CHECK_LAUNCH();
    return 0;
}
