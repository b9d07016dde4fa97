// Areas of interest, on the device: which region of the screen the point of gaze is in, for how long, how often and in which order.
// Per stream every frame's point is tested against up to 64 shapes (rectangle, ellipse, polygon of up to 16 vertices), the lowest
// containing index is the frame's AOI, and a state machine turns the sequence into visits, a dwell table and a transition matrix.
// The contract -- operation order and the state row included -- is in include/eve_hip.h (eve_gaze_aoi) and in numpy in
// tests/aoi_ref.py.
//
// One wavefront (a 64-thread workgroup) per stream; the table, the transition rows and (where they do not move) the shapes live in
// LDS for the launch.  The frames go by in passes of 64, each pass in phases:
//   0  parallel   lane t reads frame t's point, time and flags, and tests what does not depend on history
//   1  parallel   the hit tests: with G = 64 / A, lane l holds the pair (frame tl = l / A of a group of G frames, AOI a = l % A), so the
//                 wave tests G frames at once; one ballot per group, and the frame's mask is its A bits of the ballot.  A = 64: an AOI
//                 per lane, a ballot per frame; A = 1: 64 frames in one go
//   2  serial     lane 0 walks the pass: the time-order test, the gap rule, visits, the table, the transitions, the store
//   3  parallel   lane t writes frame t's three outputs
// Float64 throughout, + - * / and comparisons only, every operation rounded on its own: the bits do not depend on this structure.
// Every branch around a barrier or a ballot is uniform over the wave.
#include "common.h"

#pragma clang fp contract(off)

namespace eve {
namespace {

constexpr int GA_WAVE = 64;
constexpr int GA_STATE = 16;             // doubles per state row (include/eve_hip.h has the layout)
constexpr int GA_ROW = 8;                // doubles per table row and per stored visit
constexpr int GA_SHAPE = 36;             // floats per AOI
constexpr int GA_MAX = 64;               // AOIs
enum { GA_TICKS = 0, GA_HAS_PREV, GA_T_PREV, GA_PREV_AOI, GA_OPEN, GA_V_AOI, GA_T_ENTER, GA_T_LAST, GA_V_SAMPLES, GA_V_FIXATIONS, GA_V_INDEX,
       GA_NEXT_INDEX, GA_LAST_AOI, GA_FIX_ID, GA_FIX_AOI };
enum { GA_DWELL = 0, GA_SAMPLES, GA_VISITS, GA_T_FIRST_ENTRY, GA_TAB_T_LAST, GA_FIXATIONS, GA_T_FIRST_FIXATION };

__device__ __forceinline__ bool ga_finite(const double x) { return fabs(x) <= 1.79769313486231570815e308; }      // false for a NaN

// Does the AOI row r (36 floats, in LDS or in global memory) contain (x, y)?
__device__ __forceinline__ bool ga_contains(const float* __restrict__ r, const double x, const double y) {
#pragma clang fp contract(off)
    const float kind = r[0];
    if (kind == 1.0f || kind == 2.0f) {
        const double c0 = (double)r[4], c1 = (double)r[5], c2 = (double)r[6], c3 = (double)r[7];
        if (!(ga_finite(c0) && ga_finite(c1) && ga_finite(c2) && ga_finite(c3))) return false;
        if (kind == 1.0f) return c0 <= x && x < c2 && c1 <= y && y < c3;
        if (!(c2 > 0.0 && c3 > 0.0)) return false;
        const double u = (x - c0) / c2, v = (y - c1) / c3;
        return u * u + v * v <= 1.0;
    }
    if (kind != 3.0f) return false;
    const float nf = r[1];
    if (!(nf >= 3.0f && nf <= 16.0f)) return false;
    const int n = (int)nf;
    if ((float)n != nf) return false;
    double xj = (double)r[4 + 2 * (n - 1)], yj = (double)r[5 + 2 * (n - 1)];      // edge (i, j): j = n - 1 for i = 0, else i - 1
    bool finite = true, inside = false;
    for (int i = 0; i < n; ++i) {
        const double xi = (double)r[4 + 2 * i], yi = (double)r[5 + 2 * i];
        finite = finite && ga_finite(xi) && ga_finite(yi);
        if ((yi > y) != (yj > y)) {
            if (x < (xj - xi) * (y - yi) / (yj - yi) + xi) inside = !inside;
        }
        xj = xi;
        yj = yi;
    }
    return finite && inside;
}

// Closes the open visit of the state row st (lane 0 only): a row into the store, or a drop where it is full.
// cd (in LDS, so that nothing lives in scratch): the stream's count and dropped.
__device__ __forceinline__ void ga_close(double* st, double* __restrict__ rows, const int V, int* cd) {
    if (st[GA_OPEN] == 0.0) return;
    st[GA_OPEN] = 0.0;
    st[GA_LAST_AOI] = st[GA_V_AOI];
    const int cnt = cd[0];
    if (cnt >= V) {
        cd[1] = cd[1] + 1;
        return;
    }
    double* dst = rows + (size_t)cnt * GA_ROW;
    dst[0] = st[GA_V_AOI] - 1.0;
    dst[1] = st[GA_T_ENTER];
    dst[2] = st[GA_T_LAST];
    dst[3] = st[GA_V_SAMPLES];
    dst[4] = st[GA_V_FIXATIONS];
    dst[5] = st[GA_V_INDEX];
    dst[6] = 0.0;
    dst[7] = 0.0;
    cd[0] = cnt + 1;
}

__global__ __launch_bounds__(GA_WAVE) void gaze_aoi_kernel(const int T, const int A, const float* __restrict__ pog, const float* __restrict__ shapes,
                                                           const int per_frame, const double* __restrict__ frame_time,
                                                           const uint8_t* __restrict__ valid, const uint8_t* __restrict__ valid_key,
                                                           const int* __restrict__ fixation_id, const uint8_t* __restrict__ fixating,
                                                           const int* __restrict__ lengths, const int* __restrict__ reset,
                                                           const int* __restrict__ flush, const double fps, const double max_gap,
                                                           double* __restrict__ state, double* __restrict__ table, int* __restrict__ trans,
                                                           const int V, double* __restrict__ visits, int* __restrict__ count,
                                                           int* __restrict__ dropped, int* __restrict__ out_id,
                                                           long long* __restrict__ out_mask, float* __restrict__ out_ms) {
#pragma clang fp contract(off)
    __shared__ double st[GA_STATE];
    __shared__ double s_tab[(GA_MAX + 1) * GA_ROW];
    __shared__ int s_trans[(GA_MAX + 1) * GA_MAX];
    __shared__ float s_shapes[GA_MAX * GA_SHAPE];
    __shared__ double s_x[GA_WAVE], s_y[GA_WAVE], s_tt[GA_WAVE], s_ms[GA_WAVE];
    __shared__ unsigned long long s_mask[GA_WAVE];
    __shared__ int s_flag[GA_WAVE], s_id[GA_WAVE], s_fix[GA_WAVE];       // fix: the frame's fixation id where it counts, else -1
    __shared__ int s_cd[2];                                            // the stream's count and dropped (lane 0's)
    const int lane = threadIdx.x;
    const long long b = blockIdx.x;
    double* row = state + (size_t)b * GA_STATE;
    double* tab = table + (size_t)b * (A + 1) * GA_ROW;
    int* tr = trans + (size_t)b * (A + 1) * A;
    double* rows = visits + (size_t)b * V * GA_ROW;
    if (lane < GA_STATE) st[lane] = row[lane];
    for (int i = lane; i < (A + 1) * GA_ROW; i += GA_WAVE) s_tab[i] = tab[i];
    for (int i = lane; i < (A + 1) * A; i += GA_WAVE) s_trans[i] = tr[i];
    if (T > 0 && !per_frame) {
        const float* src = shapes + (size_t)b * A * GA_SHAPE;
        for (int i = lane; i < A * GA_SHAPE; i += GA_WAVE) s_shapes[i] = src[i];
    }
    __syncthreads();
    if (lane == 0) {
        s_cd[0] = min(max(count[b], 0), V);
        s_cd[1] = dropped[b];
        if (reset && reset[b] != 0) {
            ga_close(st, rows, V, s_cd);
            const double keep = st[GA_NEXT_INDEX];
            for (int i = 0; i < GA_STATE; ++i) st[i] = 0.0;
            st[GA_NEXT_INDEX] = keep;
        }
    }
    __syncthreads();
    int len = T;
    if (lengths) len = min(max(lengths[b], 0), T);
    const double ticks0 = st[GA_TICKS];
    const int G = GA_WAVE / A;                                         // frames tested at once
    const int tl = lane / A, al = lane - tl * A;                       // this lane's frame within a group, and its AOI
    const unsigned long long amask = A == 64 ? ~0ull : (1ull << A) - 1ull;
    for (int base = 0; base < T; base += GA_WAVE) {                    // (T, base, len: the same in every lane)
        const int f = base + lane;
        const long long n = b * T + f;
        // ---- phase 0
        bool ok = false;
        int fix = -1;
        if (f < len) {
            const double tt = frame_time ? frame_time[n] : (ticks0 + (double)f) / fps;
            const double x = (double)pog[n * 2], y = (double)pog[n * 2 + 1];
            ok = (!valid || valid[n] != 0) && (!valid_key || valid_key[n] != 0) && ga_finite(x) && ga_finite(y) && ga_finite(tt);
            if (fixation_id && fixating[n] != 0 && fixation_id[n] >= 0) fix = fixation_id[n];
            s_x[lane] = x;
            s_y[lane] = y;
            s_tt[lane] = tt;
        }
        s_flag[lane] = ok ? 1 : 0;
        s_fix[lane] = fix;
        __syncthreads();
        // ---- phase 1
        const int m = min(GA_WAVE, len - base);                        // the pass's delivered frames (<= 0: none)
        for (int g = 0; g < m; g += G) {
            const int t = g + tl;
            bool hit = false;
            if (tl < G && t < m && s_flag[t] != 0) {
                const float* r = per_frame ? shapes + ((size_t)(b * T + base + t) * A + al) * GA_SHAPE : s_shapes + al * GA_SHAPE;
                hit = ga_contains(r, s_x[t], s_y[t]);
            }
            const unsigned long long hits = __ballot(hit);
            if (tl < G && t < m && al == 0) s_mask[t] = (hits >> (tl * A)) & amask;
        }
        __syncthreads();
        // ---- phase 2
        if (lane == 0) {
            const int mt = min(GA_WAVE, T - base);
            for (int t = 0; t < mt; ++t) {
                int id = -2;
                double ms = 0.0;
                unsigned long long mk = 0ull;
                const bool sample = t < m && s_flag[t] != 0 && (st[GA_HAS_PREV] == 0.0 || s_tt[t] > st[GA_T_PREV]);
                if (sample) {
                    const double tt = s_tt[t];
                    const double dt = tt - st[GA_T_PREV];
                    const bool restart = st[GA_HAS_PREV] == 0.0 || dt > max_gap;
                    mk = s_mask[t];
                    const int a = mk == 0ull ? -1 : __ffsll((long long)mk) - 1;
                    const double a1 = (double)(a + 1);
                    if (restart) ga_close(st, rows, V, s_cd);
                    else if (st[GA_OPEN] != 0.0 && a1 != st[GA_V_AOI]) ga_close(st, rows, V, s_cd);
                    if (a >= 0) {
                        double* ta = s_tab + a * GA_ROW;
                        if (st[GA_OPEN] == 0.0) {
                            st[GA_OPEN] = 1.0;
                            st[GA_V_AOI] = a1;
                            st[GA_T_ENTER] = tt;
                            st[GA_V_SAMPLES] = 0.0;
                            st[GA_V_FIXATIONS] = 0.0;
                            st[GA_V_INDEX] = st[GA_NEXT_INDEX];
                            st[GA_NEXT_INDEX] = st[GA_NEXT_INDEX] + 1.0;
                            if (ta[GA_VISITS] == 0.0) ta[GA_T_FIRST_ENTRY] = tt;
                            ta[GA_VISITS] = ta[GA_VISITS] + 1.0;
                            const double last = st[GA_LAST_AOI];            // (a row loaded by the caller may hold anything)
                            const int from = last >= 1.0 && last <= (double)A ? (int)last - 1 : A;
                            s_trans[from * A + a] += 1;
                        } else {
                            ta[GA_DWELL] = ta[GA_DWELL] + dt;
                        }
                        st[GA_V_SAMPLES] = st[GA_V_SAMPLES] + 1.0;
                        st[GA_T_LAST] = tt;
                        ta[GA_SAMPLES] = ta[GA_SAMPLES] + 1.0;
                        ta[GA_TAB_T_LAST] = tt;
                        ms = 1000.0 * (tt - st[GA_T_ENTER]);
                        const int fx = s_fix[t];
                        if (fx >= 0 && ((double)fx + 1.0 != st[GA_FIX_ID] || a1 != st[GA_FIX_AOI])) {
                            if (ta[GA_FIXATIONS] == 0.0) ta[GA_T_FIRST_FIXATION] = tt;
                            ta[GA_FIXATIONS] = ta[GA_FIXATIONS] + 1.0;
                            st[GA_V_FIXATIONS] = st[GA_V_FIXATIONS] + 1.0;
                            st[GA_FIX_ID] = (double)fx + 1.0;
                            st[GA_FIX_AOI] = a1;
                        }
                    } else {
                        double* ta = s_tab + A * GA_ROW;
                        ta[GA_SAMPLES] = ta[GA_SAMPLES] + 1.0;
                        if (!restart && st[GA_PREV_AOI] == 0.0) ta[GA_DWELL] = ta[GA_DWELL] + dt;
                    }
                    st[GA_HAS_PREV] = 1.0;
                    st[GA_T_PREV] = tt;
                    st[GA_PREV_AOI] = a1;
                    id = a;
                }
                s_id[t] = id;
                s_ms[t] = ms;
                s_mask[t] = mk;
            }
        }
        __syncthreads();
        // ---- phase 3
        if (f < T) {
            out_id[n] = s_id[lane];
            out_mask[n] = (long long)s_mask[lane];
            out_ms[n] = (float)s_ms[lane];
        }
        __syncthreads();
    }
    if (lane == 0) {
        st[GA_TICKS] = ticks0 + (double)len;
        if (flush && flush[b] != 0) ga_close(st, rows, V, s_cd);
        count[b] = s_cd[0];
        dropped[b] = s_cd[1];
    }
    __syncthreads();
    if (lane < GA_STATE) row[lane] = st[lane];
    for (int i = lane; i < (A + 1) * GA_ROW; i += GA_WAVE) tab[i] = s_tab[i];
    for (int i = lane; i < (A + 1) * A; i += GA_WAVE) tr[i] = s_trans[i];
}

__host__ bool ga_positive(const double x) { return x > 0.0 && x <= 1.79769313486231570815e308; }

}  // namespace
}  // namespace eve

using namespace eve;

extern "C" int eve_gaze_aoi(long long B, int T, int A, const float* pog, const float* shapes, int shapes_per_frame, const double* frame_time,
                            const uint8_t* valid, const uint8_t* valid_key, const int* fixation_id, const uint8_t* fixating, const int* lengths,
                            const int* reset, const int* flush, double fps, double max_gap_s, double* state, double* table, int* trans,
                            int visit_capacity, double* visits, int* count, int* dropped, int* id, long long* mask, float* visit_ms,
                            eve_stream_t stream) {
    const char* why = nullptr;
    const long long LIM = 0x7fffffff;
    if (!state || !table || !trans || !visits || !count || !dropped) why = "a null carried buffer";
    else if (B < 1 || T < 0 || A < 1 || A > GA_MAX || visit_capacity < 1) why = "B >= 1, T >= 0, A in 1 .. 64 and visit_capacity >= 1";
    else if (T > 0 && (!pog || !shapes || !id || !mask || !visit_ms)) why = "a null frame input or output with T > 0";
    else if ((fixation_id == nullptr) != (fixating == nullptr)) why = "fixation_id and fixating come together";
    else if (B > LIM / ((long long)(A + 1) * GA_ROW) || B > LIM / ((long long)(A + 1) * A) || B > LIM / ((long long)A * GA_SHAPE))
        why = "B * (A + 1) * 8, B * (A + 1) * A and B * A * 36 must fit 31 bits";
    else if (B > LIM / GA_ROW / visit_capacity) why = "B * visit_capacity * 8 must fit 31 bits";
    else if (T > 0 && B > LIM / 2 / T) why = "B * T * 2 must fit 31 bits";
    else if (T > 0 && shapes_per_frame && B * T > LIM / ((long long)A * GA_SHAPE)) why = "B * T * A * 36 must fit 31 bits";
    else if (!ga_positive(max_gap_s)) why = "max_gap_s must be a finite number > 0";
    else if (T > 0 && !frame_time && !ga_positive(fps)) why = "without frame_time, fps must be a finite number > 0";
    if (why) {
        char msg[160];
        snprintf(msg, sizeof(msg), "gaze_aoi: %s", why);
        return set_error_msg(msg);
    }
    EVE_LAUNCH("gaze_aoi_kernel", gaze_aoi_kernel, dim3((unsigned)B), dim3(GA_WAVE), 0, (hipStream_t)stream, T, A, pog, shapes,
               shapes_per_frame ? 1 : 0, frame_time, valid, valid_key, fixation_id, fixating, lengths, reset, flush, frame_time ? 1.0 : fps,
               max_gap_s, state, table, trans, visit_capacity, visits, count, dropped, id, mask, visit_ms);
    EVE_CHECK_LAUNCH();
    return 0;
}
