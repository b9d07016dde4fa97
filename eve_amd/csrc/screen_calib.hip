// Screen-space gaze calibration, on the device: the residual that depends on the position on the screen -- what is left after the
// per-person offset kappa (calibration.hip) -- removed by a low-order map of the pipeline's OUTPUT point, fitted to the dots of a five-
// or nine-point procedure.  With (x, y) the output point in pixels, u = (x + x) / W - 1, v = (y + y) / H - 1 and phi = (1, u, v, u*u,
// u*v, v*v) cut to K terms (1 offset, 3 affine, 6 quadratic) the correction in millimetres is s_a = sum_k phi_k C[a][k].  Three
// stages; the contract -- operation order included -- is in include/eve_hip.h (eve_screen_calib_append, eve_screen_calib_fit,
// eve_screen_calib_apply) and in numpy in tests/screen_calib_ref.py.
//
//   eve_screen_calib_append  one THREAD per stream, which walks the chunk's frames in time order: every usable frame is reduced to 12
//                            doubles and appended to the stream's store.  No atomics: eve_calib_append's scheme without the eye axis.
//   eve_screen_calib_fit     one wavefront per stream: weighted linear least squares by Cholesky, re-weighted under a Huber loss until
//                            no coefficient moves, then a final pass that takes the accuracy report.  Lane l adds the contributions of
//                            rows l, l + 64, ... in order, the partial sums go through LDS, lane j adds column j over the lanes in
//                            order, every lane reads the sums back: from there on all 64 lanes hold the same bits, so every branch
//                            is wave-uniform.  Mode 1 evaluates the stored map and solves nothing.
//   eve_screen_calib_apply   one thread per frame.
// Float64 throughout, every operation rounded on its own.
#include "common.h"

#pragma clang fp contract(off)

namespace eve {
namespace {

constexpr int SC_WAVE = 64;
constexpr int SC_ROW = 12;               // u, v, xm, ym, tmx, tmy, e0, e1, e2, the weight, two reserved 0.0
constexpr int SC_KMAX = 6;
constexpr int SC_TRI = SC_KMAX * (SC_KMAX + 1) / 2;
constexpr int SC_NC = SC_TRI + 2 * SC_KMAX + 5;      // G's lower triangle (21), bx (6), by (6), cost, w*r2, w*r, inl, 1
constexpr int SC_NF = 8;                 // the final pass: w*r2, w*r, inl, 1, w*deg, and w*r2, w*r, w*deg at C = 0
constexpr int SC_NM = 3;                 // its maxima: r, r at C = 0, the length of the correction
constexpr int SC_MAX_SOLVES = 64;
constexpr double SC_RAD2DEG = 57.29577951308232;     // 180 / pi

__device__ __forceinline__ bool sc_finite(const double x) { return fabs(x) <= 1.79769313486231570815e308; }      // false for a NaN

__host__ __device__ __forceinline__ int sc_terms(const int kind) { return kind == 1 ? 1 : kind == 2 ? 3 : kind == 3 ? 6 : 0; }

__device__ __forceinline__ void sc_phi(const double u, const double v, double (&phi)[SC_KMAX]) {
#pragma clang fp contract(off)
    phi[0] = 1.0;
    phi[1] = u;
    phi[2] = v;
    phi[3] = u * u;
    phi[4] = u * v;
    phi[5] = v * v;
}

// s = C[0]; s = s + phi_k * C[k], k = 1 .. K-1 (K = 0: 0.0)
__device__ __forceinline__ double sc_shift(const double (&phi)[SC_KMAX], const double* c, const int K) {
#pragma clang fp contract(off)
    double s = 0.0;
    if (K > 0) s = s + c[0];
#pragma unroll
    for (int k = 1; k < SC_KMAX; ++k)
        if (k < K) s = s + phi[k] * c[k];
    return s;
}

// One frame -> its row; false where the frame is not usable.
__device__ __forceinline__ bool sc_reduce(const float* __restrict__ pog, const float* __restrict__ origin, const float* __restrict__ T,
                                          const float* __restrict__ ppm, const float* __restrict__ target, const double W, const double H,
                                          double (&row)[SC_ROW]) {
#pragma clang fp contract(off)
    const double x = (double)pog[0], y = (double)pog[1], sx = (double)ppm[0], sy = (double)ppm[1], tx = (double)target[0], ty = (double)target[1];
    bool fin = sc_finite(x) && sc_finite(y) && sc_finite(sx) && sc_finite(sy) && sc_finite(tx) && sc_finite(ty);
    double Tm[16], o[3];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        Tm[i] = (double)T[i];
        fin = fin && sc_finite(Tm[i]);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        o[i] = (double)origin[i];
        fin = fin && sc_finite(o[i]);
    }
    if (!fin) return false;
    row[0] = (x + x) / W - 1.0;
    row[1] = (y + y) / H - 1.0;
    row[2] = x / sx;
    row[3] = y / sy;
    row[4] = tx / sx;
    row[5] = ty / sy;
#pragma unroll
    for (int i = 0; i < 3; ++i) row[6 + i] = ((Tm[i * 4] * o[0] + Tm[i * 4 + 1] * o[1]) + Tm[i * 4 + 2] * o[2]) + Tm[i * 4 + 3];
    row[9] = 1.0;
    row[10] = 0.0;
    row[11] = 0.0;
    bool ok = sx > 0.0 && sy > 0.0 && row[8] != 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) ok = ok && sc_finite(row[i]);
    return ok;
}

__global__ __launch_bounds__(SC_WAVE) void screen_calib_append_kernel(const long long B, const int T, const float* __restrict__ pog,
                                                                      const float* __restrict__ origin, const float* __restrict__ inv_cam,
                                                                      const float* __restrict__ ppm, const float* __restrict__ target,
                                                                      const uint8_t* __restrict__ valid, const int* __restrict__ lengths,
                                                                      const uint8_t* __restrict__ frame_valid, const double W, const double H,
                                                                      const int C, double* __restrict__ samples, int* __restrict__ count,
                                                                      int* __restrict__ dropped) {
#pragma clang fp contract(off)
    const long long b = (long long)blockIdx.x * SC_WAVE + threadIdx.x;      // the stream
    if (b >= B) return;
    int len = T;
    if (lengths) len = min(max(lengths[b], 0), T);
    int cnt = min(max(count[b], 0), C), drop = dropped[b];
    for (int f = 0; f < len; ++f) {
        const long long n = b * T + f;
        if (valid && valid[n] == 0) continue;
        if (frame_valid && frame_valid[n] == 0) continue;
        double row[SC_ROW];
        if (!sc_reduce(pog + n * 2, origin + n * 3, inv_cam + n * 16, ppm + n * 2, target + n * 2, W, H, row)) continue;
        if (cnt >= C) {
            ++drop;
            continue;
        }
        double* dst = samples + ((size_t)b * C + cnt) * SC_ROW;
#pragma unroll
        for (int i = 0; i < SC_ROW; ++i) dst[i] = row[i];
        ++cnt;
    }
    count[b] = cnt;
    dropped[b] = drop;
}

// The column sums of the header's order: every lane's `NCOL` partial sums -> out[0 .. NCOL-1], the same bits in every lane.  Columns
// from `first_max` on are maxima (of values >= 0, from 0.0) in place of sums.
template <int NCOL>
__device__ __forceinline__ void sc_columns(const double (&acc)[NCOL], const int lane, const int first_max, double* c_lds, double* s_lds,
                                           double (&out)[NCOL]) {
#pragma clang fp contract(off)
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NCOL; ++j) c_lds[lane * NCOL + j] = acc[j];
    __syncthreads();
    if (lane < NCOL) {
        double s = 0.0;
        if (lane < first_max) {
            for (int l = 0; l < SC_WAVE; ++l) s = s + c_lds[l * NCOL + lane];
        } else {
            for (int l = 0; l < SC_WAVE; ++l) {
                const double m = c_lds[l * NCOL + lane];
                s = m > s ? m : s;
            }
        }
        s_lds[lane] = s;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NCOL; ++j) out[j] = s_lds[j];
}

// One pass of the contract at the coefficients c [2][6] -> the SC_NC sums (columns of terms >= K stay 0).
__device__ __forceinline__ void sc_pass(const double* __restrict__ rows, const int n, const int lane, const double (&c)[2 * SC_KMAX], const int K,
                                        const double huber, double* c_lds, double* s_lds, double (&S)[SC_NC]) {
#pragma clang fp contract(off)
    double acc[SC_NC];
#pragma unroll
    for (int j = 0; j < SC_NC; ++j) acc[j] = 0.0;
    for (int i = lane; i < n; i += SC_WAVE) {
        const double* r = rows + (size_t)i * SC_ROW;
        const double w = r[9];
        if (!(w > 0.0)) continue;
        double phi[SC_KMAX];
        sc_phi(r[0], r[1], phi);
        const double px = sc_shift(phi, c, K), py = sc_shift(phi, c + SC_KMAX, K);
        const double ex = r[4] - r[2], ey = r[5] - r[3];
        const double rx = px - ex, ry = py - ey;
        const double r2 = rx * rx + ry * ry, rr = sqrt(r2);
        double ws = w, cost = w * r2, inl = 1.0;
        if (huber > 0.0) {
            const bool inlier = !(rr > huber);
            ws = w * (inlier ? 1.0 : huber / rr);
            cost = w * (inlier ? r2 : huber * ((rr + rr) - huber));
            inl = inlier ? 1.0 : 0.0;
        }
#pragma unroll
        for (int a = 0; a < SC_KMAX; ++a) {
            if (a < K) {
                const double wp = ws * phi[a];
#pragma unroll
                for (int b = 0; b <= a; ++b)
                    if (b < K) acc[a * (a + 1) / 2 + b] = acc[a * (a + 1) / 2 + b] + wp * phi[b];
                acc[SC_TRI + a] = acc[SC_TRI + a] + wp * ex;
                acc[SC_TRI + SC_KMAX + a] = acc[SC_TRI + SC_KMAX + a] + wp * ey;
            }
        }
        acc[SC_NC - 5] = acc[SC_NC - 5] + cost;
        acc[SC_NC - 4] = acc[SC_NC - 4] + w * r2;
        acc[SC_NC - 3] = acc[SC_NC - 3] + w * rr;
        acc[SC_NC - 2] = acc[SC_NC - 2] + inl;
        acc[SC_NC - 1] = acc[SC_NC - 1] + 1.0;
    }
    sc_columns<SC_NC>(acc, lane, SC_NC, c_lds, s_lds, S);
}

// G c_a = b_a for both axes: Cholesky row by row, forward then backward substitution; false at a failed pivot.
__device__ __forceinline__ bool sc_solve(const double (&S)[SC_NC], const int K, double (&c)[2 * SC_KMAX]) {
#pragma clang fp contract(off)
    double L[SC_TRI];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < SC_KMAX; ++j) {
        if (j < K) {
            const double gjj = S[j * (j + 1) / 2 + j];
            double s = gjj;
#pragma unroll
            for (int k = 0; k < j; ++k) s = s - L[j * (j + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
            ok = ok && gjj > 0.0 && s > 1e-10 * gjj;
            const double ljj = sqrt(s);
            L[j * (j + 1) / 2 + j] = ljj;
#pragma unroll
            for (int i = j + 1; i < SC_KMAX; ++i) {
                if (i < K) {
                    double t = S[i * (i + 1) / 2 + j];
#pragma unroll
                    for (int k = 0; k < j; ++k) t = t - L[i * (i + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
                    L[i * (i + 1) / 2 + j] = t / ljj;
                }
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        double y[SC_KMAX];
#pragma unroll
        for (int i = 0; i < SC_KMAX; ++i) {
            y[i] = 0.0;
            if (i < K) {
                double t = S[SC_TRI + a * SC_KMAX + i];
#pragma unroll
                for (int k = 0; k < i; ++k) t = t - L[i * (i + 1) / 2 + k] * y[k];
                y[i] = t / L[i * (i + 1) / 2 + i];
            }
        }
#pragma unroll
        for (int i = SC_KMAX - 1; i >= 0; --i) {
            c[a * SC_KMAX + i] = 0.0;
            if (i < K) {
                double t = y[i];
#pragma unroll
                for (int k = i + 1; k < SC_KMAX; ++k)
                    if (k < K) t = t - L[k * (k + 1) / 2 + i] * c[a * SC_KMAX + k];
                c[a * SC_KMAX + i] = t / L[i * (i + 1) / 2 + i];
            }
        }
    }
    return ok;
}

// deg = atan2(|a x b|, a . b) * (180 / pi), a = (ax, ay, mz), b = (bx, by, mz)
__device__ __forceinline__ double sc_angle(const double ax, const double ay, const double bx, const double by, const double mz) {
#pragma clang fp contract(off)
    const double c0 = ay * mz - mz * by, c1 = mz * bx - ax * mz, c2 = ax * by - ay * bx;
    const double cross = sqrt((c0 * c0 + c1 * c1) + c2 * c2), dot = (ax * bx + ay * by) + mz * mz;
    return atan2(cross, dot) * SC_RAD2DEG;
}

// The final pass at c -> F[0 .. 7] sums, F[8 .. 10] maxima.
__device__ __forceinline__ void sc_final(const double* __restrict__ rows, const int n, const int lane, const double (&c)[2 * SC_KMAX], const int K,
                                         const double huber, double* c_lds, double* s_lds, double (&F)[SC_NF + SC_NM]) {
#pragma clang fp contract(off)
    double acc[SC_NF + SC_NM];
#pragma unroll
    for (int j = 0; j < SC_NF + SC_NM; ++j) acc[j] = 0.0;
    for (int i = lane; i < n; i += SC_WAVE) {
        const double* r = rows + (size_t)i * SC_ROW;
        const double w = r[9];
        if (!(w > 0.0)) continue;
        double phi[SC_KMAX];
        sc_phi(r[0], r[1], phi);
        const double px = sc_shift(phi, c, K), py = sc_shift(phi, c + SC_KMAX, K);
        const double xm = r[2], ym = r[3], tmx = r[4], tmy = r[5], e0 = r[6], e1 = r[7], mz = -r[8];
        const double ex = tmx - xm, ey = tmy - ym;
        const double rx = px - ex, ry = py - ey, qx = 0.0 - ex, qy = 0.0 - ey;
        const double r2 = rx * rx + ry * ry, rr = sqrt(r2), q2 = qx * qx + qy * qy, qq = sqrt(q2);
        const double inl = (huber > 0.0 && rr > huber) ? 0.0 : 1.0;
        const double deg = sc_angle((xm + px) - e0, (ym + py) - e1, tmx - e0, tmy - e1, mz);
        const double deg_raw = sc_angle((xm + 0.0) - e0, (ym + 0.0) - e1, tmx - e0, tmy - e1, mz);
        const double sh = sqrt(px * px + py * py);
        acc[0] = acc[0] + w * r2;
        acc[1] = acc[1] + w * rr;
        acc[2] = acc[2] + inl;
        acc[3] = acc[3] + 1.0;
        acc[4] = acc[4] + w * deg;
        acc[5] = acc[5] + w * q2;
        acc[6] = acc[6] + w * qq;
        acc[7] = acc[7] + w * deg_raw;
        acc[8] = rr > acc[8] ? rr : acc[8];
        acc[9] = qq > acc[9] ? qq : acc[9];
        acc[10] = sh > acc[10] ? sh : acc[10];
    }
    sc_columns<SC_NF + SC_NM>(acc, lane, SC_NF, c_lds, s_lds, F);
}

__global__ __launch_bounds__(SC_WAVE) void screen_calib_fit_kernel(const int C, const double* __restrict__ samples, const int* __restrict__ count,
                                                                   const uint8_t* __restrict__ select, const int mode, const int kind,
                                                                   const double huber, const int min_samples, const double max_shift,
                                                                   double* __restrict__ coef, double* __restrict__ report, int* __restrict__ used,
                                                                   int* __restrict__ inliers, int* __restrict__ solves, uint8_t* __restrict__ ok_out,
                                                                   double* __restrict__ coef_store, uint8_t* __restrict__ kind_store) {
#pragma clang fp contract(off)
    __shared__ double c_lds[SC_WAVE * SC_NC];
    __shared__ double s_lds[SC_NC];
    const int lane = threadIdx.x;
    const long long q = blockIdx.x;
    const bool chosen = !select || select[q] != 0;
    int n = C;
    if (count) n = min(max(count[q], 0), C);
    const double* rows = samples + (size_t)q * C * SC_ROW;
    double c[2 * SC_KMAX], F[SC_NF + SC_NM];
#pragma unroll
    for (int j = 0; j < 2 * SC_KMAX; ++j) c[j] = 0.0;
#pragma unroll
    for (int j = 0; j < SC_NF + SC_NM; ++j) F[j] = 0.0;
    bool ok = false;
    int n_used = 0, n_solves = 0, k_out = kind;
    if (chosen && mode == 1) {               // (uniform over the workgroup, like every branch below)
        k_out = kind_store[q];
        const int K = sc_terms(k_out);
        if (K > 0) {
#pragma unroll
            for (int j = 0; j < 2 * SC_KMAX; ++j) c[j] = coef_store[q * 2 * SC_KMAX + j];
        }
        sc_final(rows, n, lane, c, K, 0.0, c_lds, s_lds, F);
        n_used = (int)F[3];
        ok = n_used >= 1;
    } else if (chosen) {
        const int K = sc_terms(kind);
        double S[SC_NC];
        sc_pass(rows, n, lane, c, K, huber, c_lds, s_lds, S);
        n_used = (int)S[SC_NC - 1];
        bool go = n_used >= min_samples && n_used >= K && sc_finite(S[SC_NC - 5]);
        if (go) {
            go = sc_solve(S, K, c);
            n_solves = 1;
        }
        if (go && huber > 0.0) {
            bool converged = false;
            while (go && !converged) {
                double cn[2 * SC_KMAX];
                sc_pass(rows, n, lane, c, K, huber, c_lds, s_lds, S);
                go = sc_solve(S, K, cn);
                ++n_solves;
                double step = 0.0;
                bool fin = true;
#pragma unroll
                for (int j = 0; j < 2 * SC_KMAX; ++j) {
                    const double d = fabs(cn[j] - c[j]);
                    step = d > step ? d : step;
                    fin = fin && sc_finite(cn[j]);
                    c[j] = cn[j];
                }
                converged = go && fin && step <= 1e-6;
                if (!converged && n_solves == SC_MAX_SOLVES) go = false;
            }
        }
        if (go) {
            sc_final(rows, n, lane, c, K, huber, c_lds, s_lds, F);
            ok = !(F[10] > max_shift);
        }
    }
    if (lane == 0) {
        const double nn = F[3];
#pragma unroll
        for (int j = 0; j < 2 * SC_KMAX; ++j) coef[q * 2 * SC_KMAX + j] = ok ? c[j] : 0.0;
        double* rep = report + q * 8;
        rep[0] = ok ? sqrt(F[0] / nn) : 0.0;
        rep[1] = ok ? F[1] / nn : 0.0;
        rep[2] = ok ? F[8] : 0.0;
        rep[3] = ok ? F[4] / nn : 0.0;
        rep[4] = ok ? sqrt(F[5] / nn) : 0.0;
        rep[5] = ok ? F[6] / nn : 0.0;
        rep[6] = ok ? F[9] : 0.0;
        rep[7] = ok ? F[7] / nn : 0.0;
        used[q] = n_used;
        inliers[q] = ok ? (int)F[2] : 0;
        solves[q] = ok ? n_solves : 0;
        ok_out[q] = ok ? 1 : 0;
        if (ok && mode == 0 && coef_store) {
#pragma unroll
            for (int j = 0; j < 2 * SC_KMAX; ++j) coef_store[q * 2 * SC_KMAX + j] = c[j];
            kind_store[q] = (uint8_t)k_out;
        }
    }
}

__global__ __launch_bounds__(256) void screen_calib_apply_kernel(const long long N, const int T, const float* __restrict__ px_in,
                                                                 const float* __restrict__ ppm, const double* __restrict__ coef,
                                                                 const uint8_t* __restrict__ kind, const double W, const double H,
                                                                 float* __restrict__ px_out) {
#pragma clang fp contract(off)
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const long long b = n / T;
    const int K = sc_terms(kind[b]);
    const float xf = px_in[2 * n], yf = px_in[2 * n + 1];
    if (K == 0) {                            // no map: the input's bits
        px_out[2 * n] = xf;
        px_out[2 * n + 1] = yf;
        return;
    }
    const double x = (double)xf, y = (double)yf;
    double phi[SC_KMAX];
    sc_phi((x + x) / W - 1.0, (y + y) / H - 1.0, phi);
    const double* c = coef + b * 2 * SC_KMAX;
    const double xs = x + sc_shift(phi, c, K) * (double)ppm[2 * n], ys = y + sc_shift(phi, c + SC_KMAX, K) * (double)ppm[2 * n + 1];
    px_out[2 * n] = (float)(xs < 0.0 ? 0.0 : (xs > W ? W : xs));      // (a NaN stays a NaN)
    px_out[2 * n + 1] = (float)(ys < 0.0 ? 0.0 : (ys > H ? H : ys));
}

}  // namespace
}  // namespace eve

using namespace eve;

extern "C" int eve_screen_calib_append(long long B, int T, const float* pog, const float* origin, const float* inv_cam, const float* ppm,
                                       const float* target, const uint8_t* valid, const int* lengths, const uint8_t* frame_valid, double W,
                                       double H, int C, double* samples, int* count, int* dropped, eve_stream_t stream) {
    const char* why = nullptr;
    if (B <= 0 || T <= 0 || C <= 0 || !pog || !origin || !inv_cam || !ppm || !target || !samples || !count || !dropped) why = "bad arguments";
    else if (!(W > 0.0) || !(H > 0.0) || !(W <= 1.79769313486231570815e308) || !(H <= 1.79769313486231570815e308))
        why = "W and H must be finite numbers > 0";
    else if (B > (long long)0x7fffffff / T) why = "B * T must fit 31 bits";
    else if (B > (long long)0x7fffffff / C) why = "B * C must fit 31 bits";
    if (why) {
        char msg[128];
        snprintf(msg, sizeof(msg), "screen_calib_append: %s", why);
        return set_error_msg(msg);
    }
    EVE_LAUNCH("screen_calib_append_kernel", screen_calib_append_kernel, dim3((unsigned)((B + SC_WAVE - 1) / SC_WAVE)), dim3(SC_WAVE), 0,
               (hipStream_t)stream, B, T, pog, origin, inv_cam, ppm, target, valid, lengths, frame_valid, W, H, C, samples, count, dropped);
    EVE_CHECK_LAUNCH();
    return 0;
}

extern "C" int eve_screen_calib_fit(long long S, int C, const double* samples, const int* count, const uint8_t* select, int mode, int kind,
                                    double huber_mm, int min_samples, double max_shift_mm, double* coef, double* report, int* used,
                                    int* inliers, int* solves, uint8_t* ok, double* coef_store, uint8_t* kind_store, eve_stream_t stream) {
    const char* why = nullptr;
    if (S <= 0 || C <= 0 || !samples || !coef || !report || !used || !inliers || !solves || !ok) why = "bad arguments";
    else if (S > (long long)0x7fffffff / C) why = "S * C must fit 31 bits";
    else if (mode != 0 && mode != 1) why = "mode is 0 (fit) or 1 (evaluate the stored map)";
    else if ((coef_store != nullptr) != (kind_store != nullptr)) why = "coef_store and kind_store come together";
    else if (mode == 1 && !coef_store) why = "mode 1 reads coef_store and kind_store";
    else if (mode == 0 && (kind < 1 || kind > 3)) why = "kind is 1 (offset), 2 (affine) or 3 (quadratic)";
    else if (mode == 0 && min_samples < 1) why = "min_samples must be >= 1";
    else if (mode == 0 && !(huber_mm <= 1.79769313486231570815e308)) why = "huber_mm must be a number (<= 0: no loss)";      // a NaN
    else if (mode == 0 && !(max_shift_mm > 0.0)) why = "max_shift_mm must be > 0";
    if (why) {
        char msg[128];
        snprintf(msg, sizeof(msg), "screen_calib_fit: %s", why);
        return set_error_msg(msg);
    }
    EVE_LAUNCH("screen_calib_fit_kernel", screen_calib_fit_kernel, dim3((unsigned)S), dim3(SC_WAVE), 0, (hipStream_t)stream, C, samples, count,
               select, mode, kind, huber_mm > 0.0 ? huber_mm : 0.0, min_samples, max_shift_mm, coef, report, used, inliers, solves, ok, coef_store,
               kind_store);
    EVE_CHECK_LAUNCH();
    return 0;
}

extern "C" int eve_screen_calib_apply(long long B, int T, const float* px_in, const float* ppm, const double* coef, const uint8_t* kind, double W,
                                      double H, float* px_out, eve_stream_t stream) {
    const char* why = nullptr;
    if (B <= 0 || T <= 0 || !px_in || !ppm || !coef || !kind || !px_out) why = "bad arguments";
    else if (!(W > 0.0) || !(H > 0.0) || !(W <= 1.79769313486231570815e308) || !(H <= 1.79769313486231570815e308))
        why = "W and H must be finite numbers > 0";
    else if (B > (long long)0x7fffffff / 2 / T) why = "B * T * 2 must fit 31 bits";
    if (why) {
        char msg[128];
        snprintf(msg, sizeof(msg), "screen_calib_apply: %s", why);
        return set_error_msg(msg);
    }
    const long long N = B * T;
    EVE_LAUNCH("screen_calib_apply_kernel", screen_calib_apply_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, N, T,
               px_in, ppm, coef, kind, W, H, px_out);
    EVE_CHECK_LAUNCH();
    return 0;
}
