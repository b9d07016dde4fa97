// Per-person gaze calibration, on the device: the constant angular offset kappa = (pitch, yaw) between what EyeNet sees (the optical
// axis) and where a person looks (the visual axis), in the offset model eve_gaze_to_pog already applies as a training augmentation
// (gaze_geometry.hip, apply_offset_augmentation).  Two stages; the contract -- operation order included -- is in include/eve_hip.h
// (eve_calib_append, eve_calib_fit) and in numpy in tests/calib_ref.py.
//
//   eve_calib_append  one THREAD per (stream, eye), which walks the chunk's frames in time order: every usable frame is reduced to the
//                     16 doubles the fit needs (A = -(T3 R^T Rh Q), e, the target in millimetres, a weight) and appended to that
//                     sequence's sample store.  No atomics, no cross-lane operation: the store is a deterministic function of the steps.
//   eve_calib_fit     one wavefront (a 64-thread workgroup) per (stream, eye): Levenberg-Marquardt on the two angles from kappa = 0.
//                     Lane l adds the 9 contributions of samples l, l + 64, ... in order, writes its 9 partial sums to LDS, lane j < 9
//                     adds column j over the lanes 0 .. 63 in order, every lane reads the 9 sums back: from there on the 2 x 2 solve and
//                     the accept / reject decision are the same bits in all 64 lanes, so every branch is wave-uniform.
// Float64 throughout, every operation rounded on its own.
#include "common.h"

#pragma clang fp contract(off)

namespace eve {
namespace {

constexpr int CF_WAVE = 64;
constexpr int CF_ROW = 16;               // doubles per sample: A (9, row-major), e (3), m (2), the weight, a reserved 0.0
constexpr int CF_NC = 9;                 // JtJ (00, 01, 11), g (2), the cost, the squared error, the inliers, the used samples
constexpr int CF_MAX_ACCEPTED = 32;
constexpr int CF_MAX_EVALS = 64;

__device__ __forceinline__ bool cf_finite(const double x) { return fabs(x) <= 1.79769313486231570815e308; }      // false for a NaN

// C = A B, 3 x 3 row-major, each entry (a0*b0 + a1*b1) + a2*b2
__device__ __forceinline__ void cf_mul(const double (&A)[9], const double (&Bm)[9], double (&Cm)[9]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Cm[i * 3 + j] = (A[i * 3] * Bm[j] + A[i * 3 + 1] * Bm[3 + j]) + A[i * 3 + 2] * Bm[6 + j];
}

// One frame of one eye -> its row; false where the sample is not usable (a value that is not finite, c0 = 0, a target behind the eye).
__device__ __forceinline__ bool cf_reduce(const float* __restrict__ g, const float* __restrict__ head_R, const float* __restrict__ origin,
                                          const float* __restrict__ R, const float* __restrict__ T, const float* __restrict__ ppm,
                                          const float* __restrict__ target, double (&row)[CF_ROW]) {
#pragma clang fp contract(off)
    bool fin = true;
    double Rh[9], Re[9], Tm[16], o[3];
    const double p = (double)g[0], y = (double)g[1], sx = (double)ppm[0], sy = (double)ppm[1], cx = (double)target[0], cy = (double)target[1];
    fin = cf_finite(p) && cf_finite(y) && cf_finite(sx) && cf_finite(sy) && cf_finite(cx) && cf_finite(cy);
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        Rh[i] = (double)head_R[i];
        Re[i] = (double)R[i];
        fin = fin && cf_finite(Rh[i]) && cf_finite(Re[i]);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        Tm[i] = (double)T[i];
        fin = fin && cf_finite(Tm[i]);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        o[i] = (double)origin[i];
        fin = fin && cf_finite(o[i]);
    }
    if (!fin) return false;
    const double cp = cos(p), sp = sin(p), cyw = cos(y), syw = sin(y);
    const double v[3] = {cp * syw, sp, cp * cyw};
    double u[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) u[j] = (Rh[j] * v[0] + Rh[3 + j] * v[1]) + Rh[6 + j] * v[2];      // Rh^T v
    const double nu = sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
    const double ux = u[0] / nu, uy = u[1] / nu, uz = u[2] / nu;
    const double c0 = sqrt(ux * ux + uz * uz);
    if (!(c0 > 0.0)) return false;                                                                    // (also a NaN: nu = 0)
    const double s0 = uy, s1 = ux / c0, c1 = uz / c0;
    // Q = Ry Rx
    const double Q[9] = {c1, -(s1 * s0), s1 * c0, 0.0, c0, s0, -s1, -(c1 * s0), c1 * c0};
    double M1[9], M2[9], ReT[9], T3[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            ReT[i * 3 + j] = Re[j * 3 + i];
            T3[i * 3 + j] = Tm[i * 4 + j];
        }
    cf_mul(Rh, Q, M1);
    cf_mul(ReT, M1, M2);
    cf_mul(T3, M2, M1);
#pragma unroll
    for (int i = 0; i < 9; ++i) row[i] = -M1[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) row[9 + i] = ((Tm[i * 4] * o[0] + Tm[i * 4 + 1] * o[1]) + Tm[i * 4 + 2] * o[2]) + Tm[i * 4 + 3];
    row[12] = cx / sx;
    row[13] = cy / sy;
    row[14] = 1.0;
    row[15] = 0.0;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 14; ++i) ok = ok && cf_finite(row[i]);
    return ok && (-row[11] / row[8] > 0.0);                                                            // A k(0) = A's third column
}

__global__ __launch_bounds__(CF_WAVE) void calib_append_kernel(const long long S, const int T, const int E, const float* __restrict__ g,
                                                               const float* __restrict__ head_R, const float* __restrict__ origin,
                                                               const float* __restrict__ R, const float* __restrict__ inv_cam,
                                                               const float* __restrict__ ppm, const float* __restrict__ target,
                                                               const uint8_t* __restrict__ valid, const int* __restrict__ lengths,
                                                               const uint8_t* __restrict__ eye_valid, const int C,
                                                               double* __restrict__ samples, int* __restrict__ count,
                                                               int* __restrict__ dropped) {
#pragma clang fp contract(off)
    const long long q = (long long)blockIdx.x * CF_WAVE + threadIdx.x;      // the sequence: stream b, eye e
    if (q >= S) return;
    const long long b = q / E, N = (S / E) * T;
    const int e = (int)(q % E);
    int len = T;
    if (lengths) len = min(max(lengths[b], 0), T);
    int cnt = min(max(count[q], 0), C), drop = dropped[q];
    for (int f = 0; f < len; ++f) {
        const long long n = b * T + f, ne = (long long)e * N + n;
        if (valid && valid[n] == 0) continue;
        if (eye_valid && eye_valid[n * E + e] == 0) continue;
        double row[CF_ROW];
        if (!cf_reduce(g + ne * 2, head_R + n * 9, origin + ne * 3, R + ne * 9, inv_cam + n * 16, ppm + n * 2, target + n * 2, row)) continue;
        if (cnt >= C) {
            ++drop;
            continue;
        }
        double* dst = samples + ((size_t)q * C + cnt) * CF_ROW;
#pragma unroll
        for (int i = 0; i < CF_ROW; ++i) dst[i] = row[i];
        ++cnt;
    }
    count[q] = cnt;
    dropped[q] = drop;
}

// eval(kappa) of the contract -> the 9 sums, the same bits in every lane.
template <bool ROBUST>
__device__ __forceinline__ void cf_eval(const double* __restrict__ rows, const int n, const int lane, const double kp, const double ky,
                                        const double huber, double* c_lds, double* s_lds, double (&S)[CF_NC]) {
#pragma clang fp contract(off)
    const double cp = cos(kp), sp = sin(kp), cy = cos(ky), sy = sin(ky);
    const double k[3] = {cp * sy, sp, cp * cy};
    const double a[3] = {-(sp * sy), cp, -(sp * cy)};                    // d k / d pitch
    const double b0 = cp * cy, b2 = -(cp * sy);                          // d k / d yaw = (b0, 0, b2)
    double acc[CF_NC];
#pragma unroll
    for (int j = 0; j < CF_NC; ++j) acc[j] = 0.0;
    for (int i = lane; i < n; i += CF_WAVE) {
        const double* r = rows + (size_t)i * CF_ROW;
        const double w = r[14];
        if (!(w > 0.0)) continue;
        double d[3], dp[3], dy[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            d[j] = (r[3 * j] * k[0] + r[3 * j + 1] * k[1]) + r[3 * j + 2] * k[2];
            dp[j] = (r[3 * j] * a[0] + r[3 * j + 1] * a[1]) + r[3 * j + 2] * a[2];
            dy[j] = r[3 * j] * b0 + r[3 * j + 2] * b2;
        }
        const double ez = r[11], z2 = d[2] * d[2];
        const double rx = (r[9] - ez * (d[0] / d[2])) - r[12], ry = (r[10] - ez * (d[1] / d[2])) - r[13];
        const double Jxp = -(ez * ((dp[0] * d[2] - d[0] * dp[2]) / z2)), Jxy = -(ez * ((dy[0] * d[2] - d[0] * dy[2]) / z2));
        const double Jyp = -(ez * ((dp[1] * d[2] - d[1] * dp[2]) / z2)), Jyy = -(ez * ((dy[1] * d[2] - d[1] * dy[2]) / z2));
        const double r2 = rx * rx + ry * ry;
        double ws = w, cost = w * r2, inl = 1.0;
        if constexpr (ROBUST) {
            const double rr = sqrt(r2);
            const bool inlier = !(rr > huber);
            ws = w * (inlier ? 1.0 : huber / rr);
            cost = w * (inlier ? r2 : huber * ((rr + rr) - huber));
            inl = inlier ? 1.0 : 0.0;
        }
        acc[0] = acc[0] + ws * (Jxp * Jxp + Jyp * Jyp);
        acc[1] = acc[1] + ws * (Jxp * Jxy + Jyp * Jyy);
        acc[2] = acc[2] + ws * (Jxy * Jxy + Jyy * Jyy);
        acc[3] = acc[3] + ws * (Jxp * rx + Jyp * ry);
        acc[4] = acc[4] + ws * (Jxy * rx + Jyy * ry);
        acc[5] = acc[5] + cost;
        acc[6] = acc[6] + w * r2;
        acc[7] = acc[7] + inl;
        acc[8] = acc[8] + 1.0;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < CF_NC; ++j) c_lds[lane * CF_NC + j] = acc[j];
    __syncthreads();
    if (lane < CF_NC) {
        double s = 0.0;
        for (int l = 0; l < CF_WAVE; ++l) s = s + c_lds[l * CF_NC + lane];
        s_lds[lane] = s;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < CF_NC; ++j) S[j] = s_lds[j];
}

// The lower Cholesky factor of [[m00, m01], [m01, m11]]; false where a pivot is not above thr times its diagonal entry.
__device__ __forceinline__ bool cf_cholesky(const double m00, const double m01, const double m11, const double thr, double& l00, double& l10,
                                            double& l11) {
#pragma clang fp contract(off)
    bool ok = m00 > thr * m00;
    l00 = sqrt(m00);
    l10 = m01 / l00;
    const double s = m11 - l10 * l10;
    ok = ok && (s > thr * m11);
    l11 = sqrt(s);
    return ok;
}

template <bool ROBUST>
__global__ __launch_bounds__(CF_WAVE) void calib_fit_kernel(const int C, const double* __restrict__ samples, const int* __restrict__ count,
                                                            const uint8_t* __restrict__ select, const double huber, const int min_samples,
                                                            double* __restrict__ kappa, double* __restrict__ rms_mm, int* __restrict__ used,
                                                            int* __restrict__ inliers, uint8_t* __restrict__ ok_out,
                                                            float* __restrict__ kappa_store, uint8_t* __restrict__ ok_store) {
#pragma clang fp contract(off)
    __shared__ double c_lds[CF_WAVE * CF_NC];
    __shared__ double s_lds[16];
    const int lane = threadIdx.x;
    const long long q = blockIdx.x;
    const bool chosen = !select || select[q] != 0;
    int n = C;
    if (count) n = min(max(count[q], 0), C);
    const double* rows = samples + (size_t)q * C * CF_ROW;
    double kp = 0.0, ky = 0.0, S[CF_NC];
    bool ok = false;
    int n_used = 0;
    if (chosen) {                            // (uniform over the workgroup, like every branch below)
        cf_eval<ROBUST>(rows, n, lane, kp, ky, huber, c_lds, s_lds, S);
        n_used = (int)S[8];
        bool go = n_used >= min_samples && n_used >= 1 && cf_finite(S[5]);
        double lam = 1e-3;
        int accepted = 0, evals = 1;
        bool converged = false;
        while (go && !converged && evals < CF_MAX_EVALS) {
            double l00, l10, l11;
            if (!cf_cholesky(S[0] + lam * S[0], S[1], S[2] + lam * S[2], 0.0, l00, l10, l11)) break;
            const double y0 = -S[3] / l00, y1 = (-S[4] - l10 * y0) / l11;
            const double d1 = y1 / l11, d0 = (y0 - l10 * d1) / l00;
            const bool finite = cf_finite(d0) && cf_finite(d1);
            const double dm = fabs(d0) > fabs(d1) ? fabs(d0) : fabs(d1);
            const bool small = finite && dm <= 1e-12;
            const double kpc = kp + d0, kyc = ky + d1;
            double Sc[CF_NC];
            cf_eval<ROBUST>(rows, n, lane, kpc, kyc, huber, c_lds, s_lds, Sc);
            ++evals;
            if (finite && Sc[5] <= S[5]) {
                kp = kpc;
                ky = kyc;
#pragma unroll
                for (int j = 0; j < CF_NC; ++j) S[j] = Sc[j];
                lam = lam / 10.0;
                ++accepted;
                if (small) converged = true;
                else if (accepted == CF_MAX_ACCEPTED) go = false;
            } else if (small) {
                converged = true;
            } else {
                lam = lam * 10.0;
                if (lam > 1e12) go = false;
            }
        }
        if (go && converged) {
            // observability: the undamped normal matrix must factor with pivots that are not rounding residue
            double l00, l10, l11;
            ok = cf_cholesky(S[0], S[1], S[2], 1e-10, l00, l10, l11);
            ok = ok && !(sqrt(kp * kp + ky * ky) > 0.35);
        }
    }
    if (lane == 0) {
        kappa[2 * q] = ok ? kp : 0.0;
        kappa[2 * q + 1] = ok ? ky : 0.0;
        rms_mm[q] = ok ? sqrt(S[6] / S[8]) : 0.0;
        used[q] = n_used;
        inliers[q] = ok ? (int)S[7] : 0;
        ok_out[q] = ok ? 1 : 0;
        if (ok && kappa_store) {
            kappa_store[2 * q] = (float)kp;
            kappa_store[2 * q + 1] = (float)ky;
        }
        if (ok && ok_store) ok_store[q] = 1;
    }
}

}  // namespace
}  // namespace eve

using namespace eve;

extern "C" int eve_calib_append(long long B, int T, int E, const float* g, const float* head_R, const float* origin, const float* R,
                                const float* inv_cam, const float* ppm, const float* target, const uint8_t* valid, const int* lengths,
                                const uint8_t* eye_valid, int C, double* samples, int* count, int* dropped, eve_stream_t stream) {
    const char* why = nullptr;
    if (B <= 0 || T <= 0 || C <= 0 || !g || !head_R || !origin || !R || !inv_cam || !ppm || !target || !samples || !count || !dropped)
        why = "bad arguments";
    else if (E != 1 && E != 2) why = "E is 1 (one eye) or 2 (left, right)";
    else if (B > (long long)0x7fffffff / 2 / T) why = "B * T * E must fit 31 bits";
    else if (B * E > (long long)0x7fffffff / C) why = "B * E * C must fit 31 bits";
    if (why) {
        char msg[128];
        snprintf(msg, sizeof(msg), "calib_append: %s", why);
        return set_error_msg(msg);
    }
    const long long S = B * E;
    EVE_LAUNCH("calib_append_kernel", calib_append_kernel, dim3((unsigned)((S + CF_WAVE - 1) / CF_WAVE)), dim3(CF_WAVE), 0, (hipStream_t)stream, S,
               T, E, g, head_R, origin, R, inv_cam, ppm, target, valid, lengths, eye_valid, C, samples, count, dropped);
    EVE_CHECK_LAUNCH();
    return 0;
}

extern "C" int eve_calib_fit(long long S, int C, const double* samples, const int* count, const uint8_t* select, double huber_mm, int min_samples,
                             double* kappa, double* rms_mm, int* used, int* inliers, uint8_t* ok, float* kappa_store, uint8_t* ok_store,
                             eve_stream_t stream) {
    const char* why = nullptr;
    if (S <= 0 || C <= 0 || !samples || !kappa || !rms_mm || !used || !inliers || !ok) why = "bad arguments";
    else if (S > (long long)0x7fffffff / C) why = "S * C must fit 31 bits";
    else if (min_samples < 1) why = "min_samples must be >= 1";
    else if (!(huber_mm <= 1.79769313486231570815e308)) why = "huber_mm must be a number (<= 0: no loss)";      // a NaN
    else if ((kappa_store != nullptr) != (ok_store != nullptr)) why = "kappa_store and ok_store come together";
    if (why) {
        char msg[128];
        snprintf(msg, sizeof(msg), "calib_fit: %s", why);
        return set_error_msg(msg);
    }
    const dim3 grid((unsigned)S), block(CF_WAVE);
    if (huber_mm > 0.0)
        EVE_LAUNCH("calib_fit_kernel", calib_fit_kernel<true>, grid, block, 0, (hipStream_t)stream, C, samples, count, select, huber_mm,
                   min_samples, kappa, rms_mm, used, inliers, ok, kappa_store, ok_store);
    else
        EVE_LAUNCH("calib_fit_kernel", calib_fit_kernel<false>, grid, block, 0, (hipStream_t)stream, C, samples, count, select, 0.0, min_samples,
                   kappa, rms_mm, used, inliers, ok, kappa_store, ok_store);
    EVE_CHECK_LAUNCH();
    return 0;
}
