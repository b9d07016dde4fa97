// Head pose from face landmarks, on the device: what a face tracker really delivers (2-D landmarks of the undistorted image) plus the
// head model they belong to -> head_R, head_t per frame, the stage a live caller ran cv2.solvePnP for.  A weighted perspective-n-point
// solve by Levenberg-Marquardt on the reprojection error in normalised image coordinates, the rotation updated through the Cayley
// map, so that only + - * / and sqrt occur; the contract -- operation order included -- is in include/eve_hip.h
// (eve_face_pose_solve) and in numpy in tests/face_pose_ref.py.
//
// One wavefront (a 64-thread workgroup) per sequence, which walks its frames in time order: each frame starts from the previous
// frame's float64 solution, the first one from the carried state.  Lanes own landmarks (lane i: points i and i + 64, L <= 68).  Per
// evaluation every lane writes its points' 29 contributions (21 entries of J^T W J, 6 of the gradient, the cost, the squared pixel
// error) to LDS, lane j < 29 adds column j in landmark order 0 .. L-1, and every lane reads the 29 sums back: from there on the
// damped 6 x 6 Cholesky solve and the accept / reject decision are the same bits in all 64 lanes, so every branch is wave-uniform.
// Float64 throughout, every operation rounded on its own.  A frame costs 5-7 evaluations from a warm start (tens of microseconds
// of dependent float64 latency, no bandwidth); S sequences run side by side on S compute units.
#include "common.h"

#pragma clang fp contract(off)

namespace eve {
namespace {

constexpr int FP_WAVE = 64;
constexpr int FP_MIN_L = 4, FP_MAX_L = 68;
constexpr int FP_NC = 29;                // 21 + 6 + cost + pixel error
constexpr int FP_MAX_ACCEPTED = 32;

__device__ __forceinline__ bool fp_finite(const double x) { return fabs(x) <= 1.79769313486231570815e308; }      // false for a NaN

struct FpPoints {                        // the (up to) two landmarks of this lane
    double X[2][3], x[2], y[2], w[2];
    bool has[2], used[2];
};

// The in-order sums: every lane has written its rows of c_lds[l][FP_NC] (columns 0 .. NCOLS-1); lane j adds column j over l = 0 ..
// L-1 from 0.0 and all lanes read the sums back.
template <int NCOLS>
__device__ __forceinline__ void fp_ordered_sums(const int lane, const int L, double* c_lds, double* s_lds, double (&S)[NCOLS]) {
#pragma clang fp contract(off)
    __syncthreads();
    if (lane < NCOLS) {
        double s = 0.0;
        for (int l = 0; l < L; ++l) s = s + c_lds[l * FP_NC + lane];
        s_lds[lane] = s;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NCOLS; ++j) S[j] = s_lds[j];
}

// eval(R, t) of the contract -> the 29 sums; returns behind (a used point with not P2 > 0), wave-uniform.
__device__ __forceinline__ bool fp_eval(const double (&R)[9], const double (&t)[3], const double fx, const double fy, const FpPoints& p,
                                        const int lane, const int L, double* c_lds, double* s_lds, double (&S)[FP_NC]) {
#pragma clang fp contract(off)
    bool behind = false;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (!p.has[k]) continue;
        double* row = c_lds + (lane + k * FP_WAVE) * FP_NC;
        if (!p.used[k]) {
#pragma unroll
            for (int j = 0; j < FP_NC; ++j) row[j] = 0.0;
            continue;
        }
        double q[3], P[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            q[i] = (R[i * 3] * p.X[k][0] + R[i * 3 + 1] * p.X[k][1]) + R[i * 3 + 2] * p.X[k][2];
            P[i] = q[i] + t[i];
        }
        behind = behind || !(P[2] > 0.0);
        const double iz = 1.0 / P[2], px = P[0] / P[2], py = P[1] / P[2];
        const double ex = px - p.x[k], ey = py - p.y[k], a = px * iz, b = py * iz, w = p.w[k];
        const double Jx[6] = {-(a * q[1]), iz * q[2] + a * q[0], -(iz * q[1]), iz, 0.0, -a};
        const double Jy[6] = {-(iz * q[2] + b * q[1]), b * q[0], iz * q[0], 0.0, iz, -b};
        int c = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) row[c++] = w * (Jx[i] * Jx[j] + Jy[i] * Jy[j]);
#pragma unroll
        for (int i = 0; i < 6; ++i) row[21 + i] = w * (Jx[i] * ex + Jy[i] * ey);
        row[27] = w * (ex * ex + ey * ey);
        row[28] = w * ((fx * ex) * (fx * ex) + (fy * ey) * (fy * ey));
    }
    fp_ordered_sums<FP_NC>(lane, L, c_lds, s_lds, S);
    return __any(behind ? 1 : 0) != 0;
}

// Cholesky(M, thr) of the contract: the lower factor in Lo; false where a pivot fails.
__device__ __forceinline__ bool fp_cholesky(const double (&M)[6][6], const double thr, double (&Lo)[6][6]) {
#pragma clang fp contract(off)
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double s = M[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) s = s - Lo[j][k] * Lo[j][k];
        ok = ok && (s > thr * M[j][j]);
        Lo[j][j] = sqrt(s);
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double u = M[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) u = u - Lo[i][k] * Lo[j][k];
            Lo[i][j] = u / Lo[j][j];
        }
    }
    return ok;                           // (after a failed pivot the rest is garbage that nobody reads)
}

__device__ __forceinline__ void fp_unpack(const double (&S)[FP_NC], double (&A)[6][6]) {
    int c = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) {
            A[i][j] = S[c];
            A[j][i] = S[c];
            ++c;
        }
}

// One frame.  R, t: the initial pose when warm, and the solution where the frame is valid.  -> valid; *rms = sqrt(pix / sw).
__device__ __forceinline__ bool fp_solve_frame(const bool warm, double (&R)[9], double (&t)[3], const double fx, const double fy, const FpPoints& p,
                                               const int lane, const int L, double* c_lds, double* s_lds, double* rms) {
#pragma clang fp contract(off)
    // sw, and the cold start's centroids: in-order sums like every other
    double S1[6];
#pragma unroll
    for (int k = 0; k < 2; ++k)
        if (p.has[k]) {
            double* row = c_lds + (lane + k * FP_WAVE) * FP_NC;
            const double w = p.w[k];
            row[0] = w;
            row[1] = w * p.x[k];
            row[2] = w * p.y[k];
            row[3] = w * p.X[k][0];
            row[4] = w * p.X[k][1];
            row[5] = w * p.X[k][2];
        }
    fp_ordered_sums<6>(lane, L, c_lds, s_lds, S1);
    const double sw = S1[0];
    if (!warm) {
        const double mx = S1[1] / sw, my = S1[2] / sw, MX = S1[3] / sw, MY = S1[4] / sw, MZ = S1[5] / sw;
        double S2[2];
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (p.has[k]) {
                double* row = c_lds + (lane + k * FP_WAVE) * FP_NC;
                const double dx = p.x[k] - mx, dy = p.y[k] - my, dX = p.X[k][0] - MX, dY = p.X[k][1] - MY;
                row[0] = p.w[k] * (dx * dx + dy * dy);
                row[1] = p.w[k] * (dX * dX + dY * dY);
            }
        fp_ordered_sums<2>(lane, L, c_lds, s_lds, S2);
        if (!(S2[0] > 0.0 && S2[1] > 0.0)) return false;
        const double Z = sqrt(S2[1] / S2[0]);
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
        t[0] = mx * Z - MX;
        t[1] = my * Z - MY;
        t[2] = Z - MZ;
    }
    double S[FP_NC];
    if (fp_eval(R, t, fx, fy, p, lane, L, c_lds, s_lds, S) || !fp_finite(S[27])) return false;
    double lam = 1e-3;
    int accepted = 0;
    // accepted <= 32 and lam moves one decade per pass between 1e-35 and 1e12: fewer than 96 passes, whatever the data
    for (int pass = 0; pass < 96; ++pass) {
        double M[6][6], Lo[6][6];
        fp_unpack(S, M);
#pragma unroll
        for (int i = 0; i < 6; ++i) M[i][i] = M[i][i] + lam * M[i][i];
        if (!fp_cholesky(M, 0.0, Lo)) return false;
        double yv[6], d[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double s = -S[21 + i];
#pragma unroll
            for (int k = 0; k < i; ++k) s = s - Lo[i][k] * yv[k];
            yv[i] = s / Lo[i][i];
        }
#pragma unroll
        for (int i = 5; i >= 0; --i) {
            double s = yv[i];
#pragma unroll
            for (int k = i + 1; k < 6; ++k) s = s - Lo[k][i] * d[k];
            d[i] = s / Lo[i][i];
        }
        bool finite = true;
        double dm = 0.0, tm = 1.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            finite = finite && fp_finite(d[i]);
            if (fabs(d[i]) > dm) dm = fabs(d[i]);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (fabs(t[i]) > tm) tm = fabs(t[i]);
        const bool small = finite && dm < 1e-10 * tm;
        // the Cayley map of d[0:3], applied from the left
        const double a0 = 0.5 * d[0], a1 = 0.5 * d[1], a2 = 0.5 * d[2];
        const double s = (a0 * a0 + a1 * a1) + a2 * a2;
        const double den = 1.0 + s, e = 1.0 - s;
        const double C[9] = {(e + 2.0 * (a0 * a0)) / den, (2.0 * (a0 * a1 - a2)) / den, (2.0 * (a0 * a2 + a1)) / den,
                             (2.0 * (a0 * a1 + a2)) / den, (e + 2.0 * (a1 * a1)) / den, (2.0 * (a1 * a2 - a0)) / den,
                             (2.0 * (a0 * a2 - a1)) / den, (2.0 * (a1 * a2 + a0)) / den, (e + 2.0 * (a2 * a2)) / den};
        double Rc[9], tc[3], Sc[FP_NC];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) Rc[i * 3 + j] = (C[i * 3] * R[j] + C[i * 3 + 1] * R[3 + j]) + C[i * 3 + 2] * R[6 + j];
            tc[i] = t[i] + d[3 + i];
        }
        const bool behind = fp_eval(Rc, tc, fx, fy, p, lane, L, c_lds, s_lds, Sc);
        bool converged = false;
        if (finite && !behind && Sc[27] <= S[27]) {
#pragma unroll
            for (int i = 0; i < 9; ++i) R[i] = Rc[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) t[i] = tc[i];
#pragma unroll
            for (int i = 0; i < FP_NC; ++i) S[i] = Sc[i];
            lam = lam / 10.0;
            ++accepted;
            if (small) converged = true;
            else if (accepted == FP_MAX_ACCEPTED) return false;
        } else if (small) {
            converged = true;
        } else {
            lam = lam * 10.0;
            if (lam > 1e12) return false;
        }
        if (converged) {
            // observability: the undamped normal matrix must factor with pivots that are not rounding residue
            fp_unpack(S, M);
            if (!fp_cholesky(M, 1e-10, Lo)) return false;
            *rms = sqrt(S[28] / sw);
            return true;
        }
    }
    return false;
}

__global__ __launch_bounds__(FP_WAVE) void face_pose_solve_kernel(const int T, const int L, const int LC, const float* __restrict__ landmarks,
                                                                  const float* __restrict__ rig, const int* __restrict__ lengths,
                                                                  double* __restrict__ state, const int* __restrict__ reset,
                                                                  float* __restrict__ head_R, float* __restrict__ head_t,
                                                                  float* __restrict__ rms_out, uint8_t* __restrict__ valid_out) {
#pragma clang fp contract(off)
    __shared__ double c_lds[FP_MAX_L * FP_NC];
    __shared__ double s_lds[32];
    const int lane = threadIdx.x;
    const long long s = blockIdx.x;
    const float* r = rig + (size_t)s * (12 + 3 * L);
    FpPoints p;
    bool rig_ok = true;
#pragma unroll
    for (int j = 0; j < 12; ++j) rig_ok = rig_ok && fp_finite((double)r[j]);
    const double fx = (double)r[0], fy = (double)r[1], cx = (double)r[2], cy = (double)r[3];
    rig_ok = rig_ok && fx > 0.0 && fy > 0.0;
    bool pts_ok = true;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int l = lane + k * FP_WAVE;
        p.has[k] = l < L;
        p.used[k] = false;
        p.x[k] = p.y[k] = p.w[k] = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            p.X[k][i] = p.has[k] ? (double)r[12 + 3 * l + i] : 0.0;
            pts_ok = pts_ok && fp_finite(p.X[k][i]);
        }
    }
    rig_ok = rig_ok && __all(pts_ok ? 1 : 0) != 0;

    int len = T;
    if (lengths) len = min(max(lengths[s], 0), T);
    double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0};
    bool have = false, dirty = false;
    if (state) {
        const double* st = state + (size_t)s * 13;
        have = st[12] != 0.0;
        if (have) {
#pragma unroll
            for (int i = 0; i < 9; ++i) R[i] = st[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) t[i] = st[9 + i];
        }
    }
    if (reset && reset[s] != 0) {
        have = false;
        dirty = true;
    }
    for (int f = 0; f < T; ++f) {
        const long long n = s * T + f;
        bool valid = false;
        double rms = 0.0;
        if (f < len) {
            bool lm_ok = true;
#pragma unroll
            for (int k = 0; k < 2; ++k)
                if (p.has[k]) {
                    const float* q = landmarks + ((size_t)n * L + (lane + k * FP_WAVE)) * LC;
                    const double u = (double)q[0], v = (double)q[1], w = LC == 3 ? (double)q[2] : 1.0;
                    lm_ok = lm_ok && fp_finite(u) && fp_finite(v) && fp_finite(w);
                    p.used[k] = w > 0.0;
                    p.w[k] = p.used[k] ? w : 0.0;
                    p.x[k] = (u - cx) / fx;
                    p.y[k] = (v - cy) / fy;
                }
            const int count = __popcll(__ballot(p.used[0] ? 1 : 0)) + __popcll(__ballot(p.used[1] ? 1 : 0));
            const bool ok = rig_ok && __all(lm_ok ? 1 : 0) != 0 && count >= 4;
            if (ok) valid = fp_solve_frame(have, R, t, fx, fy, p, lane, L, c_lds, s_lds, &rms);
            have = valid;
            dirty = true;
            if (!valid) {
#pragma unroll
                for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
#pragma unroll
                for (int i = 0; i < 3; ++i) t[i] = 0.0;
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 9; ++i) head_R[(size_t)n * 9 + i] = valid ? (float)R[i] : ((i % 4 == 0) ? 1.0f : 0.0f);
#pragma unroll
            for (int i = 0; i < 3; ++i) head_t[(size_t)n * 3 + i] = valid ? (float)t[i] : 0.0f;
            rms_out[n] = valid ? (float)rms : 0.0f;
            valid_out[n] = valid ? 1 : 0;
        }
    }
    if (state && dirty && lane == 0) {
        double* st = state + (size_t)s * 13;
#pragma unroll
        for (int i = 0; i < 9; ++i) st[i] = have ? R[i] : ((i % 4 == 0) ? 1.0 : 0.0);
#pragma unroll
        for (int i = 0; i < 3; ++i) st[9 + i] = have ? t[i] : 0.0;
        st[12] = have ? 1.0 : 0.0;
    }
}

}  // namespace
}  // namespace eve

using namespace eve;

extern "C" int eve_face_pose_solve(long long S, int T, int L, int landmark_cols, const float* landmarks, const float* rig, const int* lengths,
                                   double* state, const int* reset, float* head_R, float* head_t, float* reproj_rms, uint8_t* valid,
                                   eve_stream_t stream) {
    const char* why = nullptr;
    if (S <= 0 || T <= 0 || !landmarks || !rig || !head_R || !head_t || !reproj_rms || !valid) why = "bad arguments";
    else if (L < FP_MIN_L || L > FP_MAX_L) why = "L must lie in 4..68";
    else if (landmark_cols != 2 && landmark_cols != 3) why = "landmarks have 2 or 3 columns (u, v[, w])";
    else if (S > (long long)0x7fffffff / T) why = "S * T must fit 31 bits";
    if (why) {
        char msg[128];
        snprintf(msg, sizeof(msg), "face_pose_solve: %s", why);
        return set_error_msg(msg);
    }
    EVE_LAUNCH("face_pose_solve_kernel", face_pose_solve_kernel, dim3((unsigned)S), dim3(FP_WAVE), 0, (hipStream_t)stream, T, L, landmark_cols,
               landmarks, rig, lengths, state, reset, head_R, head_t, reproj_rms, valid);
    EVE_CHECK_LAUNCH();
    return 0;
}
