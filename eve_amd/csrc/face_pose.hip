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
//
// eve_face_pose_solve_ex instantiates the same kernel over (LENS, ROBUST).  LENS: the landmarks are pixels of the RAW frame; when a
// frame's landmarks are loaded every lane inverts the lens model for its own points by Newton's method (fp_undistort: its own trip
// count, no barrier, no cross-lane operation), a point it cannot invert is dropped, and `used`, the count and sw follow from the
// survivors before anything wave-uniform is decided.  ROBUST: a Huber loss in pixels -- the weights of the 21 + 6 columns are
// scaled per point, the cost column becomes the Huber cost, a 30th column counts the inliers (68 x 30 doubles of LDS, summed by
// lanes 0 .. 29).  <false, false> is eve_face_pose_solve, bit for bit.  eve_undistort_points runs fp_undistort one thread per point.
#include "common.h"

#pragma clang fp contract(off)

namespace eve {
namespace {

constexpr int FP_WAVE = 64;
constexpr int FP_MIN_L = 4, FP_MAX_L = 68;
constexpr int FP_NC = 29;                // 21 + 6 + cost + pixel error
constexpr int FP_NC_ROBUST = 30;         // ... + the inlier count (the Huber loss)
constexpr int FP_MAX_NEWTON = 12;
constexpr int FP_MAX_ACCEPTED = 32;

__device__ __forceinline__ bool fp_finite(const double x) { return fabs(x) <= 1.79769313486231570815e308; }      // false for a NaN

struct FpPoints {                        // the (up to) two landmarks of this lane
    double X[2][3], x[2], y[2], w[2];
    bool has[2], used[2];
};

// The in-order sums: every lane has written its rows of c_lds[l][NC] (columns 0 .. NCOLS-1); lane j adds column j over l = 0 ..
// L-1 from 0.0 and all lanes read the sums back.
template <int NCOLS, int NC>
__device__ __forceinline__ void fp_ordered_sums(const int lane, const int L, double* c_lds, double* s_lds, double (&S)[NCOLS]) {
#pragma clang fp contract(off)
    __syncthreads();
    if (lane < NCOLS) {
        double s = 0.0;
        for (int l = 0; l < L; ++l) s = s + c_lds[l * NC + lane];
        s_lds[lane] = s;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NCOLS; ++j) S[j] = s_lds[j];
}

// A lens row of the contract (eve_undistort_points), widened.
struct FpLens {
    double fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6;
    bool plain;                          // all eight coefficients +-0: x = xd, y = yd, no iteration
};

// -> the row is usable: every entry finite, fx > 0, fy > 0.
__device__ __forceinline__ bool fp_lens_load(const float* __restrict__ row, FpLens& q) {
    double v[12];
    bool ok = true, plain = true;
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        v[j] = (double)row[j];
        ok = ok && fp_finite(v[j]);
        if (j >= 4) plain = plain && v[j] == 0.0;
    }
    q.fx = v[0], q.fy = v[1], q.cx = v[2], q.cy = v[3], q.k1 = v[4], q.k2 = v[5], q.p1 = v[6], q.p2 = v[7], q.k3 = v[8], q.k4 = v[9];
    q.k5 = v[10], q.k6 = v[11];
    q.plain = plain;
    return ok && q.fx > 0.0 && q.fy > 0.0;
}

// The raw pixel (u, v) -> the normalised point (x, y) of the undistorted image by Newton's method on the forward model; false
// (and x = y = 0.0) where the point is unusable.  The trip count differs from lane to lane: no barrier and no cross-lane
// operation in here.
__device__ __forceinline__ bool fp_undistort(const FpLens& q, const double u, const double v, double& xo, double& yo) {
#pragma clang fp contract(off)
    const double xd = (u - q.cx) / q.fx, yd = (v - q.cy) / q.fy;
    if (q.plain) {
        xo = xd;
        yo = yd;
        return true;
    }
    double x = xd, y = yd;
    bool done = false;
    for (int it = 0; it < FP_MAX_NEWTON; ++it) {
        const double xx = x * x, yy = y * y, xy = x * y, r2 = xx + yy;
        const double N = ((q.k3 * r2 + q.k2) * r2 + q.k1) * r2 + 1.0;
        const double D = ((q.k6 * r2 + q.k5) * r2 + q.k4) * r2 + 1.0;
        const double rad = N / D, a = xy + xy;
        const double gx = (x * rad + q.p1 * a) + q.p2 * (r2 + (xx + xx));
        const double gy = (y * rad + q.p1 * (r2 + (yy + yy))) + q.p2 * a;
        const double Np = ((3.0 * q.k3) * r2 + 2.0 * q.k2) * r2 + q.k1;
        const double Dp = ((3.0 * q.k6) * r2 + 2.0 * q.k5) * r2 + q.k4;
        const double rp = (Np - rad * Dp) / D, tw = rp + rp;
        const double j00 = ((rad + xx * tw) + 2.0 * (q.p1 * y)) + 6.0 * (q.p2 * x);
        const double j01 = (xy * tw + 2.0 * (q.p1 * x)) + 2.0 * (q.p2 * y);
        const double j11 = ((rad + yy * tw) + 6.0 * (q.p1 * y)) + 2.0 * (q.p2 * x);
        const double ex = gx - xd, ey = gy - yd, det = j00 * j11 - j01 * j01;
        const double dx = (j11 * ex - j01 * ey) / det, dy = (j00 * ey - j01 * ex) / det;
        if (!(fp_finite(dx) && fp_finite(dy))) break;
        x = x - dx;
        y = y - dy;
        double m = 1.0;
        if (fabs(x) > m) m = fabs(x);
        if (fabs(y) > m) m = fabs(y);
        const double dm = fabs(dx) > fabs(dy) ? fabs(dx) : fabs(dy);
        if (dm <= 4e-15 * m) {
            done = true;
            break;
        }
    }
    if (done) {
        const double xx = x * x, yy = y * y, r2 = xx + yy;
        done = ((q.k6 * r2 + q.k5) * r2 + q.k4) * r2 + 1.0 > 0.0;
    }
    xo = done ? x : 0.0;
    yo = done ? y : 0.0;
    return done;
}

// eval(R, t) of the contract -> the NC sums (29, or 30 with the Huber loss of huber pixels); returns behind (a used point with
// not P2 > 0), wave-uniform.
template <bool ROBUST, int NC>
__device__ __forceinline__ bool fp_eval(const double (&R)[9], const double (&t)[3], const double fx, const double fy, const double huber,
                                        const FpPoints& p, const int lane, const int L, double* c_lds, double* s_lds, double (&S)[NC]) {
#pragma clang fp contract(off)
    bool behind = false;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (!p.has[k]) continue;
        double* row = c_lds + (lane + k * FP_WAVE) * NC;
        if (!p.used[k]) {
#pragma unroll
            for (int j = 0; j < NC; ++j) row[j] = 0.0;
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
        const double p2 = (fx * ex) * (fx * ex) + (fy * ey) * (fy * ey);
        double ws = w;
        if constexpr (ROBUST) {
            const double r = sqrt(p2);
            const bool inlier = !(r > huber);
            ws = w * (inlier ? 1.0 : huber / r);
            row[27] = w * (inlier ? p2 : huber * ((r + r) - huber));
            row[NC - 1] = inlier ? 1.0 : 0.0;
        } else {
            row[27] = w * (ex * ex + ey * ey);
        }
        int c = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) row[c++] = ws * (Jx[i] * Jx[j] + Jy[i] * Jy[j]);
#pragma unroll
        for (int i = 0; i < 6; ++i) row[21 + i] = ws * (Jx[i] * ex + Jy[i] * ey);
        row[28] = w * p2;
    }
    fp_ordered_sums<NC, NC>(lane, L, c_lds, s_lds, S);
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

template <int NC>
__device__ __forceinline__ void fp_unpack(const double (&S)[NC], double (&A)[6][6]) {
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

// One frame.  R, t: the initial pose when warm, and the solution where the frame is valid.  -> valid; *rms = sqrt(pix / sw);
// with the Huber loss (ROBUST, huber pixels) *inliers = the 30th column's sum, and fewer than 4 of them make the frame invalid.
template <bool ROBUST>
__device__ __forceinline__ bool fp_solve_frame(const bool warm, double (&R)[9], double (&t)[3], const double fx, const double fy, const double huber,
                                               const FpPoints& p, const int lane, const int L, double* c_lds, double* s_lds, double* rms,
                                               int* inliers) {
#pragma clang fp contract(off)
    constexpr int NC = ROBUST ? FP_NC_ROBUST : FP_NC;
    // sw, and the cold start's centroids: in-order sums like every other
    double S1[6];
#pragma unroll
    for (int k = 0; k < 2; ++k)
        if (p.has[k]) {
            double* row = c_lds + (lane + k * FP_WAVE) * NC;
            const double w = p.w[k];
            row[0] = w;
            row[1] = w * p.x[k];
            row[2] = w * p.y[k];
            row[3] = w * p.X[k][0];
            row[4] = w * p.X[k][1];
            row[5] = w * p.X[k][2];
        }
    fp_ordered_sums<6, NC>(lane, L, c_lds, s_lds, S1);
    const double sw = S1[0];
    if (!warm) {
        const double mx = S1[1] / sw, my = S1[2] / sw, MX = S1[3] / sw, MY = S1[4] / sw, MZ = S1[5] / sw;
        double S2[2];
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (p.has[k]) {
                double* row = c_lds + (lane + k * FP_WAVE) * NC;
                const double dx = p.x[k] - mx, dy = p.y[k] - my, dX = p.X[k][0] - MX, dY = p.X[k][1] - MY;
                row[0] = p.w[k] * (dx * dx + dy * dy);
                row[1] = p.w[k] * (dX * dX + dY * dY);
            }
        fp_ordered_sums<2, NC>(lane, L, c_lds, s_lds, S2);
        if (!(S2[0] > 0.0 && S2[1] > 0.0)) return false;
        const double Z = sqrt(S2[1] / S2[0]);
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
        t[0] = mx * Z - MX;
        t[1] = my * Z - MY;
        t[2] = Z - MZ;
    }
    double S[NC];
    if (fp_eval<ROBUST, NC>(R, t, fx, fy, huber, p, lane, L, c_lds, s_lds, S) || !fp_finite(S[27])) return false;
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
        double Rc[9], tc[3], Sc[NC];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) Rc[i * 3 + j] = (C[i * 3] * R[j] + C[i * 3 + 1] * R[3 + j]) + C[i * 3 + 2] * R[6 + j];
            tc[i] = t[i] + d[3 + i];
        }
        const bool behind = fp_eval<ROBUST, NC>(Rc, tc, fx, fy, huber, p, lane, L, c_lds, s_lds, Sc);
        bool converged = false;
        if (finite && !behind && Sc[27] <= S[27]) {
#pragma unroll
            for (int i = 0; i < 9; ++i) R[i] = Rc[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) t[i] = tc[i];
#pragma unroll
            for (int i = 0; i < NC; ++i) S[i] = Sc[i];
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
            if constexpr (ROBUST) {
                if (S[NC - 1] < 4.0) return false;
                *inliers = (int)S[NC - 1];
            }
            *rms = sqrt(S[28] / sw);
            return true;
        }
    }
    return false;
}

// LENS: the landmarks are raw-frame pixels, undistorted through lens[n] (one row per frame) when they are loaded.  ROBUST: the Huber
// loss of huber pixels.  <false, false> is eve_face_pose_solve; inliers_out may be null.
template <bool LENS, bool ROBUST>
__global__ __launch_bounds__(FP_WAVE) void face_pose_solve_kernel(const int T, const int L, const int LC, const float* __restrict__ landmarks,
                                                                  const float* __restrict__ rig, const float* __restrict__ lens, const double huber,
                                                                  const int* __restrict__ lengths, double* __restrict__ state,
                                                                  const int* __restrict__ reset, float* __restrict__ head_R,
                                                                  float* __restrict__ head_t, float* __restrict__ rms_out,
                                                                  uint8_t* __restrict__ valid_out, uint8_t* __restrict__ inliers_out) {
#pragma clang fp contract(off)
    __shared__ double c_lds[FP_MAX_L * (ROBUST ? FP_NC_ROBUST : FP_NC)];
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
        int inl = 0;
        if (f < len) {
            bool lm_ok = true;
            FpLens lq;
            bool lens_ok = true;
            if constexpr (LENS) lens_ok = fp_lens_load(lens + (size_t)n * 12, lq);      // the same row in every lane
#pragma unroll
            for (int k = 0; k < 2; ++k)
                if (p.has[k]) {
                    const float* q = landmarks + ((size_t)n * L + (lane + k * FP_WAVE)) * LC;
                    const double u = (double)q[0], v = (double)q[1], w = LC == 3 ? (double)q[2] : 1.0;
                    const bool fin = fp_finite(u) && fp_finite(v) && fp_finite(w);
                    lm_ok = lm_ok && fin;
                    p.used[k] = w > 0.0;
                    if constexpr (LENS) {
                        // per lane, its own trip count; a frame that is invalid anyway skips the iteration
                        const bool usable = lens_ok && fin && fp_undistort(lq, u, v, p.x[k], p.y[k]);
                        if (!usable) p.x[k] = p.y[k] = 0.0;
                        p.used[k] = p.used[k] && usable;
                    } else {
                        p.x[k] = (u - cx) / fx;
                        p.y[k] = (v - cy) / fy;
                    }
                    p.w[k] = p.used[k] ? w : 0.0;
                }
            const int count = __popcll(__ballot(p.used[0] ? 1 : 0)) + __popcll(__ballot(p.used[1] ? 1 : 0));
            const bool ok = rig_ok && lens_ok && __all(lm_ok ? 1 : 0) != 0 && count >= 4;
            if (ok) valid = fp_solve_frame<ROBUST>(have, R, t, fx, fy, huber, p, lane, L, c_lds, s_lds, &rms, &inl);
            if constexpr (!ROBUST) inl = count;
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
            if (inliers_out) inliers_out[n] = valid ? (uint8_t)inl : 0;
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

// One thread per point: the contract of eve_undistort_points.
__global__ __launch_bounds__(256) void undistort_points_kernel(const long long N, const float* __restrict__ points, const float* __restrict__ lens,
                                                               const long long lens_stride, double* __restrict__ xy, uint8_t* __restrict__ ok_out) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    FpLens lq;
    const double u = (double)points[2 * i], v = (double)points[2 * i + 1];
    double x = 0.0, y = 0.0;
    bool ok = fp_lens_load(lens + (size_t)(i * lens_stride), lq) && fp_finite(u) && fp_finite(v);
    if (ok) ok = fp_undistort(lq, u, v, x, y);
    xy[2 * i] = ok ? x : 0.0;
    xy[2 * i + 1] = ok ? y : 0.0;
    ok_out[i] = ok ? 1 : 0;
}

}  // namespace
}  // namespace eve

using namespace eve;

namespace {
const char* fp_refusal(long long S, int T, int L, int landmark_cols, const void* landmarks, const void* rig, const void* head_R, const void* head_t,
                       const void* reproj_rms, const void* valid) {
    if (S <= 0 || T <= 0 || !landmarks || !rig || !head_R || !head_t || !reproj_rms || !valid) return "bad arguments";
    if (L < FP_MIN_L || L > FP_MAX_L) return "L must lie in 4..68";
    if (landmark_cols != 2 && landmark_cols != 3) return "landmarks have 2 or 3 columns (u, v[, w])";
    if (S > (long long)0x7fffffff / T) return "S * T must fit 31 bits";
    return nullptr;
}
}  // namespace

extern "C" int eve_face_pose_solve(long long S, int T, int L, int landmark_cols, const float* landmarks, const float* rig, const int* lengths,
                                   double* state, const int* reset, float* head_R, float* head_t, float* reproj_rms, uint8_t* valid,
                                   eve_stream_t stream) {
    if (const char* why = fp_refusal(S, T, L, landmark_cols, landmarks, rig, head_R, head_t, reproj_rms, valid)) {
        char msg[128];
        snprintf(msg, sizeof(msg), "face_pose_solve: %s", why);
        return set_error_msg(msg);
    }
    EVE_LAUNCH("face_pose_solve_kernel", (face_pose_solve_kernel<false, false>), dim3((unsigned)S), dim3(FP_WAVE), 0, (hipStream_t)stream, T, L,
               landmark_cols, landmarks, rig, (const float*)nullptr, 0.0, lengths, state, reset, head_R, head_t, reproj_rms, valid,
               (uint8_t*)nullptr);
    EVE_CHECK_LAUNCH();
    return 0;
}

extern "C" int eve_face_pose_solve_ex(long long S, int T, int L, int landmark_cols, const float* landmarks, const float* rig, const float* lens,
                                      double huber_px, const int* lengths, double* state, const int* reset, float* head_R, float* head_t,
                                      float* reproj_rms, uint8_t* valid, uint8_t* inliers, eve_stream_t stream) {
    const char* why = fp_refusal(S, T, L, landmark_cols, landmarks, rig, head_R, head_t, reproj_rms, valid);
    if (!why && !inliers) why = "bad arguments";
    if (!why && !(huber_px <= 1.79769313486231570815e308)) why = "huber_px must be a number (<= 0: no loss)";      // a NaN
    if (why) {
        char msg[128];
        snprintf(msg, sizeof(msg), "face_pose_solve_ex: %s", why);
        return set_error_msg(msg);
    }
    const bool robust = huber_px > 0.0;
    const dim3 grid((unsigned)S), block(FP_WAVE);
#define FP_EX_LAUNCH(LENS, ROBUST)                                                                                                              \
    EVE_LAUNCH("face_pose_solve_ex_kernel", (face_pose_solve_kernel<LENS, ROBUST>), grid, block, 0, (hipStream_t)stream, T, L, landmark_cols,     \
               landmarks, rig, lens, huber_px, lengths, state, reset, head_R, head_t, reproj_rms, valid, inliers)
    if (lens && robust) FP_EX_LAUNCH(true, true);
    else if (lens) FP_EX_LAUNCH(true, false);
    else if (robust) FP_EX_LAUNCH(false, true);
    else FP_EX_LAUNCH(false, false);
#undef FP_EX_LAUNCH
    EVE_CHECK_LAUNCH();
    return 0;
}

extern "C" int eve_undistort_points(long long N, const float* points, const float* lens, long long lens_stride, double* xy, uint8_t* ok,
                                    eve_stream_t stream) {
    const char* why = nullptr;
    if (N <= 0 || !points || !lens || !xy || !ok) why = "bad arguments";
    else if (lens_stride != 0 && lens_stride != 12) why = "lens_stride is 12 (one row per point) or 0 (one row for all)";
    else if (N > (long long)0x7fffffff * 256) why = "N is too large for one launch";
    if (why) {
        char msg[128];
        snprintf(msg, sizeof(msg), "undistort_points: %s", why);
        return set_error_msg(msg);
    }
    EVE_LAUNCH("undistort_points_kernel", undistort_points_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, N, points,
               lens, lens_stride, xy, ok);
    EVE_CHECK_LAUNCH();
    return 0;
}

