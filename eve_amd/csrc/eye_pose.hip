// Eye normalisation from the head pose, on the device: what a live caller's face tracker delivers (cv2.solvePnP's rvec and tvec, the
// camera matrix, the two eye centres of the head model) -> everything the pipeline reads per frame and eye: the warp inv(W) that
// eve_eye_warp_u8_* cuts the patch through, the rotation R that de-normalises the predicted gaze, the gaze origin o, the normalised
// head pose h, and head_R.  The procedure is the published one the reference cites for its precomputed values (Zhang et al. 2018,
// "Revisiting data normalization for appearance-based gaze estimation"); the contract -- operation order included -- is in
// include/eve_hip.h (eve_eye_pose_normalize) and in numpy in tests/eye_pose_ref.py.
//
// One thread per (frame, eye), eye-major: thread i < N is frame i's left eye, thread N + i its right eye; the left eye's thread also
// writes head_R (both compute it: sin and cos of the same bits).  Float64 throughout, every operation rounded on its own (no
// contraction: none of these products is exact), each stage rounded to float32 and the next continued from the rounded value, so
// o, R and warp are bit-exact functions of the head_R that was written.  A few hundred flops and 180 bytes per thread: the launch
// is at the launch floor at every batch the pipeline sees, and nothing about its shape depends on the data.
#include "common.h"

#pragma clang fp contract(off)

namespace eve {
namespace {

constexpr int EP_THREADS = 64;
constexpr int EP_MAX_PATCH = 4096;       // OH, OW: the limit of the warp kernels that read the result

__device__ __forceinline__ double norm3(const double a0, const double a1, const double a2) {
#pragma clang fp contract(off)
    return sqrt((a0 * a0 + a1 * a1) + a2 * a2);
}

__device__ __forceinline__ void cross3(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
#pragma clang fp contract(off)
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ bool finite64(const double x) { return fabs(x) <= 1.79769313486231570815e308; }      // false for a NaN

// Stages 2-6 of the contract for eye i = e * N + n, from H = the float32 head_R just written (widened) and the translation tv:
// shared by the pose form (stage 1 = Rodrigues) and by eve_eye_pose_normalize_rt (head_R and head_t as they come).
__device__ __forceinline__ void eye_normalize_from_rt(const long long i, const int e, const double (&H)[3][3], const double (&tv)[3], const double fx,
                                                      const double fy, const double cx, const double cy, const double (&cl)[3],
                                                      const double (&cr)[3], const double f, const double dn, const bool row_ok, const int OH,
                                                      const int OW, float* __restrict__ o_out, float* __restrict__ R_out,
                                                      float* __restrict__ warp_out, float* __restrict__ h_out, uint8_t* __restrict__ valid_out) {
#pragma clang fp contract(off)
    // 2. o = head_R c + t, rounded to float32
    const double c0 = e ? cr[0] : cl[0], c1 = e ? cr[1] : cl[1], c2 = e ? cr[2] : cl[2];
    float o32[3];
    double o[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        o32[a] = (float)(((H[a][0] * c0 + H[a][1] * c1) + H[a][2] * c2) + tv[a]);
        o[a] = (double)o32[a];
    }

    // 3. R: rows right, down, forward, rounded to float32
    const double d = norm3(o[0], o[1], o[2]);
    const double fw[3] = {o[0] / d, o[1] / d, o[2] / d};
    const double hx[3] = {H[0][0], H[1][0], H[2][0]};
    double t3[3];
    cross3(fw, hx, t3);
    const double nd = norm3(t3[0], t3[1], t3[2]);
    const double down[3] = {t3[0] / nd, t3[1] / nd, t3[2] / nd};
    cross3(down, fw, t3);
    const double nr = norm3(t3[0], t3[1], t3[2]);
    const double right[3] = {t3[0] / nr, t3[1] / nr, t3[2] / nr};
    float R32[3][3];
    double R[3][3];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        R32[0][b] = (float)right[b];
        R32[1][b] = (float)down[b];
        R32[2][b] = (float)fw[b];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) R[a][b] = (double)R32[a][b];

    // 4. warp = inv(W) = K R^T diag(1, 1, d / dn) Kn^-1
    const double z = d / dn, g = 1.0 / f, px = ((double)OW * 0.5) / f, py = ((double)OH * 0.5) / f;
    double A[3][3], B[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        A[a][0] = R[0][a];
        A[a][1] = R[1][a];
        A[a][2] = R[2][a] * z;
    }
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        B[0][b] = fx * A[0][b] + cx * A[2][b];
        B[1][b] = fy * A[1][b] + cy * A[2][b];
        B[2][b] = A[2][b];
    }
    float w32[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        w32[a][0] = (float)(B[a][0] * g);
        w32[a][1] = (float)(B[a][1] * g);
        w32[a][2] = (float)((B[a][2] - B[a][0] * px) - B[a][1] * py);
    }

    // 5. h from the third column of R head_R
    double m[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) m[a] = (R[a][0] * H[0][2] + R[a][1] * H[1][2]) + R[a][2] * H[2][2];
    const float h0 = (float)asin(fmin(fmax(m[1], -1.0), 1.0)), h1 = (float)atan2(m[0], m[2]);

    // 6. valid; an invalid eye: warp = 0, R = I, o = 0, h = 0
    const bool valid = row_ok && o[2] > 0.0 && d > 0.0 && nd > 0.0 && nr > 0.0;
    float* po = o_out + (size_t)i * 3;
    float* pR = R_out + (size_t)i * 9;
    float* pw = warp_out + (size_t)i * 9;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        po[a] = valid ? o32[a] : 0.0f;
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            pR[a * 3 + b] = valid ? R32[a][b] : (a == b ? 1.0f : 0.0f);
            pw[a * 3 + b] = valid ? w32[a][b] : 0.0f;
        }
    }
    h_out[(size_t)i * 2] = valid ? h0 : 0.0f;
    h_out[(size_t)i * 2 + 1] = valid ? h1 : 0.0f;
    valid_out[i] = valid ? 1 : 0;
}

__global__ __launch_bounds__(EP_THREADS) void eye_pose_normalize_kernel(const int N, const float* __restrict__ pose, const int OH, const int OW,
                                                                        float* __restrict__ head_R, float* __restrict__ o_out,
                                                                        float* __restrict__ R_out, float* __restrict__ warp_out,
                                                                        float* __restrict__ h_out, uint8_t* __restrict__ valid_out) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * EP_THREADS + threadIdx.x;
    if (i >= 2LL * N) return;
    const int e = i >= N ? 1 : 0, n = (int)(i - (long long)e * N);
    double p[18];
    bool row_ok = true;
#pragma unroll
    for (int j = 0; j < 18; ++j) {
        p[j] = (double)pose[(size_t)n * 18 + j];
        row_ok = row_ok && finite64(p[j]);
    }
    const double fx = p[0], fy = p[1], cx = p[2], cy = p[3], f = p[16], dn = p[17];
    row_ok = row_ok && fx > 0.0 && fy > 0.0 && f > 0.0 && dn > 0.0;

    // 1. head_R (Rodrigues), rounded to float32
    double H[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    const double th = norm3(p[4], p[5], p[6]);
    if (finite64(p[4]) && finite64(p[5]) && finite64(p[6]) && th != 0.0) {
        const double k0 = p[4] / th, k1 = p[5] / th, k2 = p[6] / th;
        const double c = cos(th), s = sin(th);
        const double v = 1.0 - c;
        const double vk0 = v * k0, vk1 = v * k1, vk2 = v * k2, sk0 = s * k0, sk1 = s * k1, sk2 = s * k2;
        H[0][0] = c + vk0 * k0;   H[0][1] = vk0 * k1 - sk2; H[0][2] = vk0 * k2 + sk1;
        H[1][0] = vk1 * k0 + sk2; H[1][1] = c + vk1 * k1;   H[1][2] = vk1 * k2 - sk0;
        H[2][0] = vk2 * k0 - sk1; H[2][1] = vk2 * k1 + sk0; H[2][2] = c + vk2 * k2;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const float r = (float)H[a][b];
            if (e == 0) head_R[(size_t)n * 9 + a * 3 + b] = r;
            H[a][b] = (double)r;
        }

    const double tv[3] = {p[7], p[8], p[9]}, cl[3] = {p[10], p[11], p[12]}, cr[3] = {p[13], p[14], p[15]};
    eye_normalize_from_rt(i, e, H, tv, fx, fy, cx, cy, cl, cr, f, dn, row_ok, OH, OW, o_out, R_out, warp_out, h_out, valid_out);
}

// eve_eye_pose_normalize_rt: the same threads, head_R and head_t read instead of derived.  Frame n reads row n / T of `rows`.
__global__ __launch_bounds__(EP_THREADS) void eye_pose_normalize_rt_kernel(const int N, const int T, const float* __restrict__ rows, const int stride,
                                                                           const float* __restrict__ head_R, const float* __restrict__ head_t,
                                                                           const uint8_t* __restrict__ valid_in, const int OH, const int OW,
                                                                           float* __restrict__ o_out, float* __restrict__ R_out,
                                                                           float* __restrict__ warp_out, float* __restrict__ h_out,
                                                                           uint8_t* __restrict__ valid_out) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * EP_THREADS + threadIdx.x;
    if (i >= 2LL * N) return;
    const int e = i >= N ? 1 : 0, n = (int)(i - (long long)e * N);
    const float* row = rows + (size_t)(n / T) * stride;
    double p[12], H[3][3], tv[3];
    bool row_ok = valid_in == nullptr || valid_in[n] != 0;
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        p[j] = (double)row[j];
        row_ok = row_ok && finite64(p[j]);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            H[a][b] = (double)head_R[(size_t)n * 9 + a * 3 + b];
            row_ok = row_ok && finite64(H[a][b]);
        }
        tv[a] = (double)head_t[(size_t)n * 3 + a];
        row_ok = row_ok && finite64(tv[a]);
    }
    const double fx = p[0], fy = p[1], cx = p[2], cy = p[3], f = p[10], dn = p[11];
    row_ok = row_ok && fx > 0.0 && fy > 0.0 && f > 0.0 && dn > 0.0;
    const double cl[3] = {p[4], p[5], p[6]}, cr[3] = {p[7], p[8], p[9]};
    eye_normalize_from_rt(i, e, H, tv, fx, fy, cx, cy, cl, cr, f, dn, row_ok, OH, OW, o_out, R_out, warp_out, h_out, valid_out);
}

}  // namespace
}  // namespace eve

using namespace eve;

extern "C" int eve_eye_pose_normalize(long long N, const float* pose, int OH, int OW, float* head_R, float* o, float* R, float* warp, float* h,
                                      uint8_t* valid, eve_stream_t stream) {
    const char* why = nullptr;
    if (N <= 0 || OH <= 0 || OW <= 0 || !pose || !head_R || !o || !R || !warp || !h || !valid) why = "bad arguments";
    else if (OH > EP_MAX_PATCH || OW > EP_MAX_PATCH) why = "patch too large (OH and OW <= 4096)";
    else if (N > (long long)0x3fffffff) why = "2 N must fit 31 bits";
    if (why) {
        char msg[128];
        snprintf(msg, sizeof(msg), "eye_pose_normalize: %s", why);
        return set_error_msg(msg);
    }
    const dim3 grid((unsigned)((2 * N + EP_THREADS - 1) / EP_THREADS));
    EVE_LAUNCH("eye_pose_normalize_kernel", eye_pose_normalize_kernel, grid, dim3(EP_THREADS), 0, (hipStream_t)stream, (int)N, pose, OH, OW, head_R, o,
               R, warp, h, valid);
    EVE_CHECK_LAUNCH();
    return 0;
}

extern "C" int eve_eye_pose_normalize_rt(long long N, int frames_per_row, const float* rows, int row_stride, const float* head_R, const float* head_t,
                                         const uint8_t* valid_in, int OH, int OW, float* o, float* R, float* warp, float* h, uint8_t* valid,
                                         eve_stream_t stream) {
    const char* why = nullptr;
    if (N <= 0 || frames_per_row <= 0 || OH <= 0 || OW <= 0 || !rows || !head_R || !head_t || !o || !R || !warp || !h || !valid) why = "bad arguments";
    else if (row_stride < 12) why = "a row has at least 12 entries";
    else if (OH > EP_MAX_PATCH || OW > EP_MAX_PATCH) why = "patch too large (OH and OW <= 4096)";
    else if (N > (long long)0x3fffffff) why = "2 N must fit 31 bits";
    if (why) {
        char msg[128];
        snprintf(msg, sizeof(msg), "eye_pose_normalize_rt: %s", why);
        return set_error_msg(msg);
    }
    const dim3 grid((unsigned)((2 * N + EP_THREADS - 1) / EP_THREADS));
    EVE_LAUNCH("eye_pose_normalize_rt_kernel", eye_pose_normalize_rt_kernel, grid, dim3(EP_THREADS), 0, (hipStream_t)stream, (int)N, frames_per_row,
               rows, row_stride, head_R, head_t, valid_in, OH, OW, o, R, warp, h, valid);
    EVE_CHECK_LAUNCH();
    return 0;
}
