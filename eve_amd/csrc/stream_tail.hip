// Streaming inference (eve_amd/stream.py): the EyeNet tail forward with the GRU state carried in place, and the per-stream
// hand-over of every other carried recurrent state.  Both are forward-only and launch on the caller's stream; neither
// allocates or synchronises, so a whole streaming step can be captured into one hipGraph.
#include "common.h"

namespace eve {
namespace {

// ---------------------------------------------------------------------------------------------------
// eve_eye_tail_stream_fwd: one workgroup (384 threads = six waves) per sequence.  A chunk of Tc frames is processed in
// sub-chunks of TAIL_TS frames whose activations stay in LDS; every non-recurrent layer reads its weights once per
// sub-chunk (from L2 / MALL: 0.9 MB for the whole tail), the recurrence keeps column j of W_hh^T in thread j's registers
// as gru_scan_fwd128_kernel does.  All arithmetic is float32 FMA chains, k ascending.
// ---------------------------------------------------------------------------------------------------
constexpr int TAIL_TS = 16;                 // frames per sub-chunk
constexpr int TAIL_THREADS = 384;
constexpr int TAIL_H = 128, TAIL_H3 = 384, TAIL_F = 512;
constexpr int TAIL_LDB = 132;               // row stride of the 130-wide [fc | head pose] rows (and of 128-wide rows)
constexpr int TAIL_FPT = (TAIL_TS + 2) / 3; // frames per thread of a 128-wide layer (three groups of 128 columns)

// out[t][o] = act(b[o] + sum_{k < K} in[t][k] * W[k][o]), o < 128, t < nt; in / out in LDS.  The sum is taken in blocks of
// 64 products added into a running total (the blocked accumulation of the unfused linear_mm_kernel): a single chain over
// fc's 512 inputs ends up measurably further from the float64 evaluation than the layer-by-layer tail.
template <int ACT>
__device__ __forceinline__ void tail_lin128(const float* in, int ldi, int K, const float* __restrict__ W, const float* __restrict__ b,
                                            float* out, int ldo, int nt) {
    const int o = threadIdx.x & (TAIL_H - 1), g = threadIdx.x >> 7;
    float acc[TAIL_FPT];
#pragma unroll
    for (int i = 0; i < TAIL_FPT; ++i) acc[i] = 0.f;
#pragma unroll 1
    for (int k0 = 0; k0 < K; k0 += 64) {
        const int k1 = min(K, k0 + 64);
        float blk[TAIL_FPT];
#pragma unroll
        for (int i = 0; i < TAIL_FPT; ++i) blk[i] = 0.f;
#pragma unroll 16
        for (int k = k0; k < k1; ++k) {                 // (16 weight loads in flight: at Tc = 1 the layers are load-latency bound)
            const float w0 = W[(size_t)k * TAIL_H + o];
#pragma unroll
            for (int i = 0; i < TAIL_FPT; ++i) {
                const int t = g + 3 * i;
                if (t < nt) blk[i] = fmaf(in[t * ldi + k], w0, blk[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < TAIL_FPT; ++i) acc[i] += blk[i];
    }
    const float bo = b ? b[o] : 0.f;
#pragma unroll
    for (int i = 0; i < TAIL_FPT; ++i) {
        const int t = g + 3 * i;
        const float z = acc[i] + bo;
        if (t < nt) out[t * ldo + o] = ACT == EVE_ACT_NONE ? z : act_fwd(z, ACT);
    }
}

__global__ __launch_bounds__(TAIL_THREADS) void eye_tail_stream_fwd_kernel(
        const int T, const float* __restrict__ feats, const float* __restrict__ head_pose, const eve_eye_tail_weights w,
        float* __restrict__ h_state, const int* __restrict__ reset, const int* __restrict__ lengths, float* __restrict__ gaze,
        float* __restrict__ pupil, float* __restrict__ hs) {
    __shared__ __attribute__((aligned(16))) float X[TAIL_TS * TAIL_F];        // feats; later fc_common.0, GI, head hidden rows
    __shared__ __attribute__((aligned(16))) float Bf[TAIL_TS * TAIL_LDB];     // [fc | head pose]; fc_common.2; the GRU outputs
    __shared__ __attribute__((aligned(16))) float h[TAIL_H];
    __shared__ float gh[TAIL_H3];
    const int s = blockIdx.x, j = threadIdx.x;
    const bool zero = reset != nullptr && reset[s] != 0;
    // frames of this sequence that advance the carried state (eve_eye_tail_stream_fwd_len); every frame is still computed, the
    // ones from `len` on with h held at the state after frame len - 1, so the write-back below needs no second copy of h
    const int len = lengths != nullptr ? min(max(lengths[s], 0), T) : T;
    if (j < TAIL_H) h[j] = zero ? 0.f : h_state[(size_t)s * TAIL_H + j];
    const float bhh = w.hh_b[j];
    float wr[TAIL_H];                       // column j of W_hh^T, resident for the whole chunk (loaded per sub-chunk it spills)
#pragma unroll
    for (int k = 0; k < TAIL_H; ++k) wr[k] = w.hh_w[(size_t)k * TAIL_H3 + j];
    for (int t0 = 0; t0 < T; t0 += TAIL_TS) {
        const int nt = min(TAIL_TS, T - t0);
        const size_t row0 = (size_t)s * T + t0;                                // first (sequence, frame) row of the sub-chunk
        {
            const float4* src = reinterpret_cast<const float4*>(feats + row0 * TAIL_F);
            float4* dst = reinterpret_cast<float4*>(X);
            for (int i = j; i < nt * (TAIL_F / 4); i += TAIL_THREADS) dst[i] = src[i];
            if (j < 2 * nt) Bf[(j >> 1) * TAIL_LDB + TAIL_H + (j & 1)] = head_pose[row0 * 2 + j];
        }
        __syncthreads();
        tail_lin128<EVE_ACT_NONE>(X, TAIL_F, TAIL_F, w.fc_w, w.fc_b, Bf, TAIL_LDB, nt);              // cnn_layers.fc
        __syncthreads();
        tail_lin128<EVE_ACT_SELU>(Bf, TAIL_LDB, TAIL_H + 2, w.c0_w, w.c0_b, X, TAIL_F, nt);           // fc_common.0 + SELU
        __syncthreads();
        tail_lin128<EVE_ACT_NONE>(X, TAIL_F, TAIL_H, w.c2_w, w.c2_b, Bf, TAIL_LDB, nt);              // fc_common.2
        __syncthreads();
        {                                                                                             // GI = W_ih x + b_ih
            float acc[TAIL_TS];
            const float bo = w.ih_b[j];
#pragma unroll
            for (int t = 0; t < TAIL_TS; ++t) acc[t] = bo;
#pragma unroll 4
            for (int k = 0; k < TAIL_H; k += 4) {
                const float w0 = w.ih_w[(size_t)k * TAIL_H3 + j], w1 = w.ih_w[(size_t)(k + 1) * TAIL_H3 + j];
                const float w2 = w.ih_w[(size_t)(k + 2) * TAIL_H3 + j], w3 = w.ih_w[(size_t)(k + 3) * TAIL_H3 + j];
#pragma unroll
                for (int t = 0; t < TAIL_TS; ++t) {
                    if (t < nt) {
                        const float4 x = *reinterpret_cast<const float4*>(Bf + t * TAIL_LDB + k);
                        acc[t] = fmaf(x.x, w0, acc[t]); acc[t] = fmaf(x.y, w1, acc[t]);
                        acc[t] = fmaf(x.z, w2, acc[t]); acc[t] = fmaf(x.w, w3, acc[t]);
                    }
                }
            }
#pragma unroll
            for (int t = 0; t < TAIL_TS; ++t)
                if (t < nt) X[t * TAIL_F + j] = acc[t];
        }
        __syncthreads();
        {                                                                                             // the recurrence
            for (int t = 0; t < nt; ++t) {
                float a = bhh;
#pragma unroll
                for (int k = 0; k < TAIL_H; k += 4) {
                    const float4 hv = *reinterpret_cast<const float4*>(&h[k]);
                    a = fmaf(wr[k], hv.x, a); a = fmaf(wr[k + 1], hv.y, a); a = fmaf(wr[k + 2], hv.z, a); a = fmaf(wr[k + 3], hv.w, a);
                }
                gh[j] = a;
                __syncthreads();
                float hnew = 0.f;
                if (j < TAIL_H) {
                    const float* gi = X + t * TAIL_F;
                    const float r = sigmoid_exact(gi[j] + gh[j]);
                    const float z = sigmoid_exact(gi[TAIL_H + j] + gh[TAIL_H + j]);
                    const float n = tanhf(gi[2 * TAIL_H + j] + r * gh[2 * TAIL_H + j]);
                    hnew = (1.f - z) * n + z * h[j];
                    Bf[t * TAIL_LDB + j] = hnew;
                    if (hs) hs[(row0 + t) * TAIL_H + j] = hnew;
                }
                __syncthreads();
                if (j < TAIL_H && t0 + t < len) h[j] = hnew;
                __syncthreads();
            }
        }
        tail_lin128<EVE_ACT_SELU>(Bf, TAIL_LDB, TAIL_H, w.g0_w, w.g0_b, X, TAIL_F, nt);               // fc_to_gaze.0 + SELU
        tail_lin128<EVE_ACT_SELU>(Bf, TAIL_LDB, TAIL_H, w.p0_w, w.p0_b, X + TAIL_H, TAIL_F, nt);      // fc_to_pupil.0 + SELU
        __syncthreads();
        if (j < 3 * nt) {                                                                             // the 2 + 1 output columns
            const int t = j / 3, c = j - 3 * t;
            const float* x = X + t * TAIL_F + (c == 2 ? TAIL_H : 0);
            const float* W2 = c == 2 ? w.p2_w : w.g2_w + c;
            float a = c == 2 ? w.p2_b[0] : 0.f;
#pragma unroll 16
            for (int k = 0; k < TAIL_H; ++k) a = fmaf(x[k], W2[(size_t)k * 4], a);
            const size_t row = row0 + t;
            if (c == 2) pupil[row] = a > 0.f ? a : 0.f;
            else gaze[row * 2 + c] = 1.5707963267948966f * tanhf(a);
        }
        __syncthreads();
    }
    if (j < TAIL_H) h_state[(size_t)s * TAIL_H + j] = h[j];
}

// ---------------------------------------------------------------------------------------------------
// eve_stream_state_rows: dst[s] = reset[s] ? 0 : src[s], bit copies of 4- or 2-byte elements
// eve_stream_state_rows_at (lengths != nullptr): dst[s] = src[s][lengths[s] - 1], rows with lengths[s] <= 0 left as they are;
// the length is clamped to T, so no device value reads outside src
// ---------------------------------------------------------------------------------------------------
template <typename U>
__global__ __launch_bounds__(256) void stream_state_rows_kernel(const long long row_elems, const long long src_stride,
                                                                const long long dst_stride, const U* __restrict__ src,
                                                                U* __restrict__ dst, const int* __restrict__ reset) {
    const int s = blockIdx.y;
    const bool zero = reset != nullptr && reset[s] != 0;
    const U* a = src + (size_t)s * src_stride;
    U* b = dst + (size_t)s * dst_stride;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < row_elems; i += (long long)gridDim.x * 256)
        b[i] = zero ? U(0) : a[i];
}

template <typename U>
__global__ __launch_bounds__(256) void stream_state_rows_at_kernel(const int T, const long long row_elems, const long long frame_stride,
                                                                   const long long src_stride, const long long dst_stride,
                                                                   const U* __restrict__ src, U* __restrict__ dst,
                                                                   const int* __restrict__ lengths) {
    const int s = blockIdx.y;
    const int len = min(lengths[s], T);
    if (len <= 0) return;
    const U* a = src + (size_t)s * src_stride + (size_t)(len - 1) * frame_stride;
    U* b = dst + (size_t)s * dst_stride;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < row_elems; i += (long long)gridDim.x * 256) b[i] = a[i];
}

}  // namespace
}  // namespace eve

using namespace eve;

extern "C" int eve_eye_tail_stream_fwd_len(int S, int T, const float* feats, const float* head_pose, const eve_eye_tail_weights* weights,
                                           float* h, const int* reset, const int* lengths, float* gaze, float* pupil, float* hs,
                                           eve_stream_t stream) {
    if (S <= 0 || T <= 0 || S > 65535 || !feats || !head_pose || !weights || !h || !gaze || !pupil)
        return set_error_msg("eye_tail_stream_fwd: bad arguments");
    const eve_eye_tail_weights& w = *weights;
    if (!w.fc_w || !w.fc_b || !w.c0_w || !w.c0_b || !w.c2_w || !w.c2_b || !w.ih_w || !w.ih_b || !w.hh_w || !w.hh_b || !w.g0_w ||
        !w.g0_b || !w.g2_w || !w.p0_w || !w.p0_b || !w.p2_w || !w.p2_b)
        return set_error_msg("eye_tail_stream_fwd: a weight pointer is NULL");
    if ((reinterpret_cast<uintptr_t>(feats) & 15) != 0) return set_error_msg("eye_tail_stream_fwd: feats must be 16-byte aligned");
    EVE_LAUNCH("eye_tail_stream_fwd_kernel", eye_tail_stream_fwd_kernel, dim3(S), dim3(TAIL_THREADS), 0, (hipStream_t)stream, T, feats,
               head_pose, w, h, reset, lengths, gaze, pupil, hs);
    EVE_CHECK_LAUNCH();
    return 0;
}

extern "C" int eve_eye_tail_stream_fwd(int S, int T, const float* feats, const float* head_pose, const eve_eye_tail_weights* weights,
                                       float* h, const int* reset, float* gaze, float* pupil, float* hs, eve_stream_t stream) {
    return eve_eye_tail_stream_fwd_len(S, T, feats, head_pose, weights, h, reset, nullptr, gaze, pupil, hs, stream);
}

extern "C" int eve_stream_state_rows(int dtype, int S, long long row_elems, long long src_stride, long long dst_stride, const void* src,
                                     void* dst, const int* reset, eve_stream_t stream) {
    if (S <= 0 || S > 65535 || row_elems <= 0 || src_stride < row_elems || dst_stride < row_elems || !src || !dst)
        return set_error_msg("stream_state_rows: bad arguments (strides >= row_elems)");
    if (src != dst) {                // rows must not overlap partially: in place, or disjoint
        const char* a = (const char*)src;
        const char* b = (const char*)dst;
        const size_t es = dtype == EVE_DT_F32 ? 4 : 2;
        const size_t na = ((size_t)(S - 1) * src_stride + row_elems) * es, nb = ((size_t)(S - 1) * dst_stride + row_elems) * es;
        if (a < b + nb && b < a + na) return set_error_msg("stream_state_rows: src and dst overlap without being equal");
    }
    const long long blocks_x = (row_elems + 255) / 256 < 64 ? (row_elems + 255) / 256 : 64;
    const dim3 grid((unsigned)blocks_x, (unsigned)S);
    if (dtype == EVE_DT_F32)
        EVE_LAUNCH("stream_state_rows_kernel", stream_state_rows_kernel<uint32_t>, grid, dim3(256), 0, (hipStream_t)stream, row_elems,
                   src_stride, dst_stride, (const uint32_t*)src, (uint32_t*)dst, reset);
    else if (dtype == EVE_DT_BF16 || dtype == EVE_DT_F16)
        EVE_LAUNCH("stream_state_rows_kernel", stream_state_rows_kernel<uint16_t>, grid, dim3(256), 0, (hipStream_t)stream, row_elems,
                   src_stride, dst_stride, (const uint16_t*)src, (uint16_t*)dst, reset);
    else
        return set_error_msg("stream_state_rows: dtype must be f32, bf16 or f16");
    EVE_CHECK_LAUNCH();
    return 0;
}

extern "C" int eve_stream_state_rows_at(int dtype, int S, int T, long long row_elems, long long frame_stride, long long src_stride,
                                        long long dst_stride, const void* src, void* dst, const int* lengths, eve_stream_t stream) {
    if (!src || !dst || !lengths) return set_error_msg("stream_state_rows_at: src, dst and lengths must not be NULL");
    if (T < 1) return set_error_msg("stream_state_rows_at: T must be >= 1");
    if (S <= 0 || S > 65535 || row_elems <= 0 || frame_stride < row_elems || src_stride < row_elems || dst_stride < row_elems)
        return set_error_msg("stream_state_rows_at: bad arguments (strides >= row_elems)");
    if (dtype != EVE_DT_F32 && dtype != EVE_DT_BF16 && dtype != EVE_DT_F16)
        return set_error_msg("stream_state_rows_at: dtype must be f32, bf16 or f16");
    {                                // a commit is never in place: the S x T source frames and the S destination rows are disjoint
        const char* a = (const char*)src;
        const char* b = (const char*)dst;
        const size_t es = dtype == EVE_DT_F32 ? 4 : 2;
        const size_t na = ((size_t)(S - 1) * src_stride + (size_t)(T - 1) * frame_stride + row_elems) * es;
        const size_t nb = ((size_t)(S - 1) * dst_stride + row_elems) * es;
        if (a < b + nb && b < a + na) return set_error_msg("stream_state_rows_at: src and dst overlap");
    }
    const long long blocks_x = (row_elems + 255) / 256 < 64 ? (row_elems + 255) / 256 : 64;
    const dim3 grid((unsigned)blocks_x, (unsigned)S);
    if (dtype == EVE_DT_F32)
        EVE_LAUNCH("stream_state_rows_at_kernel", stream_state_rows_at_kernel<uint32_t>, grid, dim3(256), 0, (hipStream_t)stream, T,
                   row_elems, frame_stride, src_stride, dst_stride, (const uint32_t*)src, (uint32_t*)dst, lengths);
    else
        EVE_LAUNCH("stream_state_rows_at_kernel", stream_state_rows_at_kernel<uint16_t>, grid, dim3(256), 0, (hipStream_t)stream, T,
                   row_elems, frame_stride, src_stride, dst_stride, (const uint16_t*)src, (uint16_t*)dst, lengths);
    EVE_CHECK_LAUNCH();
    return 0;
}
