// Masked streaming steps (eve_amd/stream.py: EVEStream.step(eye_mask=..., skip_invalid_pose=...)): the plan that compacts every
// sequence's usable frames to the front of the chunk, and the row gather that applies it and undoes it.  No scan changes: the
// compacted sequences run through the ragged path (per-sequence device lengths) as they are.  Both entries are forward-only,
// launch on the caller's stream and neither allocate nor synchronise, so a masked step is captured into one hipGraph whose
// replays read the mask of the chunk at hand.
#include "common.h"

namespace eve {
namespace {

// ---------------------------------------------------------------------------------------------------
// eve_stream_mask_plan: one thread per sequence, a serial walk over its T frames (T is a chunk's frame count: tens at most, and
// one launch per step) -- no ballot, no prefix scan, nothing that depends on the wave size.  Sequences 0 .. 2B-1 are the eye
// sequences (s = side * B + b), 2B .. 3B-1 the frame sequences (stream b: usable iff either eye is).
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void stream_mask_plan_kernel(const int B, const int T, const uint8_t* __restrict__ mask,
                                                              const uint8_t* __restrict__ pose_valid,
                                                              const int* __restrict__ lengths, int* __restrict__ count,
                                                              int* __restrict__ perm, int* __restrict__ inv,
                                                              uint8_t* __restrict__ eye_valid, uint8_t* __restrict__ valid) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= 3 * B) return;
    const bool frames = s >= 2 * B;
    const int side = frames ? 0 : s / B, b = s - (frames ? 2 : side) * B;
    // lengths in the layout of a ragged step: stream b's count at b (its left eye) and at B + b (its right eye), clamped here
    const int len[2] = {lengths != nullptr ? min(max(lengths[b], 0), T) : T, lengths != nullptr ? min(max(lengths[B + b], 0), T) : T};
    const size_t row = (size_t)b * T;
    auto eye = [&](int t, int e) {
        const size_t i = (row + t) * 2 + e;
        return t < len[e] && (mask == nullptr || mask[i] != 0) && (pose_valid == nullptr || pose_valid[i] != 0);
    };
    auto usable = [&](int t) { return frames ? (eye(t, 0) || eye(t, 1)) : eye(t, side); };
    int n = 0;
    for (int t = 0; t < T; ++t) n += usable(t) ? 1 : 0;
    count[s] = n;
    int* p = perm + (size_t)s * T;
    int* q = inv + (size_t)s * T;
    int head = 0, tail = n;                                  // stable partition: the usable frames ascending, then the others
    for (int t = 0; t < T; ++t) {
        const bool u = usable(t);
        const int j = u ? head++ : tail++;
        p[j] = t;
        q[t] = j;
        if (frames)
            valid[row + t] = u ? 1 : 0;
        else
            eye_valid[(row + t) * 2 + side] = u ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------------------------------
// eve_stream_permute_rows: dst[s][j] = src[s][clamp(index[s][j], 0, T - 1)], bit copies of V-sized words; one row per blockIdx.x,
// gridDim.y blocks share a long row
// ---------------------------------------------------------------------------------------------------
template <typename V>
__global__ __launch_bounds__(256) void stream_permute_rows_kernel(const int T, const long long row_words, const long long frame_stride,
                                                                  const long long seq_stride, const char* __restrict__ src,
                                                                  char* __restrict__ dst, const int* __restrict__ index) {
    const long long r = blockIdx.x;                          // s * T + j
    const long long s = r / T;
    const int t = min(max(index[r], 0), T - 1);
    const V* a = reinterpret_cast<const V*>(src + (size_t)s * seq_stride + (size_t)t * frame_stride);
    V* d = reinterpret_cast<V*>(dst) + (size_t)r * row_words;
    for (long long i = (long long)blockIdx.y * 256 + threadIdx.x; i < row_words; i += (long long)gridDim.y * 256) d[i] = a[i];
}

}  // namespace
}  // namespace eve

using namespace eve;

extern "C" int eve_stream_mask_plan(int B, int T, const uint8_t* mask, const uint8_t* pose_valid, const int* lengths, int* count,
                                    int* perm, int* inv, uint8_t* eye_valid, uint8_t* valid, eve_stream_t stream) {
    if (!count || !perm || !inv || !eye_valid || !valid)
        return set_error_msg("stream_mask_plan: count, perm, inv, eye_valid and valid must not be NULL");
    if (B < 1 || B > (1 << 20)) return set_error_msg("stream_mask_plan: B must be in 1..2^20");
    if (T < 1 || (long long)3 * B * T > 0x7fffffffLL) return set_error_msg("stream_mask_plan: T must be >= 1 and 3 * B * T < 2^31");
    EVE_LAUNCH("stream_mask_plan_kernel", stream_mask_plan_kernel, dim3((unsigned)((3 * B + 63) / 64)), dim3(64), 0, (hipStream_t)stream,
               B, T, mask, pose_valid, lengths, count, perm, inv, eye_valid, valid);
    EVE_CHECK_LAUNCH();
    return 0;
}

extern "C" int eve_stream_permute_rows(int S, int T, long long row_bytes, long long frame_stride_bytes, long long seq_stride_bytes,
                                       const void* src, void* dst, const int* index, eve_stream_t stream) {
    if (!src || !dst || !index) return set_error_msg("stream_permute_rows: src, dst and index must not be NULL");
    if (T < 1) return set_error_msg("stream_permute_rows: T must be >= 1");
    if (S < 1 || (long long)S * T > 0x7fffffffLL) return set_error_msg("stream_permute_rows: S must be >= 1 and S * T < 2^31");
    if (row_bytes <= 0 || row_bytes % 4 != 0) return set_error_msg("stream_permute_rows: row_bytes must be a positive multiple of 4");
    if (frame_stride_bytes < row_bytes || seq_stride_bytes < row_bytes || frame_stride_bytes % 4 != 0 || seq_stride_bytes % 4 != 0 ||
        (reinterpret_cast<uintptr_t>(src) & 3) != 0 || (reinterpret_cast<uintptr_t>(dst) & 3) != 0)
        return set_error_msg("stream_permute_rows: bad arguments (strides >= row_bytes; strides and pointers multiples of 4 bytes)");
    {                                // a gather is never in place: a row written could be a row still to be read
        const char* a = (const char*)src;
        const char* b = (const char*)dst;
        const size_t na = (size_t)(S - 1) * seq_stride_bytes + (size_t)(T - 1) * frame_stride_bytes + row_bytes;
        const size_t nb = (size_t)S * T * row_bytes;
        if (a < b + nb && b < a + na) return set_error_msg("stream_permute_rows: src and dst overlap");
    }
    const bool vec = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | (uintptr_t)row_bytes |
                       (uintptr_t)frame_stride_bytes | (uintptr_t)seq_stride_bytes) & 15) == 0;
    const long long words = row_bytes / (vec ? 16 : 4);
    const long long by = (words + 255) / 256 < 8 ? (words + 255) / 256 : 8;
    const dim3 grid((unsigned)((long long)S * T), (unsigned)by);
    if (vec)
        EVE_LAUNCH("stream_permute_rows_kernel", stream_permute_rows_kernel<uint4>, grid, dim3(256), 0, (hipStream_t)stream, T, words,
                   frame_stride_bytes, seq_stride_bytes, (const char*)src, (char*)dst, index);
    else
        EVE_LAUNCH("stream_permute_rows_kernel", stream_permute_rows_kernel<uint32_t>, grid, dim3(256), 0, (hipStream_t)stream, T, words,
                   frame_stride_bytes, seq_stride_bytes, (const char*)src, (char*)dst, index);
    EVE_CHECK_LAUNCH();
    return 0;
}
