// Data gradient of the ResNet stem convolution (torchvision ResNet.conv1: 7x7 / stride 2 / pad 3, C -> 64, no bias;
// /root/reference/src/models/eye_net.py:48,106): the transposed convolution from d(conv1 out) back to the float patch.
//
//   dx[n][c][y][x] = sum_{co, ky, kx} dconv[n][oy][ox][co] * W[co][c][ky][kx],   y = 2 oy - 3 + ky,  x = 2 ox - 3 + kx
//
// As one GEMM per 2x2 block ("quad") of input pixels: pixels (2q + a, 2r + b), a, b in {0, 1}, all read the same 4x4
// window of dconv, rows q-1 .. q+2 and columns r-1 .. r+2, through taps ky = a + 5 - 2 wy, kx = b + 5 - 2 wx of window
// position (wy, wx); ky or kx = -1 is a zero tap.  So per quad
//   D[j][quad] = sum_k Wt[j][k] * A[k][quad],   k = (window position, co): K = 16 x 64 = 1024,
//   j = (2a + b) * 4 + c: N = 16 columns (parity x channel, channel padded to 4),
// which is exactly one v_mfma_f32_16x16x32_{bf16,f16} tile of 16 quads per 32 k-steps (v_mfma_f32_16x16x4_f32 in the
// float32 parity mode).  The filter is re-packed once per step (eve_stem_dgrad_pack) into the MFMA's A-operand order;
// in the 16-bit modes the whole 1024 x 16 matrix lives in 128 VGPRs of every wave, in float32 it is staged in LDS.
//
// A workgroup (4 waves) owns one image and a strip of 64 quads (the whole width of a 128-wide patch, half of a 256-wide
// one) and walks a band of quad rows top to bottom.  dconv rows are staged in a 4-row LDS ring (strip width + 3 halo
// columns, zero outside the image), the next row's global loads in flight during the current row's MFMAs.  Each wave's
// accumulator holds the 4 channels of one pixel per lane, so every store is a 128-byte row segment of the NCHW output:
// float32 straight from the accumulators, no 16-bit rounding and no unpack pass.
#include "common.h"
#include "lds_dma.h"

namespace eve {

constexpr int SD_QUADS = 64;                     // quads per strip (16 per wave)
constexpr int SD_COLS = SD_QUADS + 3;            // dconv columns per staged row: r0 - 1 .. r0 + 65
constexpr int SD_THREADS = 256;
constexpr int SD_KSTEPS16 = 32;                  // 16-bit: 16 window positions x 2 steps of 32 channels
constexpr int SD_KSTEPS32 = 256;                 // float32: 16 window positions x 16 steps of 4 channels

template <typename T> struct SdTraits {
    static constexpr int PIX_BYTES = 64 * (int)sizeof(T);                 // one dconv pixel, 64 channels
    static constexpr int CHUNKS = PIX_BYTES / 16;                         // 16-byte chunks per pixel: 8 (16-bit) / 16 (f32)
    static constexpr int ROW_BYTES = SD_COLS * PIX_BYTES;
    static constexpr int RING_BYTES = 4 * ROW_BYTES;
    static constexpr int LOADS = (SD_COLS * CHUNKS + SD_THREADS - 1) / SD_THREADS;   // 16-byte loads per thread per row
    static constexpr int W_LDS_BYTES = std::is_same<T, float>::value ? SD_KSTEPS32 * 64 * 4 : 0;
    static constexpr int LDS_BYTES = RING_BYTES + W_LDS_BYTES;
};

// Filter in the MFMA A-operand order.  Lane l of a step holds row j = l & 15 and lane group g = l >> 4; within window
// position p the lane group covers channels co = 16 g .. 16 g + 15 (32 contiguous bytes of a 16-bit pixel, 64 of a float
// one), which the A side of the product (the dconv fragment) reads from the same place:
//   16-bit  step s = 2 p + h, element e = 0..7:  co = 16 g + 8 h + e      -> packed[(s * 64 + l) * 8 + e]
//   float32 step s = 16 p + t:                   co = 16 g + t            -> packed[s * 64 + l]
__device__ __forceinline__ float sd_tap(const float* __restrict__ w, int C, int p, int co, int j) {
    const int c = j & 3, par = j >> 2, a = par >> 1, b = par & 1;
    const int ky = a + 5 - 2 * (p >> 2), kx = b + 5 - 2 * (p & 3);
    if (c >= C || ky < 0 || kx < 0) return 0.f;
    return w[((co * C + c) * 7 + ky) * 7 + kx];
}

template <typename T>
__global__ __launch_bounds__(256) void stem_dgrad_pack_kernel(const float* __restrict__ w, T* __restrict__ out, int C) {
    const int i = blockIdx.x * 256 + threadIdx.x;            // 1024 x 16 elements
    if (i >= 1024 * 16) return;
    int p, co, l;
    if constexpr (std::is_same<T, float>::value) {
        const int s = i >> 6;
        l = i & 63;
        p = s >> 4;
        co = 16 * (l >> 4) + (s & 15);
    } else {
        const int e = i & 7, s = i >> 9;
        l = (i >> 3) & 63;
        p = s >> 1;
        co = 16 * (l >> 4) + 8 * (s & 1) + e;
    }
    const float v = sd_tap(w, C, p, co, l & 15);
    if constexpr (std::is_same<T, float>::value) out[i] = v;
    else reinterpret_cast<uint16_t*>(out)[i] = Elem<T>::IS_BF16 ? (uint16_t)f32_to_bf16_bits(v) : (uint16_t)(pack2_f16(v, 0.f) & 0xffffu);
}

// One dconv row (all 64 channels of SD_COLS columns starting at gx0) into registers; zeros outside the image.
template <typename T>
__device__ __forceinline__ void sd_load_row(u32x4_t (&v)[SdTraits<T>::LOADS], const u32x4_t* __restrict__ src, int n, int oy,
                                            int OH, int OW, int gx0, int tid) {
    constexpr int CH = SdTraits<T>::CHUNKS;
    const bool row_ok = oy >= 0 && oy < OH;
#pragma unroll
    for (int i = 0; i < SdTraits<T>::LOADS; ++i) {
        const int id = tid + i * SD_THREADS;
        const int col = id / CH, ch = id % CH, gx = gx0 + col;
        u32x4_t q = {0u, 0u, 0u, 0u};
        if (row_ok && id < SD_COLS * CH && gx >= 0 && gx < OW) q = src[(((size_t)n * OH + oy) * OW + gx) * CH + ch];
        v[i] = q;
    }
}
// ... and into its ring slot.  The 16-byte chunk index is XORed with the column so that the 8 lanes of one ds_read_b128
// (consecutive columns, same chunk) fall on distinct banks.
template <typename T>
__device__ __forceinline__ void sd_store_row(char* slot, const u32x4_t (&v)[SdTraits<T>::LOADS], int tid) {
    constexpr int CH = SdTraits<T>::CHUNKS;
#pragma unroll
    for (int i = 0; i < SdTraits<T>::LOADS; ++i) {
        const int id = tid + i * SD_THREADS;
        if (id < SD_COLS * CH) {
            const int col = id / CH, ch = id % CH;
            *reinterpret_cast<u32x4_t*>(slot + col * SdTraits<T>::PIX_BYTES + ((ch ^ (col & (CH - 1))) << 4)) = v[i];
        }
    }
}
template <typename T>
__device__ __forceinline__ u32x4_t sd_lds_chunk(const char* slot, int col, int ch) {
    constexpr int CH = SdTraits<T>::CHUNKS;
    return *reinterpret_cast<const u32x4_t*>(slot + col * SdTraits<T>::PIX_BYTES + ((ch ^ (col & (CH - 1))) << 4));
}

// grid: (strips * bands, N); band_rows quad rows per band.
template <typename T>
__global__ __launch_bounds__(256) void stem_dgrad_kernel(const T* __restrict__ dconv, const T* __restrict__ wpk, float* __restrict__ dx,
                                                         int IH, int IW, int C, int nstrip, int band_rows) {
    using Tr = SdTraits<T>;
    constexpr bool F32 = std::is_same<T, float>::value;
    extern __shared__ __attribute__((aligned(16))) char sd_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = lane & 15, g = lane >> 4;
    const int n = blockIdx.y;
    const int strip = blockIdx.x % nstrip, band = blockIdx.x / nstrip;
    const int OH = IH >> 1, OW = IW >> 1;                   // dconv (= conv1 output) size; also the quad grid's
    const int r0 = strip * SD_QUADS;
    const int q0 = band * band_rows;
    const int q1 = min(q0 + band_rows, OH);
    const u32x4_t* src = reinterpret_cast<const u32x4_t*>(dconv);
    char* ring = sd_lds;
    auto slot = [&](int oy) { return ring + ((oy + 1) & 3) * Tr::ROW_BYTES; };

    // filter: 16-bit -> registers (32 fragments), float32 -> LDS behind the ring
    u32x4_t wreg[F32 ? 1 : SD_KSTEPS16];
    if constexpr (F32) {
        const u32x4_t* w4 = reinterpret_cast<const u32x4_t*>(wpk);
        u32x4_t* wl = reinterpret_cast<u32x4_t*>(sd_lds + Tr::RING_BYTES);
        for (int i = tid; i < SD_KSTEPS32 * 64 / 4; i += SD_THREADS) wl[i] = w4[i];
    } else {
        const u32x4_t* w4 = reinterpret_cast<const u32x4_t*>(wpk);
#pragma unroll
        for (int s = 0; s < SD_KSTEPS16; ++s) wreg[s] = w4[s * 64 + lane];
    }

    u32x4_t nxt[Tr::LOADS];
    for (int oy = q0 - 1; oy <= q0 + 1; ++oy) {
        sd_load_row<T>(nxt, src, n, oy, OH, OW, r0 - 1, tid);
        sd_store_row<T>(slot(oy), nxt, tid);
    }
    sd_load_row<T>(nxt, src, n, q0 + 2, OH, OW, r0 - 1, tid);

    const int col0 = wave * 16 + m;                          // this lane's quad, as a ring column (window column wx adds wx)
    const int x = 2 * (r0 + col0) + (g & 1);                 // output pixel of this lane: column ...
    const int a = g >> 1;                                    // ... and row 2 q + a
    const size_t plane = (size_t)IH * IW;
    float* dxn = dx + (size_t)n * C * plane;
    for (int q = q0; q < q1; ++q) {
        sd_store_row<T>(slot(q + 2), nxt, tid);
        __syncthreads();
        if (q + 1 < q1) sd_load_row<T>(nxt, src, n, q + 3, OH, OW, r0 - 1, tid);
        f32x4_t acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int wy = 0; wy < 4; ++wy) {
            const char* sl = slot(q - 1 + wy);
#pragma unroll
            for (int wx = 0; wx < 4; ++wx) {
                const int p = wy * 4 + wx, col = col0 + wx;
                if constexpr (F32) {
                    const float* wl = reinterpret_cast<const float*>(sd_lds + Tr::RING_BYTES);
#pragma unroll
                    for (int cc = 0; cc < 4; ++cc) {
                        const f32x4_t v = __builtin_bit_cast(f32x4_t, sd_lds_chunk<T>(sl, col, 4 * g + cc));
                        const int s = 16 * p + 4 * cc;
                        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wl[s * 64 + lane], v.x, acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wl[(s + 1) * 64 + lane], v.y, acc1, 0, 0, 0);
                        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wl[(s + 2) * 64 + lane], v.z, acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wl[(s + 3) * 64 + lane], v.w, acc1, 0, 0, 0);
                    }
                } else {
                    mfma16<T>(acc0, wreg[2 * p], sd_lds_chunk<T>(sl, col, 2 * g));
                    mfma16<T>(acc1, wreg[2 * p + 1], sd_lds_chunk<T>(sl, col, 2 * g + 1));
                }
            }
        }
        // D[j][quad]: lane (m, g) holds rows j = 4 g + i -- parity (a, b) = (g >> 1, g & 1), channel c = i -- of quad m
        if (x < IW) {
            float* row = dxn + (size_t)(2 * q + a) * IW + x;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < C) row[(size_t)c * plane] = acc0[c] + acc1[c];
        }
        __syncthreads();
    }
}

template <typename T>
static int stem_dgrad_launch(int N, int IH, int IW, int C, const void* dconv, const void* w_packed, float* dx, hipStream_t stream) {
    using Tr = SdTraits<T>;
    const int OH = IH / 2, OW = IW / 2;
    const int nstrip = (OW + SD_QUADS - 1) / SD_QUADS;
    // enough workgroups to fill the machine at small batches; whole columns of quads per workgroup at training batch sizes
    int bands = (2048 + N * nstrip - 1) / (N * nstrip);
    const int max_bands = OH >= 8 ? OH / 8 : 1;
    if (bands > max_bands) bands = max_bands;
    if (bands < 1) bands = 1;
    const int band_rows = (OH + bands - 1) / bands;
    bands = (OH + band_rows - 1) / band_rows;
    EVE_LAUNCH("stem_dgrad_kernel", stem_dgrad_kernel<T>, dim3((unsigned)(nstrip * bands), (unsigned)N), dim3(SD_THREADS),
               Tr::LDS_BYTES, stream, (const T*)dconv, (const T*)w_packed, dx, IH, IW, C, nstrip, band_rows);
    EVE_CHECK_LAUNCH();
    return 0;
}

}  // namespace eve

using namespace eve;

extern "C" int eve_stem_dgrad_pack(int dtype, int C, const float* w_oihw, void* w_packed, eve_stream_t stream) {
    if (dtype < EVE_DT_F32 || dtype > EVE_DT_F16 || C < 1 || C > 4 || !w_oihw || !w_packed)
        return set_error_msg("stem_dgrad_pack: bad arguments");
    const dim3 grid(1024 * 16 / 256), block(256);
    if (dtype == EVE_DT_F32)
        hipLaunchKernelGGL(stem_dgrad_pack_kernel<float>, grid, block, 0, (hipStream_t)stream, w_oihw, (float*)w_packed, C);
    else
        EVE_DISPATCH_H16(dtype, hipLaunchKernelGGL(stem_dgrad_pack_kernel<H>, grid, block, 0, (hipStream_t)stream, w_oihw, (H*)w_packed, C));
    EVE_CHECK_LAUNCH();
    return 0;
}

extern "C" int eve_stem_dgrad(int dtype, int N, int IH, int IW, int C, const void* dconv, const void* w_packed, float* dx_nchw,
                              eve_stream_t stream) {
    if (dtype < EVE_DT_F32 || dtype > EVE_DT_F16 || N < 1 || N > 65535 || IH < 2 || IW < 2 || (IH & 1) || (IW & 1) || C < 1 || C > 4 ||
        !dconv || !w_packed || !dx_nchw)
        return set_error_msg("stem_dgrad: bad arguments (N in 1..65535, IH and IW even, C in 1..4)");
    if (((uintptr_t)dconv & 15) || ((uintptr_t)w_packed & 15)) return set_error_msg("stem_dgrad: dconv / w_packed must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (dtype == EVE_DT_F32) return stem_dgrad_launch<float>(N, IH, IW, C, dconv, w_packed, dx_nchw, s);
    if (dtype == EVE_DT_BF16) return stem_dgrad_launch<bf16_t>(N, IH, IW, C, dconv, w_packed, dx_nchw, s);
    return stem_dgrad_launch<f16_t>(N, IH, IW, C, dconv, w_packed, dx_nchw, s);
}
