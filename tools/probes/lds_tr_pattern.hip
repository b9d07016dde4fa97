// LDS transposing-read probe: cycles per ds_read_b64_tr_b16 for the lane -> address maps of the eight-wave weight-gradient tiles
// (wgrad_wg8.h: 512-byte rows; wgrad_wg8_t128.h: 256-byte dy rows and 768-byte gathered x rows), with and without the XOR key of
// tr_key, next to a linear map.  One wave per workgroup and eight waves per workgroup.
//   hipcc --offload-arch=gfx950 -O3 -o lds_tr_pattern lds_tr_pattern.hip && ./lds_tr_pattern
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
constexpr int LDS_BYTES = 65536;
__global__ void probe(const int* __restrict__ offs, int npat, unsigned long long* out, u32x2* sink) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    for (int i = threadIdx.x; i < LDS_BYTES / 4; i += blockDim.x) ((uint32_t*)smem)[i] = i;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int p = 0; p < npat; ++p) {
        const uint32_t a = (uint32_t)(uintptr_t)smem + offs[p * 64 + lane];       // (host: every offset + 8 + 7 * 4096 <= LDS_BYTES)
        u32x2 acc = {0, 0};
        __syncthreads();
        const unsigned long long t0 = __builtin_readcyclecounter();
#pragma unroll 1
        for (int it = 0; it < 256; ++it) {
            u32x2 v0, v1, v2, v3, v4, v5, v6, v7;
            asm volatile("ds_read_b64_tr_b16 %0, %8\n\tds_read_b64_tr_b16 %1, %8 offset:4096\n\tds_read_b64_tr_b16 %2, %8 offset:8192\n\t"
                         "ds_read_b64_tr_b16 %3, %8 offset:12288\n\tds_read_b64_tr_b16 %4, %8 offset:16384\n\tds_read_b64_tr_b16 %5, %8 offset:20480\n\t"
                         "ds_read_b64_tr_b16 %6, %8 offset:24576\n\tds_read_b64_tr_b16 %7, %8 offset:28672\n\t"
                         "s_waitcnt lgkmcnt(0)"
                         : "=v"(v0), "=v"(v1), "=v"(v2), "=v"(v3), "=v"(v4), "=v"(v5), "=v"(v6), "=v"(v7) : "v"(a) : "memory");
            acc += v0 + v1 + v2 + v3 + v4 + v5 + v6 + v7;
        }
        const unsigned long long t1 = __builtin_readcyclecounter();
        if (threadIdx.x == 0) out[blockIdx.x * npat + p] = t1 - t0;
        if (acc.x == 0x12345678u) sink[0] = acc;
    }
}
static int key3(int row) { return (row & 1) | (((row >> 1) & 1) << 1) | (((row >> 3) & 1) << 2); }
// the fragment address of wgrad_wg8*.h: lane (t, g) reads 8 bytes of row 8 g + t / 4, 16-byte slot (2 tile + (t & 3) / 2) ^ (key << 1)
static int frag(int lane, int rowb, int tile, bool keyed) {
    const int t = lane & 15, g = lane >> 4, row = 8 * g + (t >> 2);
    const int slot = (2 * tile + ((t & 3) >> 1)) ^ (keyed ? key3(row) << 1 : 0);
    return row * rowb + slot * 16 + (t & 1) * 8;
}
int main() {
    const int NP = 7;
    const char* names[NP] = {"linear", "256B keyed", "256B plain", "768B keyed", "768B plain", "512B keyed", "512B plain"};
    int h[NP * 64];
    for (int l = 0; l < 64; ++l) {
        h[0 * 64 + l] = l * 8;
        h[1 * 64 + l] = frag(l, 256, 3, true);
        h[2 * 64 + l] = frag(l, 256, 3, false);
        h[3 * 64 + l] = frag(l, 768, 13, true);
        h[4 * 64 + l] = frag(l, 768, 13, false);
        h[5 * 64 + l] = frag(l, 512, 5, true);
        h[6 * 64 + l] = frag(l, 512, 5, false);
    }
    for (int i = 0; i < NP * 64; ++i)
        if (h[i] < 0 || h[i] + 8 + 7 * 4096 > LDS_BYTES) { printf("offset %d out of range\n", h[i]); return 1; }
    int* d; unsigned long long* o; u32x2* s;
    if (hipMalloc(&d, sizeof(h)) != hipSuccess || hipMalloc(&o, 8 * NP * 256) != hipSuccess || hipMalloc(&s, 64) != hipSuccess) return 1;
    hipMemcpy(d, h, sizeof(h), hipMemcpyHostToDevice);
    for (int threads : {64, 512}) {
        hipLaunchKernelGGL(probe, dim3(256), dim3(threads), LDS_BYTES, 0, d, NP, o, s);
        if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); return 1; }
        unsigned long long r[NP * 256];
        hipMemcpy(r, o, 8 * NP * 256, hipMemcpyDeviceToHost);
        printf("threads %4d:", threads);
        for (int p = 0; p < NP; ++p) printf("  %s %.1f", names[p], (double)r[p] / (256.0 * 8));
        printf("   (cycle-counter ticks per ds_read_b64_tr_b16, wave 0 of block 0)\n");
    }
    return 0;
}
