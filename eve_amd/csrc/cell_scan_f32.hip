// Clip-long scans of RefineNet's conv-RNN bottleneck cells in FLOAT32: CGRUCell (forward + backward), CRNNCell (forward +
// backward) and CLSTMCell (forward; training forward + backward) -- /root/reference/src/models/common.py:331-352 (CRNN),
// :355-385 (CLSTM), :388-415 (CGRU), applied per frame by refine_net.py:132-176.  One persistent launch walks all T frames of a
// clip; before round 5 the float32 parity mode and the CLSTM / CRNN cells ran T x (1-2 convolution launches + gate kernels +
// concatenations).  The reference never back-propagates through its CLSTM cell (refine_net.py:168-174 hands the cell's INPUT on):
// clstm_scan_f32_fwd_kernel serves that default.  The training forward and the backward exist for eve_amd's opt-in config key
// refine_net_clstm_feeds_features, which departs from the reference on purpose and makes the cell's h the bottleneck features.
//
// Geometry: 5 x 8 pixels (fixed by the model), C hidden + C input channels with C = refine_net_num_features in {32, 64, 128}
// as a template parameter (64 is the shipped configuration; its instantiations keep their pre-template kernel names and
// arithmetic order).  One workgroup (512 threads, 8 waves) per sequence.  In LDS, as floats: the zero-bordered 7 x 10 halo of
// the 2C-channel convolution input (pixel stride 2C + 4 floats so that the 16 pixels of a fragment read fall into different
// banks: 68, 132 and 260 are all 4 mod 64, and the halo row stride 10 x (2C + 4) is 40 mod 64 for all three, so the three
// widths have ONE bank pattern), the convolution output [40][<= 4C], and the state(s).
//   LDS per workgroup:  C = 32: 19 KB halo + 10 / 20 KB output;  C = 64: 36 KB + 20 / 40 KB;  C = 128: 71 KB + 40 KB (CGRU, CRNN)
//   or + 80 KB (CLSTM forward: 151 KB of the CU's 160 KB, all four gates of a frame in one piece; the CLSTM backward's data
//   gradient contracts the 4C gate channels as two K slices of 2C through the same halo, 71 + 40 KB).
// A convolution is an implicit GEMM on v_mfma_f32_16x16x4_f32 (exact float32: an fmaf chain) with A = filter rows (16 output
// channels x 4 k) straight from global memory / L2 as one 16-byte load per lane and 16-channel K block, B = 16 pixels x 4 k as
// one ds_read_b128 from the halo; the four words of a lane's vector feed four MFMAs (K permutation: MFMA s takes word s of every
// lane's vector; a sum is order-free, conv_igemm.hip uses the same trick), so a lane ends up with 4 consecutive output channels
// of one pixel.  The 40 pixels are 2.5 tiles of 16: the third tile's upper half re-reads pixel 39 and is dropped.
// Filter blocks are prefetched one K block ahead.  The matrix pipe runs float32 at the vector rate (157 TFLOP/s chip-wide), so
// at C = 64 a frame is MFMA-time bound at ~13 us (gates_1) + ~7 us (gate_2): the T-sequential floor of this formulation with
// 8 waves; the arithmetic of a frame goes with C^2.
//
// Weight / bias gradients are NOT formed here: like the 16-bit scan (cgru_scan.hip) the backward emits the gradients of the
// pre-activations for all frames and the caller runs ONE batched weight-gradient launch over the T*B frames.
#include "common.h"

namespace eve {

constexpr int CS_H = 5, CS_W = 8, CS_PIX = 40;
constexpr int CS_NT = 512;

// per-width constants: STR = floats per halo pixel (2C channels + 4: bank spread), HALO = the 7 x 10 halo in floats,
// NE = elements of a [40][C] plane a thread owns in the element-wise phases
template <int C>
struct CsGeom {
    static_assert(C == 32 || C == 64 || C == 128, "bottleneck width");
    static constexpr int STR = 2 * C + 4;
    static constexpr int HALO = 7 * 10 * STR;
    static constexpr int NE = (CS_PIX * C + CS_NT - 1) / CS_NT;
    static constexpr size_t lds_bytes(int out_ch) { return (size_t)(HALO + CS_PIX * out_ch) * sizeof(float); }
};

// halo offset (floats) of pixel p's centre
template <int STR>
__device__ __forceinline__ int cs_halo_at(int p) { return (((p >> 3) + 1) * 10 + (p & 7) + 1) * STR; }

// acc[nt][pt] += sum over K blocks kb in [kb0, kb1) of W[co][tap][ci] * halo[pixel + tap][ci]
//   W: [COUT][9][CIN] floats (OHWI for a forward convolution; IHWO with FLIP for a data gradient: out[p] takes dy[p - (tap - 1)])
//   a K block = 16 consecutive channels of one tap; kb = tap * (CIN / 16) + block
// 4 consecutive filter values as floats: one 16-byte load (float32 banks) or one 8-byte load (16-bit banks; exact in float32)
__device__ __forceinline__ float4 cs_ldw(const float* p) { return *reinterpret_cast<const float4*>(p); }
template <typename WT>
__device__ __forceinline__ float4 cs_ldw(const WT* p) {
    const uint2 q = *reinterpret_cast<const uint2*>(p);
    return make_float4(Elem<WT>::lo(q.x), Elem<WT>::hi(q.x), Elem<WT>::lo(q.y), Elem<WT>::hi(q.y));
}
// a value rounded to the storage format (identity for float32): the 16-bit instantiations round where cgru_scan1.hip does
template <typename S>
__device__ __forceinline__ float cs_rnd(float v) {
    if constexpr (sizeof(S) == 4) return v;
    else return Elem<S>::round(v);
}

// WCIN > CIN: the bank holds WCIN channels per tap and W points at the first of the CIN this call contracts (a K slice: the
// CLSTM data gradient's gate pairs); the halo holds those CIN channels alone
template <int STR, int CIN, int NTILE, bool FLIP, typename WT, int WCIN = CIN>
__device__ __forceinline__ void cs_conv(const float* halo, const WT* __restrict__ W, const int co0, const int kb0, const int kb1,
                                        f32x4_t (&acc)[NTILE][3], const int lane) {
    constexpr int KB_PER_TAP = CIN / 16;
    const int i = lane & 15, kk = lane >> 4;
    int boff[3];
#pragma unroll
    for (int pt = 0; pt < 3; ++pt) {
        const int p = min(pt * 16 + i, CS_PIX - 1);
        boff[pt] = (((p >> 3)) * 10 + (p & 7)) * STR + 4 * kk;             // + tap offset (dy * 10 + dx) * STR
    }
    const WT* wrow[NTILE];
#pragma unroll
    for (int nt = 0; nt < NTILE; ++nt) wrow[nt] = W + (size_t)(co0 + nt * 16 + i) * (9 * WCIN) + 4 * kk;
    auto wofs = [](const int kb) {                                         // floats from a filter row's start to K block kb
        if constexpr (WCIN == CIN) return kb * 16;
        else return (kb / KB_PER_TAP) * WCIN + (kb % KB_PER_TAP) * 16;
    };
    float4 a_next[NTILE];
#pragma unroll
    for (int nt = 0; nt < NTILE; ++nt) a_next[nt] = cs_ldw(wrow[nt] + wofs(kb0));
    auto step = [&](const int kb) {
        float4 a[NTILE];
#pragma unroll
        for (int nt = 0; nt < NTILE; ++nt) a[nt] = a_next[nt];
        const int kn = min(kb + 1, kb1 - 1);
#pragma unroll
        for (int nt = 0; nt < NTILE; ++nt) a_next[nt] = cs_ldw(wrow[nt] + wofs(kn));
        const int tap = kb / KB_PER_TAP, blk = kb - tap * KB_PER_TAP;
        const int kh = tap / 3, kw = tap - kh * 3;
        const int dy = FLIP ? 2 - kh : kh, dx = FLIP ? 2 - kw : kw;
        const int toff = (dy * 10 + dx) * STR + blk * 16;
        float4 b[3];
#pragma unroll
        for (int pt = 0; pt < 3; ++pt) b[pt] = *reinterpret_cast<const float4*>(halo + boff[pt] + toff);
#pragma unroll
        for (int nt = 0; nt < NTILE; ++nt)
#pragma unroll
            for (int pt = 0; pt < 3; ++pt) {
                acc[nt][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[nt].x, b[pt].x, acc[nt][pt], 0, 0, 0);
                acc[nt][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[nt].y, b[pt].y, acc[nt][pt], 0, 0, 0);
                acc[nt][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[nt].z, b[pt].z, acc[nt][pt], 0, 0, 0);
                acc[nt][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[nt].w, b[pt].w, acc[nt][pt], 0, 0, 0);
            }
    };
    // C = 32 (STR = 68): 9 or 18 K blocks per wave -- left to itself the compiler unrolls the whole loop, hoists every filter load
    // and spills; one block per iteration, like the longer loops of the wider instantiations
    if constexpr (STR == 68) {
#pragma unroll 1
        for (int kb = kb0; kb < kb1; ++kb) step(kb);
    } else {
        for (int kb = kb0; kb < kb1; ++kb) step(kb);
    }
}

// out[p][co0 + 16 nt + ..] (= or +=) acc (+ bias): lane holds channels co0 + 16 nt + 4 (lane / 16) + r of pixel 16 pt + lane % 16
template <int NTILE, bool ADD>
__device__ __forceinline__ void cs_store(float* out, const int ostr, const int co0, const float* __restrict__ bias,
                                         const f32x4_t (&acc)[NTILE][3], const int lane) {
    const int j = lane & 15, g = lane >> 4;
#pragma unroll
    for (int nt = 0; nt < NTILE; ++nt) {
        const int co = co0 + nt * 16 + 4 * g;
        float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (bias) bv = *reinterpret_cast<const float4*>(bias + co);
#pragma unroll
        for (int pt = 0; pt < 3; ++pt) {
            const int p = pt * 16 + j;
            if (p < CS_PIX) {
                float4* dst = reinterpret_cast<float4*>(out + p * ostr + co);
                float4 v = make_float4(acc[nt][pt][0] + bv.x, acc[nt][pt][1] + bv.y, acc[nt][pt][2] + bv.z, acc[nt][pt][3] + bv.w);
                if (ADD) { const float4 o = *dst; v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
                *dst = v;
            }
        }
    }
}

template <int NTILE>
__device__ __forceinline__ void cs_zero(f32x4_t (&acc)[NTILE][3]) {
#pragma unroll
    for (int nt = 0; nt < NTILE; ++nt)
#pragma unroll
        for (int pt = 0; pt < 3; ++pt) acc[nt][pt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
}

// A whole convolution of the workgroup's halo into out[40][ostr]:  COUT / 16 tiles over the 8 waves.
//   8 tiles or more (COUT = 128, 256, 512): COUT / 128 tiles per wave, each wave the whole K.
//   fewer (COUT = 64, 32): a tile belongs to 8 / tiles waves which split K evenly; part 0 stores (with the bias), parts 1..
//   add one after the other, a barrier between them (fixed order: the result does not depend on timing).
// ACC: the result is added to `out` (a second K slice of the same sum).
// Ends with a barrier: `out` is complete, the halo is free.
template <int STR, int CIN, int COUT, bool FLIP, typename WT, int WCIN = CIN, bool ACC = false>
__device__ __forceinline__ void cs_conv_all(const float* halo, const WT* __restrict__ W, const float* __restrict__ bias,
                                            float* out, const int ostr, const int wave, const int lane) {
    constexpr int KB = 9 * CIN / 16, TILES = COUT / 16;
    static_assert(COUT % 16 == 0 && CIN % 16 == 0 && (TILES % 8 == 0 || 8 % TILES == 0), "COUT");
    if constexpr (TILES >= 8) {
        constexpr int NT = TILES / 8;
        f32x4_t acc[NT][3];
        cs_zero<NT>(acc);
        cs_conv<STR, CIN, NT, FLIP, WT, WCIN>(halo, W, wave * 16 * NT, 0, KB, acc, lane);
        cs_store<NT, ACC>(out, ostr, wave * 16 * NT, bias, acc, lane);
    } else {
        constexpr int KS = 8 / TILES;                 // waves per tile
        static_assert(KB % KS == 0, "K split");
        const int tile = wave % TILES, part = wave / TILES;
        f32x4_t acc[1][3];
        cs_zero<1>(acc);
        cs_conv<STR, CIN, 1, FLIP, WT, WCIN>(halo, W, tile * 16, part * (KB / KS), (part + 1) * (KB / KS), acc, lane);
        if (part == 0) cs_store<1, ACC>(out, ostr, tile * 16, bias, acc, lane);
#pragma unroll
        for (int s = 1; s < KS; ++s) {
            __syncthreads();
            if (part == s) cs_store<1, true>(out, ostr, tile * 16, nullptr, acc, lane);
        }
    }
    __syncthreads();
}

template <int HALO>
__device__ __forceinline__ void cs_zero_halo(float* halo, const int tid) {
    for (int q = tid; q < HALO; q += CS_NT) halo[q] = 0.f;
}

// the NE elements a thread owns in every element-wise phase: e = tid + 512 k -> pixel e / C, channel e % C (C = 32: 2.5 per
// thread, the last half-round is masked).  Uses the kernel's `tid`, `C` and `G::NE`.
#define CS_FOR_ELEMS(k, p, c)                                         \
    _Pragma("unroll") for (int k = 0; k < G::NE; ++k)                 \
        if (const int p = (tid + CS_NT * k) / C, c = (tid + CS_NT * k) % C; (CS_PIX * C) % CS_NT == 0 || p < CS_PIX)

// ------------------------------------------------------------------------------------------------------------------------
// CGRU forward.  xs [B][T][40][C]; h0 [B][40][C] or null; w1 OHWI [2C][9][2C] (inputs: x then h), w2 OHWI [C][9][2C]
// (inputs: r*h then x).  Outputs: hs [B][T][40][C]; time-major hs_tm, rh, og [T][B][40][C], ru [T][B][40][2C].
// ------------------------------------------------------------------------------------------------------------------------
template <int C, typename S = float>
__global__ __launch_bounds__(CS_NT) void cgru_scan_f32_fwd_kernel(const int B, const int T, const S* __restrict__ xs,
                                                                  const S* __restrict__ h0, const S* __restrict__ w1,
                                                                  const float* __restrict__ b1, const S* __restrict__ w2,
                                                                  const float* __restrict__ b2, S* __restrict__ hs,
                                                                  S* __restrict__ hs_tm, S* __restrict__ ru,
                                                                  S* __restrict__ rh, S* __restrict__ og) {
    using G = CsGeom<C>;
    constexpr int STR = G::STR, C2 = 2 * C;
    extern __shared__ __attribute__((aligned(16))) float cs_lds[];
    float* halo = cs_lds;
    float* g = halo + G::HALO;                       // [40][2C]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x;
    cs_zero_halo<G::HALO>(halo, tid);
    float h[G::NE], x[G::NE], u[G::NE];
    CS_FOR_ELEMS(k, p, c) h[k] = h0 ? Elem<S>::ld(h0 + ((size_t)b * CS_PIX + p) * C + c) : 0.f;
    __syncthreads();
    for (int t = 0; t < T; ++t) {
        const S* xt = xs + ((size_t)b * T + t) * (CS_PIX * C);
        const size_t tm = ((size_t)t * B + b) * CS_PIX;
        CS_FOR_ELEMS(k, p, c) {
            x[k] = Elem<S>::ld(xt + p * C + c);
            halo[cs_halo_at<STR>(p) + c] = x[k];
            halo[cs_halo_at<STR>(p) + C + c] = h[k];
        }
        __syncthreads();
        cs_conv_all<STR, C2, C2, false>(halo, w1, b1, g, C2, wave, lane);
        CS_FOR_ELEMS(k, p, c) {
            const float r = cs_rnd<S>(sigmoid_exact(g[p * C2 + c]));       // (16-bit: the stored gate is the one every later stage sees)
            u[k] = cs_rnd<S>(sigmoid_exact(g[p * C2 + C + c]));
            const float v = cs_rnd<S>(r * h[k]);
            Elem<S>::st(ru + (tm + p) * C2 + c, r);
            Elem<S>::st(ru + (tm + p) * C2 + C + c, u[k]);
            Elem<S>::st(rh + (tm + p) * C + c, v);
            halo[cs_halo_at<STR>(p) + c] = v;
            halo[cs_halo_at<STR>(p) + C + c] = x[k];
        }
        __syncthreads();
        cs_conv_all<STR, C2, C, false>(halo, w2, b2, g, C2, wave, lane);
        CS_FOR_ELEMS(k, p, c) {
            const float o = cs_rnd<S>(tanhf(g[p * C2 + c]));
            h[k] = cs_rnd<S>((1.f - u[k]) * o + u[k] * h[k]);
            Elem<S>::st(og + (tm + p) * C + c, o);
            Elem<S>::st(hs_tm + (tm + p) * C + c, h[k]);
            Elem<S>::st(hs + (((size_t)b * T + t) * CS_PIX + p) * C + c, h[k]);
        }
        // (the next frame's halo writes follow conv_all's closing barrier; its reads of g precede the next conv's writes by the
        //  barrier after the halo fill)
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// CGRU backward (common.py:400-415 differentiated; the per-frame kernels are recurrent.hip's cgru_gates{2,1}_bwd).
// Time-major inputs dhs_tm, og, hs_tm [T][B][40][C], ru [T][B][40][2C]; w1t IHWO [2C][9][2C], w2t IHWO [2C][9][C].
// Outputs dg1_all [T][B][40][2C], dg2_all, dxs_tm [T][B][40][C], dh0 [B][40][C] or null.
// ------------------------------------------------------------------------------------------------------------------------
template <int C, typename S = float>
__global__ __launch_bounds__(CS_NT) void cgru_scan_f32_bwd_kernel(const int B, const int T, const S* __restrict__ dhs_tm,
                                                                  const S* __restrict__ ru, const S* __restrict__ og,
                                                                  const S* __restrict__ hs_tm, const S* __restrict__ h0,
                                                                  const S* __restrict__ w1t, const S* __restrict__ w2t,
                                                                  S* __restrict__ dg1_all, S* __restrict__ dg2_all,
                                                                  S* __restrict__ dxs_tm, S* __restrict__ dh0) {
    using G = CsGeom<C>;
    constexpr int STR = G::STR, C2 = 2 * C;
    extern __shared__ __attribute__((aligned(16))) float cs_lds[];
    float* halo = cs_lds;
    float* g = halo + G::HALO;                       // [40][2C]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x;
    cs_zero_halo<G::HALO>(halo, tid);
    float carry[G::NE], du[G::NE], dhd[G::NE], r[G::NE], u[G::NE], hp[G::NE], dx2[G::NE];
    CS_FOR_ELEMS(k, p, c) carry[k] = 0.f;
    __syncthreads();
    for (int t = T - 1; t >= 0; --t) {
        const size_t tm = ((size_t)t * B + b) * CS_PIX;
        CS_FOR_ELEMS(k, p, c) {
            const float d = Elem<S>::ld(dhs_tm + (tm + p) * C + c) + carry[k];
            r[k] = Elem<S>::ld(ru + (tm + p) * C2 + c);
            u[k] = Elem<S>::ld(ru + (tm + p) * C2 + C + c);
            const float o = Elem<S>::ld(og + (tm + p) * C + c);
            hp[k] = t > 0 ? Elem<S>::ld(hs_tm + (((size_t)(t - 1) * B + b) * CS_PIX + p) * C + c)
                          : (h0 ? Elem<S>::ld(h0 + ((size_t)b * CS_PIX + p) * C + c) : 0.f);
            const float a = cs_rnd<S>(d * (1.f - u[k]) * (1.f - o * o)); // d(pre-tanh); 16-bit: rounded before the data-gradient GEMM
            du[k] = d * (hp[k] - o);                                     // d(u), post-sigmoid
            dhd[k] = d * u[k];                                           // direct path to h
            Elem<S>::st(dg2_all + (tm + p) * C + c, a);
            halo[cs_halo_at<STR>(p) + c] = a;
        }
        __syncthreads();
        cs_conv_all<STR, C, C2, true>(halo, w2t, nullptr, g, C2, wave, lane);      // d[r*h | x]
        CS_FOR_ELEMS(k, p, c) {
            const float drh = g[p * C2 + c];
            dx2[k] = g[p * C2 + C + c];
            const float a = cs_rnd<S>(drh * hp[k] * r[k] * (1.f - r[k]));   // -> pre-sigmoid reset gate
            const float bq = cs_rnd<S>(du[k] * u[k] * (1.f - u[k]));        // -> pre-sigmoid update gate
            dhd[k] += drh * r[k];                                        // d(rh) -> h
            Elem<S>::st(dg1_all + (tm + p) * C2 + c, a);
            Elem<S>::st(dg1_all + (tm + p) * C2 + C + c, bq);
            halo[cs_halo_at<STR>(p) + c] = a;
            halo[cs_halo_at<STR>(p) + C + c] = bq;
        }
        __syncthreads();
        cs_conv_all<STR, C2, C2, true>(halo, w1t, nullptr, g, C2, wave, lane);     // d[x | h]
        CS_FOR_ELEMS(k, p, c) {
            Elem<S>::st(dxs_tm + (tm + p) * C + c, g[p * C2 + c] + dx2[k]);
            carry[k] = dhd[k] + g[p * C2 + C + c];
        }
        __syncthreads();                                                 // g is read above, written by the next frame's first conv
    }
    if (dh0) CS_FOR_ELEMS(k, p, c) Elem<S>::st(dh0 + ((size_t)b * CS_PIX + p) * C + c, carry[k]);
}

// ------------------------------------------------------------------------------------------------------------------------
// CRNN: h_t = tanh(conv([x_t | h_{t-1}]) + b)   (common.py:331-352).  w OHWI [C][9][2C]; wt IHWO [2C][9][C].
// forward: hs [B][T][40][C] (+ time-major copy hs_tm);  backward: dpre_all, dxs_tm [T][B][40][C], dh0.
// ------------------------------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(CS_NT) void crnn_scan_f32_fwd_kernel(const int B, const int T, const float* __restrict__ xs,
                                                                  const float* __restrict__ h0, const float* __restrict__ w,
                                                                  const float* __restrict__ bias, float* __restrict__ hs,
                                                                  float* __restrict__ hs_tm) {
    using G = CsGeom<C>;
    constexpr int STR = G::STR, C2 = 2 * C;
    extern __shared__ __attribute__((aligned(16))) float cs_lds[];
    float* halo = cs_lds;
    float* g = halo + G::HALO;                       // [40][C]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x;
    cs_zero_halo<G::HALO>(halo, tid);
    float h[G::NE];
    CS_FOR_ELEMS(k, p, c) h[k] = h0 ? h0[((size_t)b * CS_PIX + p) * C + c] : 0.f;
    __syncthreads();
    for (int t = 0; t < T; ++t) {
        const float* xt = xs + ((size_t)b * T + t) * (CS_PIX * C);
        CS_FOR_ELEMS(k, p, c) {
            halo[cs_halo_at<STR>(p) + c] = xt[p * C + c];
            halo[cs_halo_at<STR>(p) + C + c] = h[k];
        }
        __syncthreads();
        cs_conv_all<STR, C2, C, false>(halo, w, bias, g, C, wave, lane);
        CS_FOR_ELEMS(k, p, c) {
            h[k] = tanhf(g[p * C + c]);
            hs_tm[(((size_t)t * B + b) * CS_PIX + p) * C + c] = h[k];
            hs[(((size_t)b * T + t) * CS_PIX + p) * C + c] = h[k];
        }
    }
}

template <int C>
__global__ __launch_bounds__(CS_NT) void crnn_scan_f32_bwd_kernel(const int B, const int T, const float* __restrict__ dhs_tm,
                                                                  const float* __restrict__ hs_tm, const float* __restrict__ wt,
                                                                  float* __restrict__ dpre_all, float* __restrict__ dxs_tm,
                                                                  float* __restrict__ dh0) {
    using G = CsGeom<C>;
    constexpr int STR = G::STR, C2 = 2 * C;
    extern __shared__ __attribute__((aligned(16))) float cs_lds[];
    float* halo = cs_lds;
    float* g = halo + G::HALO;                       // [40][2C]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x;
    cs_zero_halo<G::HALO>(halo, tid);
    float carry[G::NE];
    CS_FOR_ELEMS(k, p, c) carry[k] = 0.f;
    __syncthreads();
    for (int t = T - 1; t >= 0; --t) {
        const size_t tm = ((size_t)t * B + b) * CS_PIX;
        CS_FOR_ELEMS(k, p, c) {
            const float hn = hs_tm[(tm + p) * C + c];
            const float a = (dhs_tm[(tm + p) * C + c] + carry[k]) * (1.f - hn * hn);
            dpre_all[(tm + p) * C + c] = a;
            halo[cs_halo_at<STR>(p) + c] = a;
        }
        __syncthreads();
        cs_conv_all<STR, C, C2, true>(halo, wt, nullptr, g, C2, wave, lane);       // d[x | h]
        CS_FOR_ELEMS(k, p, c) {
            dxs_tm[(tm + p) * C + c] = g[p * C2 + c];
            carry[k] = g[p * C2 + C + c];
        }
        __syncthreads();
    }
    if (dh0) CS_FOR_ELEMS(k, p, c) dh0[((size_t)b * CS_PIX + p) * C + c] = carry[k];
}

// ------------------------------------------------------------------------------------------------------------------------
// CLSTM (common.py:355-385; gate order in / forget / out / cell).  w OHWI [4C][9][2C]; wt IHWO [2C][9][4C].
// forward: hs, cs [B][T][40][C].  The training forward computes the same values in the same order and also writes what the
// backward reads, time-major: the post-activation gates [T][B][40][4C], cs_tm and hs_tm [T][B][40][C].
// backward: dpre_all [T][B][40][4C], dxs_tm [T][B][40][C], dh0 / dc0 [B][40][C].
// ------------------------------------------------------------------------------------------------------------------------
template <int C, bool TRAIN>
__device__ __forceinline__ void clstm_scan_f32_fwd_body(const int B, const int T, const float* __restrict__ xs,
                                                        const float* __restrict__ h0, const float* __restrict__ c0,
                                                        const float* __restrict__ w, const float* __restrict__ bias,
                                                        float* __restrict__ hs, float* __restrict__ cs,
                                                        float* __restrict__ gates_tm, float* __restrict__ cs_tm,
                                                        float* __restrict__ hs_tm) {
    using G = CsGeom<C>;
    constexpr int STR = G::STR, C2 = 2 * C, C4 = 4 * C;
    extern __shared__ __attribute__((aligned(16))) float cs_lds[];
    float* halo = cs_lds;
    float* g = halo + G::HALO;                       // [40][4C]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x;
    cs_zero_halo<G::HALO>(halo, tid);
    float h[G::NE], cc[G::NE];
    CS_FOR_ELEMS(k, p, c) {
        h[k] = h0 ? h0[((size_t)b * CS_PIX + p) * C + c] : 0.f;
        cc[k] = c0 ? c0[((size_t)b * CS_PIX + p) * C + c] : 0.f;
    }
    __syncthreads();
    for (int t = 0; t < T; ++t) {
        const float* xt = xs + ((size_t)b * T + t) * (CS_PIX * C);
        CS_FOR_ELEMS(k, p, c) {
            halo[cs_halo_at<STR>(p) + c] = xt[p * C + c];
            halo[cs_halo_at<STR>(p) + C + c] = h[k];
        }
        __syncthreads();
        cs_conv_all<STR, C2, C4, false>(halo, w, bias, g, C4, wave, lane);
        CS_FOR_ELEMS(k, p, c) {
            const float gi = g[p * C4 + c], gf = g[p * C4 + C + c], go = g[p * C4 + 2 * C + c], gc = g[p * C4 + 3 * C + c];
            const float si = sigmoid_exact(gi), sf = sigmoid_exact(gf), so = sigmoid_exact(go), tg = tanhf(gc);
            cc[k] = sf * cc[k] + si * tg;
            h[k] = so * tanhf(cc[k]);
            if constexpr (TRAIN) {
                const size_t tm = ((size_t)t * B + b) * CS_PIX + p;
                gates_tm[tm * C4 + c] = si;
                gates_tm[tm * C4 + C + c] = sf;
                gates_tm[tm * C4 + 2 * C + c] = so;
                gates_tm[tm * C4 + 3 * C + c] = tg;
                cs_tm[tm * C + c] = cc[k];
                hs_tm[tm * C + c] = h[k];
            }
            const size_t o = (((size_t)b * T + t) * CS_PIX + p) * C + c;
            hs[o] = h[k];
            cs[o] = cc[k];
        }
    }
}

template <int C>
__global__ __launch_bounds__(CS_NT) void clstm_scan_f32_fwd_kernel(const int B, const int T, const float* __restrict__ xs,
                                                                   const float* __restrict__ h0, const float* __restrict__ c0,
                                                                   const float* __restrict__ w, const float* __restrict__ bias,
                                                                   float* __restrict__ hs, float* __restrict__ cs) {
    clstm_scan_f32_fwd_body<C, false>(B, T, xs, h0, c0, w, bias, hs, cs, nullptr, nullptr, nullptr);
}

template <int C>
__global__ __launch_bounds__(CS_NT) void clstm_scan_f32_fwd_train_kernel(const int B, const int T, const float* __restrict__ xs,
                                                                         const float* __restrict__ h0, const float* __restrict__ c0,
                                                                         const float* __restrict__ w, const float* __restrict__ bias,
                                                                         float* __restrict__ hs, float* __restrict__ cs,
                                                                         float* __restrict__ gates_tm, float* __restrict__ cs_tm,
                                                                         float* __restrict__ hs_tm) {
    clstm_scan_f32_fwd_body<C, true>(B, T, xs, h0, c0, w, bias, hs, cs, gates_tm, cs_tm, hs_tm);
}

// Backward (common.py:376-385 differentiated; per frame: recurrent.hip's clstm_gates_bwd_kernel + the gate convolution's data
// gradient).  dhs_tm, cs_tm [T][B][40][C]; gates_tm [T][B][40][4C] post-activation; dcs_tm (gradient arriving at the stored cell
// states) or null.  The data gradient contracts 4C gate channels, whose halo would be 144 KB at C = 128: it runs as two K
// slices of 2C (in + forget, then out + cell) through the 2C-channel halo, the second added to the first in LDS.
template <int C>
__global__ __launch_bounds__(CS_NT) void clstm_scan_f32_bwd_kernel(const int B, const int T, const float* __restrict__ dhs_tm,
                                                                   const float* __restrict__ dcs_tm,
                                                                   const float* __restrict__ gates_tm,
                                                                   const float* __restrict__ cs_tm, const float* __restrict__ c0,
                                                                   const float* __restrict__ wt, float* __restrict__ dpre_all,
                                                                   float* __restrict__ dxs_tm, float* __restrict__ dh0,
                                                                   float* __restrict__ dc0) {
    using G = CsGeom<C>;
    constexpr int STR = G::STR, C2 = 2 * C, C4 = 4 * C;
    extern __shared__ __attribute__((aligned(16))) float cs_lds[];
    float* halo = cs_lds;
    float* g = halo + G::HALO;                       // [40][2C]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x;
    cs_zero_halo<G::HALO>(halo, tid);
    float carry_h[G::NE], carry_c[G::NE], dpo[G::NE], dpg[G::NE];
    CS_FOR_ELEMS(k, p, c) carry_h[k] = carry_c[k] = 0.f;
    __syncthreads();
    for (int t = T - 1; t >= 0; --t) {
        const size_t tm = ((size_t)t * B + b) * CS_PIX;
        CS_FOR_ELEMS(k, p, c) {
            const float* gt = gates_tm + (tm + p) * C4 + c;
            const float gi = gt[0], gf = gt[C], go = gt[2 * C], gg = gt[3 * C];
            const float cp = t > 0 ? cs_tm[(((size_t)(t - 1) * B + b) * CS_PIX + p) * C + c]
                                   : (c0 ? c0[((size_t)b * CS_PIX + p) * C + c] : 0.f);
            const float dh = dhs_tm[(tm + p) * C + c] + carry_h[k];
            const float tc = tanhf(cs_tm[(tm + p) * C + c]);
            float dc = carry_c[k] + dh * go * (1.f - tc * tc);
            if (dcs_tm) dc += dcs_tm[(tm + p) * C + c];
            const float dpi = dc * gg * gi * (1.f - gi), dpf = dc * cp * gf * (1.f - gf);
            dpo[k] = dh * tc * go * (1.f - go);
            dpg[k] = dc * gi * (1.f - gg * gg);
            carry_c[k] = dc * gf;
            float* dp = dpre_all + (tm + p) * C4 + c;
            dp[0] = dpi; dp[C] = dpf; dp[2 * C] = dpo[k]; dp[3 * C] = dpg[k];
            halo[cs_halo_at<STR>(p) + c] = dpi;
            halo[cs_halo_at<STR>(p) + C + c] = dpf;
        }
        __syncthreads();
        cs_conv_all<STR, C2, C2, true, float, C4, false>(halo, wt, nullptr, g, C2, wave, lane);          // d[x | h], in + forget
        CS_FOR_ELEMS(k, p, c) {
            halo[cs_halo_at<STR>(p) + c] = dpo[k];
            halo[cs_halo_at<STR>(p) + C + c] = dpg[k];
        }
        __syncthreads();
        cs_conv_all<STR, C2, C2, true, float, C4, true>(halo, wt + C2, nullptr, g, C2, wave, lane);      // += out + cell
        CS_FOR_ELEMS(k, p, c) {
            dxs_tm[(tm + p) * C + c] = g[p * C2 + c];
            carry_h[k] = g[p * C2 + C + c];
        }
        __syncthreads();                                                 // g is read above, written by the next frame's first conv
    }
    CS_FOR_ELEMS(k, p, c) {
        if (dh0) dh0[((size_t)b * CS_PIX + p) * C + c] = carry_h[k];
        if (dc0) dc0[((size_t)b * CS_PIX + p) * C + c] = carry_c[k];
    }
}

static_assert(CsGeom<128>::lds_bytes(4 * 128) <= (size_t)LDS_CU, "the CLSTM scan at C = 128 must fit a CU's LDS");
static_assert(CsGeom<128>::lds_bytes(2 * 128) <= (size_t)LDS_CU,
              "the CLSTM backward at C = 128 (2C-channel halo + [40][2C] data gradient; a 4C-channel halo alone is 144 KB) must fit");

// the name a width's instantiation reports through eve_last_kernel(): C = 64 keeps the name it had before the template
#define CS_KNAME(base) (C == 64 ? base : C == 32 ? base "<32>" : base "<128>")
// run `...` with the compile-time width bound to C; false for a width without an instantiation
#define CS_DISPATCH_C(width, ...)                                   \
    switch (width) {                                                \
        case 32: { constexpr int C = 32; __VA_ARGS__; } break;      \
        case 64: { constexpr int C = 64; __VA_ARGS__; } break;      \
        case 128: { constexpr int C = 128; __VA_ARGS__; } break;    \
        default: break;                                             \
    }

}  // namespace eve

using namespace eve;

bool eve_cell_scan_width_ok(int C) { return C == 32 || C == 64 || C == 128; }

/* float32 instantiations of eve_cgru_scan_fwd_c / _bwd_c (cgru_scan.hip dispatches here for EVE_DT_F32): same operands, float. */
int eve_cgru_scan_f32_fwd(int B, int T, int width, const float* xs, const float* h0, const float* w1, const float* b1, const float* w2,
                          const float* b2, float* hs, float* hs_tm, float* ru, float* rh, float* og, hipStream_t s) {
    if (!eve_cell_scan_width_ok(width)) return set_error_msg("cgru_scan_fwd: unsupported channel count (float32: 32, 64, 128)");
    CS_DISPATCH_C(width, EVE_LAUNCH(CS_KNAME("cgru_scan_f32_fwd_kernel"), cgru_scan_f32_fwd_kernel<C>, dim3(B), dim3(CS_NT),
                                    CsGeom<C>::lds_bytes(2 * C), s, B, T, xs, h0, w1, b1, w2, b2, hs, hs_tm, ru, rh, og));
    EVE_CHECK_LAUNCH();
    return 0;
}

int eve_cgru_scan_f32_bwd(int B, int T, int width, const float* dhs_tm, const float* ru, const float* og, const float* hs_tm,
                          const float* h0, const float* w1t, const float* w2t, float* dg1_all, float* dg2_all, float* dxs_tm, float* dh0,
                          hipStream_t s) {
    if (!eve_cell_scan_width_ok(width)) return set_error_msg("cgru_scan_bwd: unsupported channel count (float32: 32, 64, 128)");
    CS_DISPATCH_C(width, EVE_LAUNCH(CS_KNAME("cgru_scan_f32_bwd_kernel"), cgru_scan_f32_bwd_kernel<C>, dim3(B), dim3(CS_NT),
                                    CsGeom<C>::lds_bytes(2 * C), s, B, T, dhs_tm, ru, og, hs_tm, h0, w1t, w2t, dg1_all, dg2_all, dxs_tm,
                                    dh0));
    EVE_CHECK_LAUNCH();
    return 0;
}

/* bf16 / f16 storage at the widths the 16-bit MFMA kernels (cgru_scan.hip, cgru_scan1.hip: C = 64) do not serve: the float32
   scan with 16-bit operands and outputs, every value rounded to the format where cgru_scan1.hip rounds it (gates, r * h, the new
   state; in the backward the two pre-activation gradients before their data-gradient GEMMs), products on the float32 MFMA. */
#define CS_HNAME(base, w) (Elem<H>::IS_BF16 ? base "<" w ", eve::bf16_t>" : base "<" w ", eve::f16_t>")
int eve_cgru_scan_h16_fwd(int dtype, int B, int T, int width, const void* xs, const void* h0, const void* w1, const float* b1,
                          const void* w2, const float* b2, void* hs, void* hs_tm, void* ru, void* rh, void* og, hipStream_t s) {
    if (width != 32 && width != 128) return set_error_msg("cgru_scan_fwd: unsupported channel count (bf16 / f16: 32, 64, 128)");
#define CS_H16_FWD(W_, WS_)                                                                                                       \
    EVE_DISPATCH_H16(dtype, EVE_LAUNCH(CS_HNAME("cgru_scan_f32_fwd_kernel", WS_), (cgru_scan_f32_fwd_kernel<W_, H>), dim3(B), dim3(CS_NT), \
                                       CsGeom<W_>::lds_bytes(2 * W_), s, B, T, (const H*)xs, (const H*)h0, (const H*)w1, b1,     \
                                       (const H*)w2, b2, (H*)hs, (H*)hs_tm, (H*)ru, (H*)rh, (H*)og))
    if (width == 32) CS_H16_FWD(32, "32"); else CS_H16_FWD(128, "128");
#undef CS_H16_FWD
    EVE_CHECK_LAUNCH();
    return 0;
}

int eve_cgru_scan_h16_bwd(int dtype, int B, int T, int width, const void* dhs_tm, const void* ru, const void* og, const void* hs_tm,
                          const void* h0, const void* w1t, const void* w2t, void* dg1_all, void* dg2_all, void* dxs_tm, void* dh0,
                          hipStream_t s) {
    if (width != 32 && width != 128) return set_error_msg("cgru_scan_bwd: unsupported channel count (bf16 / f16: 32, 64, 128)");
#define CS_H16_BWD(W_, WS_)                                                                                                       \
    EVE_DISPATCH_H16(dtype, EVE_LAUNCH(CS_HNAME("cgru_scan_f32_bwd_kernel", WS_), (cgru_scan_f32_bwd_kernel<W_, H>), dim3(B), dim3(CS_NT), \
                                       CsGeom<W_>::lds_bytes(2 * W_), s, B, T, (const H*)dhs_tm, (const H*)ru, (const H*)og,     \
                                       (const H*)hs_tm, (const H*)h0, (const H*)w1t, (const H*)w2t, (H*)dg1_all, (H*)dg2_all,     \
                                       (H*)dxs_tm, (H*)dh0))
    if (width == 32) CS_H16_BWD(32, "32"); else CS_H16_BWD(128, "128");
#undef CS_H16_BWD
    EVE_CHECK_LAUNCH();
    return 0;
}

/* CRNNCell over a clip in one launch (float32; common.py:331-352).  xs [B][T][5][8][C], h0 [B][5][8][C] or NULL, w OHWI
   [C][3][3][2C] (input channels: x then h), bias [C].  Outputs hs [B][T][5][8][C] and the time-major copy hs_tm
   [T][B][5][8][C] the backward reads.  C in {32, 64, 128}. */
extern "C" int eve_crnn_scan_fwd_c(int B, int T, int C, const float* xs, const float* h0, const float* w, const float* bias, float* hs,
                                   float* hs_tm, eve_stream_t stream) {
    if (B <= 0 || T <= 0 || !xs || !w || !bias || !hs || !hs_tm) return set_error_msg("crnn_scan_fwd: bad arguments");
    if (!eve_cell_scan_width_ok(C)) return set_error_msg("crnn_scan_fwd: unsupported channel count (32, 64, 128)");
    const int width = C;
    CS_DISPATCH_C(width, EVE_LAUNCH(CS_KNAME("crnn_scan_f32_fwd_kernel"), crnn_scan_f32_fwd_kernel<C>, dim3(B), dim3(CS_NT),
                                    CsGeom<C>::lds_bytes(2 * C), (hipStream_t)stream, B, T, xs, h0, w, bias, hs, hs_tm));
    EVE_CHECK_LAUNCH();
    return 0;
}
extern "C" int eve_crnn_scan_fwd(int B, int T, const float* xs, const float* h0, const float* w, const float* bias, float* hs,
                                 float* hs_tm, eve_stream_t stream) {
    return eve_crnn_scan_fwd_c(B, T, 64, xs, h0, w, bias, hs, hs_tm, stream);
}

/* Backward of eve_crnn_scan_fwd_c.  Time-major dhs_tm, hs_tm [T][B][5][8][C]; wt = the filter bank IHWO [2C][3][3][C].
   Outputs (time-major): dpre_all = gradient of the pre-activation (what the batched weight / bias gradients read), dxs_tm;
   dh0 [B][5][8][C] or NULL. */
extern "C" int eve_crnn_scan_bwd_c(int B, int T, int C, const float* dhs_tm, const float* hs_tm, const float* wt, float* dpre_all,
                                   float* dxs_tm, float* dh0, eve_stream_t stream) {
    if (B <= 0 || T <= 0 || !dhs_tm || !hs_tm || !wt || !dpre_all || !dxs_tm) return set_error_msg("crnn_scan_bwd: bad arguments");
    if (!eve_cell_scan_width_ok(C)) return set_error_msg("crnn_scan_bwd: unsupported channel count (32, 64, 128)");
    const int width = C;
    CS_DISPATCH_C(width, EVE_LAUNCH(CS_KNAME("crnn_scan_f32_bwd_kernel"), crnn_scan_f32_bwd_kernel<C>, dim3(B), dim3(CS_NT),
                                    CsGeom<C>::lds_bytes(2 * C), (hipStream_t)stream, B, T, dhs_tm, hs_tm, wt, dpre_all, dxs_tm, dh0));
    EVE_CHECK_LAUNCH();
    return 0;
}
extern "C" int eve_crnn_scan_bwd(int B, int T, const float* dhs_tm, const float* hs_tm, const float* wt, float* dpre_all,
                                 float* dxs_tm, float* dh0, eve_stream_t stream) {
    return eve_crnn_scan_bwd_c(B, T, 64, dhs_tm, hs_tm, wt, dpre_all, dxs_tm, dh0, stream);
}

/* CLSTMCell over a clip in one launch (float32, forward only: the reference drops tuple states from the feature path,
   refine_net.py:168-174; common.py:355-385).  w OHWI [4C][3][3][2C] (gate order in / forget / out / cell), bias [4C];
   h0 / c0 [B][5][8][C] or NULL.  Outputs hs, cs [B][T][5][8][C].  C in {32, 64, 128}. */
extern "C" int eve_clstm_scan_fwd_c(int B, int T, int C, const float* xs, const float* h0, const float* c0, const float* w,
                                    const float* bias, float* hs, float* cs, eve_stream_t stream) {
    if (B <= 0 || T <= 0 || !xs || !w || !bias || !hs || !cs) return set_error_msg("clstm_scan_fwd: bad arguments");
    if (!eve_cell_scan_width_ok(C)) return set_error_msg("clstm_scan_fwd: unsupported channel count (32, 64, 128)");
    const int width = C;
    CS_DISPATCH_C(width, EVE_LAUNCH(CS_KNAME("clstm_scan_f32_fwd_kernel"), clstm_scan_f32_fwd_kernel<C>, dim3(B), dim3(CS_NT),
                                    CsGeom<C>::lds_bytes(4 * C), (hipStream_t)stream, B, T, xs, h0, c0, w, bias, hs, cs));
    EVE_CHECK_LAUNCH();
    return 0;
}
extern "C" int eve_clstm_scan_fwd(int B, int T, const float* xs, const float* h0, const float* c0, const float* w, const float* bias,
                                  float* hs, float* cs, eve_stream_t stream) {
    return eve_clstm_scan_fwd_c(B, T, 64, xs, h0, c0, w, bias, hs, cs, stream);
}

/* eve_clstm_scan_fwd_c for training: the same hs / cs, bit for bit, plus what eve_clstm_scan_bwd_c reads, time-major:
   gates_tm [T][B][5][8][4C] (sigmoid(in), sigmoid(forget), sigmoid(out), tanh(cell)), cs_tm and hs_tm [T][B][5][8][C]. */
extern "C" int eve_clstm_scan_fwd_train_c(int B, int T, int C, const float* xs, const float* h0, const float* c0, const float* w,
                                          const float* bias, float* hs, float* cs, float* gates_tm, float* cs_tm, float* hs_tm,
                                          eve_stream_t stream) {
    if (B <= 0 || T <= 0 || !xs || !w || !bias || !hs || !cs || !gates_tm || !cs_tm || !hs_tm)
        return set_error_msg("clstm_scan_fwd_train: bad arguments");
    if (!eve_cell_scan_width_ok(C)) return set_error_msg("clstm_scan_fwd_train: unsupported channel count (32, 64, 128)");
    const int width = C;
    CS_DISPATCH_C(width, EVE_LAUNCH(CS_KNAME("clstm_scan_f32_fwd_train_kernel"), clstm_scan_f32_fwd_train_kernel<C>, dim3(B), dim3(CS_NT),
                                    CsGeom<C>::lds_bytes(4 * C), (hipStream_t)stream, B, T, xs, h0, c0, w, bias, hs, cs, gates_tm, cs_tm,
                                    hs_tm));
    EVE_CHECK_LAUNCH();
    return 0;
}

/* Backward of eve_clstm_scan_fwd_train_c, one launch walking the frames last to first.  Time-major dhs_tm, cs_tm
   [T][B][5][8][C] and gates_tm [T][B][5][8][4C]; dcs_tm = gradient arriving at the stored cell states, or NULL; c0 as in the
   forward or NULL; wt = the filter bank IHWO [2C][3][3][4C].  Outputs (time-major): dpre_all [T][B][5][8][4C] = gradient of the
   gate pre-activations (what the batched weight / bias gradients read), dxs_tm [T][B][5][8][C]; dh0 / dc0 [B][5][8][C] or NULL. */
extern "C" int eve_clstm_scan_bwd_c(int B, int T, int C, const float* dhs_tm, const float* dcs_tm, const float* gates_tm,
                                    const float* cs_tm, const float* c0, const float* wt, float* dpre_all, float* dxs_tm, float* dh0,
                                    float* dc0, eve_stream_t stream) {
    if (B <= 0 || T <= 0 || !dhs_tm || !gates_tm || !cs_tm || !wt || !dpre_all || !dxs_tm)
        return set_error_msg("clstm_scan_bwd: bad arguments");
    if (!eve_cell_scan_width_ok(C)) return set_error_msg("clstm_scan_bwd: unsupported channel count (32, 64, 128)");
    const int width = C;
    CS_DISPATCH_C(width, EVE_LAUNCH(CS_KNAME("clstm_scan_f32_bwd_kernel"), clstm_scan_f32_bwd_kernel<C>, dim3(B), dim3(CS_NT),
                                    CsGeom<C>::lds_bytes(2 * C), (hipStream_t)stream, B, T, dhs_tm, dcs_tm, gates_tm, cs_tm, c0, wt,
                                    dpre_all, dxs_tm, dh0, dc0));
    EVE_CHECK_LAUNCH();
    return 0;
}
