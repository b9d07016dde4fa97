// Wide recurrent scans, gfx950: nn.GRUCell / nn.RNNCell / nn.LSTMCell over T steps for 256 < H <= 1024, H % 16 == 0
// (recurrent.hip serves H <= 256 with one workgroup per sequence and one thread per gate row; at H = 512 the recurrent
// matrix is 3-4 MB, no longer fits LDS, and that shape would pull it through a CU once per step per SEQUENCE).
//
// Shape: one persistent workgroup (8 waves) per tile of up to 16 sequences, all T steps inside the launch; the recurrence of
// a tile never leaves its workgroup, so there is no cross-workgroup synchronisation.  Per step the product
//     [16 sequences x K] . [K x N]        forward: K = H, N = G*H (whh_t);   backward: K = G*H, N = H (whh)
// runs on v_mfma_f32_16x16x4_f32 (exact float32: an fmaf chain).  Operand maps of that instruction: lane l = (r = l & 15,
// q = l >> 4) supplies A[row r][k = q] and B[k = q][col r]; the result has col = r, row = 4 q + reg.
//   * A (the tile's state, or the step's pre-activation gradients): lane (r, q) takes ONE 16-byte read per 16 k -- the
//     four values k = kb + 4 q + i, i = 0..3 -- and feeds value i to MFMA i of that k-block; B row kb + 4 q + i goes with it.
//   * B (the weights, streamed from L2 once per step per tile): a wave owns 64 consecutive output columns j0 .. j0 + 63 per
//     gate; column tile c (0..3) of the MFMA holds the columns j0 + 4 r + c, so lane (r, q) reads whh[k][j0 + 4 r .. + 3] as
//     one dwordx4 (16 lanes = 256 contiguous bytes per row) and the epilogue's loads and stores (gi, gates, hs, ...) are
//     dwordx4 over c as well.
//   * forward: hidden state of the tile in LDS as float32, double-buffered (a wave writes h_t while others still read
//     h_{t-1}): 2 x 16 x (H + 4) x 4 B = 128.5 KB at H = 1024; one barrier per step.  The LSTM cell state is only ever
//     touched by the lane that owns (sequence, j): it re-reads its own cs[t-1] store.
//   * backward: the carry dh (LSTM: and dc) in LDS.  Phase 1 (element-wise, all threads) turns dh + dhs into the
//     pre-activation gradients, stores them to their global outputs (dgi / dgh / dpre) and leaves the direct term (GRU:
//     d * z) in dh; phase 2 reads the rows just stored (same workgroup, behind a barrier; 16 x G*H floats are more than the
//     LDS holds beside the carry at H = 1024) as the A operand and adds whh^T . dpre into dh.
// Rows of a partial last tile are computed on zero state and not stored.  Weight and bias gradients are the caller's
// batched GEMMs over S*T, as for the narrow kernels.
#include "common.h"

namespace eve {

constexpr int WS_TILE = 16;        // sequences per workgroup = rows of the MFMA
constexpr int WS_THREADS = 512;
constexpr int WS_WAVES = WS_THREADS / 64;
constexpr int WS_PAD = 4;          // floats; LDS rows of H + 4: the 16 rows of one 16-byte read group start 4 banks apart

__device__ __forceinline__ f32x4_t ws_ld4(const float* p) { return *reinterpret_cast<const f32x4_t*>(p); }
__device__ __forceinline__ void ws_st4(float* p, f32x4_t v) { *reinterpret_cast<f32x4_t*>(p) = v; }
__device__ __forceinline__ f32x4_t ws_zero4() { return f32x4_t{0.f, 0.f, 0.f, 0.f}; }

// acc[c] += A(16 x 16 k) . B(16 k x columns j + c, c = 0..3): a = the lane's four A values, b[i] = row i of its B block
__device__ __forceinline__ void ws_mfma16(f32x4_t (&acc)[4], const f32x4_t a, const f32x4_t (&b)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[i].x, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[i].y, acc[1], 0, 0, 0);
        acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[i].z, acc[2], 0, 0, 0);
        acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[i].w, acc[3], 0, 0, 0);
    }
}

// G = 3 GRU (gates r, z, n; saves gates and hn_pre), 1 RNN (tanh), 4 LSTM (i, f, g, o; saves gates and cs).
// grid = ceil(S / 16), block = 512, dynamic LDS = 2 * 16 * (H + 4) floats.  whh_t [H][G*H].
template <int G>
__global__ __launch_bounds__(WS_THREADS) void scan_wide_fwd_kernel(int S, int T, int H, const float* __restrict__ gi,
                                                                   const float* __restrict__ whh_t, const float* __restrict__ bhh,
                                                                   const float* __restrict__ h0, const float* __restrict__ c0,
                                                                   float* __restrict__ hs, float* cs, float* __restrict__ gates,
                                                                   float* __restrict__ hn_pre) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int ld = H + WS_PAD, GH = G * H, H4 = H >> 2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int s0 = blockIdx.x * WS_TILE;
    for (int i = tid; i < WS_TILE * H4; i += WS_THREADS) {
        const int row = i / H4, c4 = (i - row * H4) * 4;
        f32x4_t v = ws_zero4();
        if (h0 && s0 + row < S) v = ws_ld4(h0 + (size_t)(s0 + row) * H + c4);
        ws_st4(sm + row * ld + c4, v);
    }
    __syncthreads();
    const int nsl = (H + 63) >> 6;
    for (int t = 0; t < T; ++t) {
        const float* hc = sm + (t & 1) * WS_TILE * ld;
        float* hn = sm + ((t & 1) ^ 1) * WS_TILE * ld;
        for (int sl = wave; sl < nsl; sl += WS_WAVES) {
            const int j0 = sl * 64 + 4 * r;                       // this lane's columns j0 .. j0 + 3 of every gate
            const bool jok = j0 < H;                              // H % 64 != 0: the last slice is ragged (in units of 16)
            f32x4_t acc[G][4];
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[g][c] = ws_zero4();
            const float* arow = hc + r * ld + 4 * q;
            const float* bcol = whh_t + (size_t)(4 * q) * GH + (jok ? j0 : 0);
            // the operands of k-block kb + 16 are in flight during the MFMAs of block kb (the last block re-reads itself)
            f32x4_t a = ws_ld4(arow), b[G][4];
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
                for (int i = 0; i < 4; ++i) b[g][i] = ws_ld4(bcol + (size_t)i * GH + g * H);
            for (int kb = 0; kb < H; kb += 16) {
                const int kn = min(kb + 16, H - 16);
                const f32x4_t an = ws_ld4(arow + kn);
                f32x4_t bn[G][4];
#pragma unroll
                for (int g = 0; g < G; ++g)
#pragma unroll
                    for (int i = 0; i < 4; ++i) bn[g][i] = ws_ld4(bcol + (size_t)(kn + i) * GH + g * H);
#pragma unroll
                for (int g = 0; g < G; ++g) ws_mfma16(acc[g], a, b[g]);
                a = an;
#pragma unroll
                for (int g = 0; g < G; ++g)
#pragma unroll
                    for (int i = 0; i < 4; ++i) b[g][i] = bn[g][i];
            }
            if (!jok) continue;
            f32x4_t bias[G];
#pragma unroll
            for (int g = 0; g < G; ++g) bias[g] = ws_ld4(bhh + g * H + j0);
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int seq = 4 * q + reg, s = s0 + seq;
                f32x4_t hnew = ws_zero4();
                if (s < S) {
                    const size_t o = (size_t)s * T + t;
                    f32x4_t pre[G];
#pragma unroll
                    for (int g = 0; g < G; ++g) {
                        pre[g] = ws_ld4(gi + o * GH + g * H + j0);
#pragma unroll
                        for (int c = 0; c < 4; ++c) pre[g][c] += (G == 3 ? 0.f : acc[g][c][reg] + bias[g][c]);
                    }
                    if (G == 1) {
#pragma unroll
                        for (int c = 0; c < 4; ++c) hnew[c] = tanhf(pre[0][c]);
                    } else if (G == 3) {
                        const f32x4_t hp = ws_ld4(hc + seq * ld + j0);
                        f32x4_t rg, zg, ng, ghn;
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            rg[c] = sigmoid_exact(pre[0][c] + (acc[0][c][reg] + bias[0][c]));
                            zg[c] = sigmoid_exact(pre[1][c] + (acc[1][c][reg] + bias[1][c]));
                            ghn[c] = acc[2][c][reg] + bias[2][c];
                            ng[c] = tanhf(pre[2][c] + rg[c] * ghn[c]);
                            hnew[c] = (1.f - zg[c]) * ng[c] + zg[c] * hp[c];
                        }
                        float* go = gates + o * GH + j0;
                        ws_st4(go, rg); ws_st4(go + H, zg); ws_st4(go + 2 * H, ng);
                        ws_st4(hn_pre + o * H + j0, ghn);
                    } else {
                        f32x4_t cp = ws_zero4();
                        if (t > 0) cp = ws_ld4(cs + (o - 1) * H + j0);             // this lane's own store of the step before
                        else if (c0) cp = ws_ld4(c0 + (size_t)s * H + j0);
                        f32x4_t ig, fg, gg, og, cn;
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            ig[c] = sigmoid_exact(pre[0][c]); fg[c] = sigmoid_exact(pre[1][c]);
                            gg[c] = tanhf(pre[2][c]); og[c] = sigmoid_exact(pre[3][c]);
                            cn[c] = fg[c] * cp[c] + ig[c] * gg[c];
                            hnew[c] = og[c] * tanhf(cn[c]);
                        }
                        float* go = gates + o * GH + j0;
                        ws_st4(go, ig); ws_st4(go + H, fg); ws_st4(go + 2 * H, gg); ws_st4(go + 3 * H, og);
                        ws_st4(cs + o * H + j0, cn);
                    }
                    ws_st4(hs + o * H + j0, hnew);
                }
                ws_st4(hn + seq * ld + j0, hnew);
            }
        }
        __syncthreads();
    }
}

// grid = ceil(S / 16), block = 512, dynamic LDS = (G == 4 ? 2 : 1) * 16 * (H + 4) floats.  whh [G*H][H].
// GRU: out_a = dgi, out_b = dgh (the A operand of phase 2);  RNN / LSTM: out_b = dpre (out_a unused).
template <int G>
__global__ __launch_bounds__(WS_THREADS) void scan_wide_bwd_kernel(int S, int T, int H, const float* __restrict__ dhs,
                                                                   const float* __restrict__ dcs, const float* __restrict__ whh,
                                                                   const float* __restrict__ h0, const float* __restrict__ c0,
                                                                   const float* __restrict__ hs, const float* __restrict__ cs,
                                                                   const float* __restrict__ gates, const float* __restrict__ hn_pre,
                                                                   float* __restrict__ out_a, float* out_b, float* __restrict__ dh0,
                                                                   float* __restrict__ dc0) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int ld = H + WS_PAD, GH = G * H, H4 = H >> 2;
    float* dh = sm;                         // [16][ld] carried gradient on h_t
    float* dc = sm + WS_TILE * ld;          // [16][ld] carried gradient on c_t (LSTM)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int s0 = blockIdx.x * WS_TILE;
    for (int i = tid; i < WS_TILE * H4; i += WS_THREADS) {
        const int row = i / H4, c4 = (i - row * H4) * 4;
        ws_st4(dh + row * ld + c4, ws_zero4());
        if (G == 4) ws_st4(dc + row * ld + c4, ws_zero4());
    }
    __syncthreads();
    const int nsl = (H + 63) >> 6;
    const bool aok = s0 + r < S;            // phase 2: rows of a partial tile are zero operands
    for (int t = T - 1; t >= 0; --t) {
        // phase 1: pre-activation gradients of step t, element-wise; thread-private (sequence, j) items
        for (int i = tid; i < WS_TILE * H4; i += WS_THREADS) {
            const int row = i / H4, c4 = (i - row * H4) * 4, s = s0 + row;
            if (s >= S) continue;
            const size_t o = (size_t)s * T + t;
            f32x4_t d = ws_ld4(dh + row * ld + c4) + ws_ld4(dhs + o * H + c4);
            f32x4_t carry = ws_zero4();
            if (G == 1) {
                const f32x4_t hv = ws_ld4(hs + o * H + c4);
                ws_st4(out_b + o * H + c4, d * (1.f - hv * hv));
            } else if (G == 3) {
                const float* g = gates + o * GH + c4;
                const f32x4_t rg = ws_ld4(g), zg = ws_ld4(g + H), ng = ws_ld4(g + 2 * H);
                f32x4_t hp = ws_zero4();
                if (t > 0) hp = ws_ld4(hs + (o - 1) * H + c4);
                else if (h0) hp = ws_ld4(h0 + (size_t)s * H + c4);
                const f32x4_t dn_pre = d * (1.f - zg) * (1.f - ng * ng);
                const f32x4_t dz_pre = d * (hp - ng) * zg * (1.f - zg);
                const f32x4_t dr_pre = dn_pre * ws_ld4(hn_pre + o * H + c4) * rg * (1.f - rg);
                float* ga = out_a + o * GH + c4;
                float* gb = out_b + o * GH + c4;
                ws_st4(ga, dr_pre); ws_st4(ga + H, dz_pre); ws_st4(ga + 2 * H, dn_pre);
                ws_st4(gb, dr_pre); ws_st4(gb + H, dz_pre); ws_st4(gb + 2 * H, dn_pre * rg);
                carry = d * zg;
            } else {
                const float* g = gates + o * GH + c4;
                const f32x4_t ig = ws_ld4(g), fg = ws_ld4(g + H), gg = ws_ld4(g + 2 * H), og = ws_ld4(g + 3 * H);
                const f32x4_t cv = ws_ld4(cs + o * H + c4);
                f32x4_t tc, cp = ws_zero4();
#pragma unroll
                for (int c = 0; c < 4; ++c) tc[c] = tanhf(cv[c]);
                if (t > 0) cp = ws_ld4(cs + (o - 1) * H + c4);
                else if (c0) cp = ws_ld4(c0 + (size_t)s * H + c4);
                f32x4_t dcv = ws_ld4(dc + row * ld + c4) + d * og * (1.f - tc * tc);
                if (dcs) dcv += ws_ld4(dcs + o * H + c4);
                float* gb = out_b + o * GH + c4;
                ws_st4(gb, dcv * gg * ig * (1.f - ig));
                ws_st4(gb + H, dcv * cp * fg * (1.f - fg));
                ws_st4(gb + 2 * H, dcv * ig * (1.f - gg * gg));
                ws_st4(gb + 3 * H, d * tc * og * (1.f - og));
                ws_st4(dc + row * ld + c4, dcv * fg);
            }
            ws_st4(dh + row * ld + c4, carry);
        }
        __syncthreads();                    // the rows of out_b stored above are this workgroup's A operand below
        // phase 2: dh[seq][j] += sum_k dpre[seq][k] * whh[k][j]
        const float* arow = out_b + ((size_t)(aok ? s0 + r : 0) * T + t) * GH + 4 * q;
        for (int sl = wave; sl < nsl; sl += WS_WAVES) {
            const int j0 = sl * 64 + 4 * r;
            const bool jok = j0 < H;
            f32x4_t acc[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = ws_zero4();
            const float* bcol = whh + (size_t)(4 * q) * H + (jok ? j0 : 0);
            f32x4_t a = ws_ld4(arow), b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) b[i] = ws_ld4(bcol + (size_t)i * H);
            for (int kb = 0; kb < GH; kb += 16) {
                const int kn = min(kb + 16, GH - 16);
                const f32x4_t an = ws_ld4(arow + kn);
                f32x4_t bn[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) bn[i] = ws_ld4(bcol + (size_t)(kn + i) * H);
                ws_mfma16(acc, aok ? a : ws_zero4(), b);
                a = an;
#pragma unroll
                for (int i = 0; i < 4; ++i) b[i] = bn[i];
            }
            if (!jok) continue;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                float* p = dh + (4 * q + reg) * ld + j0;
                ws_st4(p, ws_ld4(p) + f32x4_t{acc[0][reg], acc[1][reg], acc[2][reg], acc[3][reg]});
            }
        }
        __syncthreads();
    }
    for (int i = tid; i < WS_TILE * H4; i += WS_THREADS) {
        const int row = i / H4, c4 = (i - row * H4) * 4, s = s0 + row;
        if (s >= S) continue;
        if (dh0) ws_st4(dh0 + (size_t)s * H + c4, ws_ld4(dh + row * ld + c4));
        if (G == 4 && dc0) ws_st4(dc0 + (size_t)s * H + c4, ws_ld4(dc + row * ld + c4));
    }
}

static size_t ws_lds(int H, int buffers) { return (size_t)buffers * WS_TILE * (H + WS_PAD) * sizeof(float); }

bool scan_wide_ok(int H) { return H > 256 && H <= 1024 && H % 16 == 0; }

// gates / hn_pre (GRU), cs / gates (LSTM), c0 (LSTM) as the kernels above name them; unused ones are null
int scan_wide_fwd(int G, int S, int T, int H, const float* gi, const float* whh_t, const float* bhh, const float* h0, const float* c0,
                  float* hs, float* cs, float* gates, float* hn_pre, hipStream_t stream) {
    const dim3 grid((S + WS_TILE - 1) / WS_TILE), block(WS_THREADS);
    const size_t lds = ws_lds(H, 2);
    if (G == 1)
        EVE_LAUNCH("rnn_scan_wide_fwd_kernel", scan_wide_fwd_kernel<1>, grid, block, lds, stream, S, T, H, gi, whh_t, bhh, h0, c0, hs, cs,
                   gates, hn_pre);
    else if (G == 3)
        EVE_LAUNCH("gru_scan_wide_fwd_kernel", scan_wide_fwd_kernel<3>, grid, block, lds, stream, S, T, H, gi, whh_t, bhh, h0, c0, hs, cs,
                   gates, hn_pre);
    else
        EVE_LAUNCH("lstm_scan_wide_fwd_kernel", scan_wide_fwd_kernel<4>, grid, block, lds, stream, S, T, H, gi, whh_t, bhh, h0, c0, hs, cs,
                   gates, hn_pre);
    const hipError_t e = take_launch_error();
    return e == hipSuccess ? 0 : set_error(e, "scan_wide_fwd");
}

int scan_wide_bwd(int G, int S, int T, int H, const float* dhs, const float* dcs, const float* whh, const float* h0, const float* c0,
                  const float* hs, const float* cs, const float* gates, const float* hn_pre, float* out_a, float* out_b, float* dh0,
                  float* dc0, hipStream_t stream) {
    const dim3 grid((S + WS_TILE - 1) / WS_TILE), block(WS_THREADS);
    const size_t lds = ws_lds(H, G == 4 ? 2 : 1);
    if (G == 1)
        EVE_LAUNCH("rnn_scan_wide_bwd_kernel", scan_wide_bwd_kernel<1>, grid, block, lds, stream, S, T, H, dhs, dcs, whh, h0, c0, hs, cs,
                   gates, hn_pre, out_a, out_b, dh0, dc0);
    else if (G == 3)
        EVE_LAUNCH("gru_scan_wide_bwd_kernel", scan_wide_bwd_kernel<3>, grid, block, lds, stream, S, T, H, dhs, dcs, whh, h0, c0, hs, cs,
                   gates, hn_pre, out_a, out_b, dh0, dc0);
    else
        EVE_LAUNCH("lstm_scan_wide_bwd_kernel", scan_wide_bwd_kernel<4>, grid, block, lds, stream, S, T, H, dhs, dcs, whh, h0, c0, hs, cs,
                   gates, hn_pre, out_a, out_b, dh0, dc0);
    const hipError_t e = take_launch_error();
    return e == hipSuccess ? 0 : set_error(e, "scan_wide_bwd");
}

}  // namespace eve
