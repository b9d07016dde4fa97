/* eve_hip.h -- C ABI of libeve_hip.so: the MI355X (gfx950) kernels behind the EVE hot path
 * (EyeNet encoder + RefineNet point-of-gaze refiner, /root/reference/src/models/).
 *
 * The reference has no native layer (it is 100% PyTorch); what each entry point replaces is
 * therefore an ATen op site inside the reference's Python modules, cited per function as
 * `file:line` relative to /root/reference.  A binding (ctypes / cffi / a torch extension) passes
 *   - raw DEVICE pointers (activations NHWC, element type selected by `dtype`),
 *   - explicit shapes,
 *   - the HIP stream to launch on (a hipStream_t passed as void*; NULL = the null stream).
 * No entry point allocates, synchronises the device, or keeps state between calls (the one process-wide
 * object is the read-mostly kernel-selection table, eve_dispatch_config below).  Every function
 * returns 0 on success and a non-zero code on failure; eve_last_error() returns a thread-local
 * message for the last failure.  The Python side (eve_amd/_lib.py) raises RuntimeError from it.
 *
 * Layout conventions
 *   activations   [N][H][W][C]   (NHWC), C a multiple of 4 (f32) / 8 (bf16): 16-byte channel vectors
 *   conv weights  forward : [Cout][KH][KW][Cin]  ("OHWI", K = KH*KW*Cin contiguous per output channel)
 *                 dgrad   : [Cin][KH][KW][Cout]  ("IHWO")
 *   statistics    float [N][C][2] = (mean, rstd) per instance-norm plane
 *   weight / bias / affine gradients are always float and are ACCUMULATED into (caller zeroes them)
 */
#ifndef EVE_HIP_H_
#define EVE_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EVE_ABI_VERSION 10

typedef void* eve_stream_t; /* hipStream_t */

enum { EVE_DT_F32 = 0, EVE_DT_BF16 = 1, EVE_DT_F16 = 2 };   /* F16: IEEE half, the second 16-bit instantiation */
enum {
    EVE_ACT_NONE = 0,
    EVE_ACT_RELU = 1,    /* nn.ReLU          (eye_net trunk; refine_net.py:38 encoder blocks)   */
    EVE_ACT_LEAKY = 2,   /* nn.LeakyReLU(.01) (refine_net.py:108,113,221)                        */
    EVE_ACT_SELU = 3,    /* nn.SELU          (eye_net.py:54,77,83,89)                            */
    EVE_ACT_TANH = 4,    /* nn.Tanh / torch.tanh (eye_net.py:85; common.py:351,380,413)          */
    EVE_ACT_SIGMOID = 5  /* nn.Sigmoid / torch.sigmoid (refine_net.py:223; common.py:377-379,410) */
};

int eve_abi_version(void);
/* Symbol (without namespace / signature) of the kernel the last conv / stem call of this thread launched; lets a
 * profiler attribute a timed launch to the row of the same name in a rocprofv3 kernel summary.            */
const char* eve_last_kernel(void);
const char* eve_last_error(void);
/* Kernel selection (ABI v6).  Which kernel an entry point dispatches for a given shape is a pure function of the shape and
 * of THIS structure.  It is filled ONCE, when the library is loaded: built-in defaults, overridden by the EVE_* environment
 * variables named per field (tuning experiments; nothing on a call path reads the environment).  A test harness prints
 * eve_get_dispatch_config() and asserts it equals eve_get_default_dispatch_config() before it makes a parity claim
 * (tests/conftest.py), and forces a variant -- e.g. the four-wave convolution next to the eight-wave one -- with
 * eve_set_dispatch_config(), never through the environment of a running process.                                        */
typedef struct eve_dispatch_config {
    int struct_bytes;              /* sizeof(eve_dispatch_config): ABI guard                                              */
    int conv_impl_v1;              /* EVE_CONV_IMPL=v1      0   first-generation register-staged igemm / wgrad kernels     */
    int conv_tile_big;             /* EVE_CONV_TILE=2       0   256 x 128 per-tap tiles                                    */
    int conv_halo;                 /* EVE_CONV_HALO         1   halo-resident 3x3 kernels (conv_fast.h)                    */
    int conv_ws64;                 /* EVE_CONV_WS64         1   conv3x3_ws64_kernel for 32 x 32 x 64 -> 64                 */
    int conv_wg8;                  /* EVE_CONV_WG8          1   eight-wave kernels (0 off, 3: not for 16 x 16 x 128)       */
    int conv_wg8_min_tiles;        /* EVE_CONV_WG8_MIN_TILES 224  fewer tiles: four-wave kernels                          */
    int conv_wg8_s2_min_tiles;     /* EVE_CONV_WG8_S2_MIN_TILES 48  the same floor for the stride-2 forward / data grad.  */
    int halo_persist;              /* EVE_HALO_PERSIST      1   persistent tile stream for <= 64 input channels            */
    int wgrad_target_wgs;          /* EVE_WGRAD_TARGET_WGS  0   (0: 256 x resident workgroups per CU)                      */
    int wgrad_min_rows;            /* EVE_WGRAD_MIN_ROWS    1536 shortest pixel range of a weight-gradient split          */
    int wgrad_halo;                /* EVE_WGRAD_HALO        1   band-resident weight gradients (wgrad_halo.h)              */
    int wgrad_wg8;                 /* EVE_WGRAD_WG8         1   eight-wave weight gradients: the 256 x 256 tile (wgrad_wg8.h) and, for 3x3 layers with 128 input channels from 65 536 pixels up, the 128 x 384 tile (wgrad_wg8_t128.h); 2: the 128 x 384 tile at any pixel count (tests); 3: the 256 x 256 tile only (A/B); 0: neither */
    int wg64_th, wg64_nreg;        /* EVE_WG64_TH / _NREG   0 0 (0: largest band / region count that fits LDS)             */
    int wg64_fixed;                /* EVE_WG64_FIXED        1   unrolled wgrad_halo64_kernel for 32-wide planes            */
    int in_split;                  /* EVE_IN_SPLIT          1   64 Ki-element InstanceNorm planes as two channel halves    */
    int in_min_threads;            /* EVE_IN_MIN_THREADS    512                                                            */
    int in_stats_one_pass;         /* EVE_IN_STATS_ONE_PASS 1   shifted-moment statistics for planes beyond L2             */
    int stem_split;                /* EVE_STEM_SPLIT        1   two waves per image in the fused stem at small batches     */
    int in_trunk_kernels;          /* EVE_IN_TRUNK          1   branch-free InstanceNorm kernels for the ResNet trunk's cases */
    int stem_fused_wgrad;          /* EVE_STEM_FUSED_WGRAD  1   stem backward + weight gradient in one launch (eve_stem_bwd_wgrad) */
    int stem_fwd_pairs;            /* EVE_STEM_FWD_PAIRS    1   fused stem forward with two waves per image (32 channels each)       */
    int conv1x1_stream;            /* EVE_CONV1X1_STREAM    1   1x1 convolutions between 16..128 channels on the streaming kernel (no LDS), and the trunk's 1x1 / stride-2 shortcuts (64 -> 128, 128 -> 256: forward and accumulating data gradient) on its strided sibling; 2: stride 1 only */
    int conv3x3_stream;            /* EVE_CONV3X3_STREAM    1   3x3 / stride 1 between 16..64 channels on 64 / 128-wide images: row-streaming kernel */
    int in_big_planes;             /* EVE_IN_BIG_PLANES     1   register-resident InstanceNorm (no affine) for planes beyond 8 192 vectors, dealt by channels */
    int cgru_seq_max_b;            /* EVE_CGRU_SEQ_MAX_B    384 16-bit conv-GRU clip scans: one sequence per workgroup (cgru_scan1.hip) up to this many sequences, three per workgroup (cgru_scan.hip) beyond */
    int cgru_scan;                 /* EVE_CGRU_SCAN         1   conv-RNN bottleneck as ONE clip-long launch per direction (0: per-frame launches; 2: forward scan only, per-frame backward; 3: also the combinations the default leaves per frame because their scan measured slower: 16-bit CGRU / CLSTM at width 128) */
    int small_linear;              /* EVE_SMALL_LINEAR      1   float32 nn.Linear of the tail on the small-tile FMA kernels (linear_small.hip)  */
    int tail_loss_node;            /* EVE_TAIL_LOSS_NODE    1   EyeNet tail + losses as one autograd node (ops.EyeTailLossFn)                   */
    int bucket_elems;              /* EVE_BUCKET_ELEMS      4194304  floats per data-parallel gradient bucket (parallel.GradSync)              */
    int gate_wait_polls;           /* EVE_GATE_WAIT_POLLS   1<<21    polls (64 x 64 clocks apart) before a stream gate gives up and poisons the step */
    long long wgrad_halo_min_m;    /* EVE_WGRAD_HALO_MIN_M  1<<20 pixels from which the band-resident weight gradient runs */
} eve_dispatch_config;
int eve_get_dispatch_config(eve_dispatch_config* out);           /* what the entry points use now                         */
int eve_get_default_dispatch_config(eve_dispatch_config* out);   /* the built-in defaults (environment ignored)           */
int eve_set_dispatch_config(const eve_dispatch_config* cfg);     /* explicit override (tests, tuning); struct_bytes checked */
/* Device scratch is CALLER-OWNED and passed PER CALL (ABI v6; v5 kept one process-global pointer): the entry points that can
 * use scratch take `workspace` (16-byte aligned device pointer, or NULL) and `workspace_bytes`, use it on the stream of that
 * call only, and fall back to their scratch-free form when it is missing or too small.  Users: the split-K weight gradient of
 * the 256..512-channel layers (per-split partial filters with plain stores + a summing launch instead of 16 M float atomics)
 * and the data gradient of the stride-2 3x3 layers (filters re-packed per call for conv3x3_wg8_kernel<.., NT>).           */

/* ------------------------------------------------------------------------------------------------
 * Convolution as implicit GEMM on MFMA.  Replaces every nn.Conv2d / nn.Linear forward on the path:
 * torchvision ResNet convs built at src/models/eye_net.py:48-50 and run at :106; nn.Linear at
 * eye_net.py:51-56,81-92; nn.Conv2d at src/models/refine_net.py:48,52,61,214,217,221-222 and
 * src/models/common.py:338,362,395-398.  A Linear is the KH=KW=1, IH=IW=1 case.
 * ------------------------------------------------------------------------------------------------ */
typedef struct eve_conv_desc {
    int dtype;               /* EVE_DT_* of x / w / y                                   */
    int N, IH, IW, Cin;      /* x  : [N][IH][IW][Cin]                                   */
    int OH, OW, Cout;        /* y  : [N][OH][OW][Cout]                                  */
    int KH, KW, stride, pad; /* cross-correlation, zero padding                         */
} eve_conv_desc;

/* y = act(conv(x', w) + bias),  x' = pro_act(x * scale[n,c] + shift[n,c]) when in_scale_shift != NULL
 * (float [N][Cin][2]; padding stays zero AFTER the transform), else x' = x.  bias may be NULL.
 * epi_act = EVE_ACT_* [| EVE_EPI_ACCUMULATE]: with the flag the result is ADDED to what y holds (y += act(...)) in the
 * kernel epilogue -- `layers(x) + skip_layer(x)` of RefineNet's BasicBlock (refine_net.py:64-67) is the 1x1 skip
 * convolution accumulating into the 3x3 branch's output, no add launch.                                              */
#define EVE_EPI_ACCUMULATE 0x100
int eve_conv2d_fwd(const eve_conv_desc* d, const void* x, const void* w_ohwi, const float* bias,
                   int epi_act, const float* in_scale_shift, int pro_act, void* y,
                   eve_stream_t stream);
/* The same, and the InstanceNorm2d statistics of the output -- mean_rstd [N][Cout][2] = (mean, 1 / sqrt(biased variance + eps)) per
 * plane, taken on the stored (rounded) values -- from the convolution's own epilogue when the dispatched kernel walks whole
 * images (the row-streaming 3x3 kernel; ABI v7).  *stats_written = 1 if filled, 0 if the shape took another kernel (run
 * eve_instnorm_stats then).  refine_net.py:45-53: every convolution of a pre-activation block is followed by InstanceNorm2d. */
int eve_conv2d_fwd_stats(const eve_conv_desc* d, const void* x, const void* w_ohwi, const float* bias, int epi_act, void* y,
                         float* mean_rstd, float eps, int* stats_written, eve_stream_t stream);
/* dx = conv_transpose(dy, w): gradient w.r.t. the conv INPUT.  w_ihwo is [Cin][KH][KW][Cout].    */
int eve_conv2d_dgrad(const eve_conv_desc* d, const void* dy, const void* w_ihwo, void* dx,
                     void* workspace, unsigned long long workspace_bytes, eve_stream_t stream);
/* dx += the same data gradient (dx already holds the gradient of the block's other branch: autograd's add at
 * the residual fork of torchvision BasicBlock, fused into the epilogue).                              */
int eve_conv2d_dgrad_acc(const eve_conv_desc* d, const void* dy, const void* w_ihwo, void* dx,
                     eve_stream_t stream);
/* dw[Cout][KH][KW][Cin] (float, accumulated) += sum_m dy[m][co] * x'[m][(kh,kw,ci)]              */
int eve_conv2d_wgrad(const eve_conv_desc* d, const void* x, const void* dy,
                     const float* in_scale_shift, int pro_act, float* dw_ohwi,
                     void* workspace, unsigned long long workspace_bytes, eve_stream_t stream);
/* ... together with db[Cout] (float, accumulated) += sum_m dy[m][co] in the same pass over dy: autograd of a biased
 * nn.Conv2d (refine_net.py's U-Net and conv-GRU convolutions all carry one).                                   */
int eve_conv2d_wgrad_bias(const eve_conv_desc* d, const void* x, const void* dy, float* dw_ohwi, float* db,
                          void* workspace, unsigned long long workspace_bytes, eve_stream_t stream);
/* ResNet stem (torchvision ResNet.conv1: 7x7 / stride 2 / pad 3, 3 -> 64, no bias; eye_net.py:48-50), bf16:
 * eve_stem_pack_input writes x_padded [N][IH+6][IW+8][4] bf16 (channels 0..C-1, zero 4th channel and borders)
 * from the float NCHW patch; eve_stem7x7s2_fwd computes y [N][IH/2][IW/2][64] from it and the OHWI weights
 * with Cin padded to 8 ([64][7][7][8] bf16).  IH even, IW a multiple of 128.                           */
int eve_stem_pack_input(int dtype /* EVE_DT_BF16 | EVE_DT_F16 */, int N, int C, int IH, int IW, const float* src_nchw, void* x_padded,
                        eve_stream_t stream);
int eve_stem7x7s2_fwd(int dtype, int N, int IH, int IW, const void* x_padded, const void* w_ohwi8, void* y,
                      eve_stream_t stream);
/* Decoded uint8 frames on the device (datasources/eve_sequences.py:196-211 does this on the host and ships floats):
 * dst[n][c][y][x] (float) = src[n][y][x][c] * scale (+ shift): eye patches scale 2/255, shift -1; screen frames
 * scale 1/255, no shift.  One rounded multiply and one rounded add, bit-identical to the numpy expressions.      */
int eve_frames_u8_to_nchw(long long N, int H, int W, int C, const uint8_t* src_nhwc, float scale, float shift,
                          int has_shift, float* dst_nchw, eve_stream_t stream);
/* ... and the same values straight into the stem kernels' packed input x_padded [N][IH+6][IW+8][4] bf16 (what
 * eve_stem_pack_input builds from the float NCHW tensor).                                                      */
int eve_frames_u8_to_stem(int dtype, long long N, int C, int IH, int IW, const uint8_t* src_nhwc, float scale, float shift,
                          void* x_padded, eve_stream_t stream);
/* The whole stem in one launch: conv1 -> bn1 (InstanceNorm2d, no affine) -> relu -> maxpool 3x3/2 pad 1
 * (torchvision ResNet._forward_impl as built by eye_net.py:48-50).  The 64-channel convolution output is never
 * written: y_pool [N][IH/4][IW/4][64] bf16, idx (window position kh*3+kw of the arg-max, same shape, uint8) and
 * mean_rstd [N][64][2] are the only outputs.  IW == 128, IH a multiple of 4.                              */
int eve_stem_fwd_fused(int dtype, int N, int IH, int IW, const void* x_padded, const void* w_ohwi8, float eps,
                       void* y_pool, uint8_t* idx, float* mean_rstd, eve_stream_t stream);
/* Its backward up to the convolution output: dx [N][IH/2][IW/2][64] bf16 = d(conv1 out) from dy_pool, recomputing
 * the convolution from x_padded (autograd of bn1/relu/maxpool in eye_net.py:106); feed dx to eve_conv2d_wgrad. */
/* Round 4: backward AND weight gradient of the fused stem in ONE launch -- dw [64][7][8][4] float (accumulated; filter column
 * 7 and channel 3 do not exist) straight from d(y_pool): every recomputed convolution row's d(conv1 out) stays in LDS and is
 * multiplied there with the input rows the recomputation has staged anyway; the 1 GB d(conv1 out) tensor of
 * eve_stem_bwd_dx + eve_stem_wgrad is never written or read.  Same arithmetic per channel (float summation order aside).    */
int eve_stem_bwd_wgrad(int dtype, int N, int IH, int IW, const void* x_padded, const void* w_ohwi8, const float* mean_rstd,
                       const void* dy_pool, const void* dy_pool2, const void* y_pool, const uint8_t* idx, float* dw,
                       void* workspace, unsigned long long workspace_bytes, eve_stream_t stream);
/* `workspace`: at least eve_stem_bwd_wgrad_workspace(dtype, N, IH) bytes, 16-byte aligned, caller-owned, used on `stream` by this
 * call only: the two InstanceNorm plane sums and the masked, summed gradient are formed by a streaming pass of their own
 * (stem_grad_prep_kernel) and the fused kernel reads one pooled tensor and the arg-max codes, once.  REQUIRED since ABI v9 (v8
 * fell back to a one-launch form that read the three pooled tensors twice and spilled registers): NULL / too small is an error. */
unsigned long long eve_stem_bwd_wgrad_workspace(int dtype, int N, int IH);
/* ... and the stem's weight gradient from the same packed patches: dw [64][7][8][4] float (accumulated; filter
 * column 7 and channel 3 do not exist and are ignored by the caller).  Replaces autograd of conv1 (eye_net.py:106). */
int eve_stem_wgrad(int dtype, int N, int IH, int IW, const void* x_padded, const void* dconv, float* dw, eve_stream_t stream);
int eve_stem_bwd_dx(int dtype, int N, int IH, int IW, const void* x_padded, const void* w_ohwi8, const float* mean_rstd,
                    const void* dy_pool, const void* dy_pool2 /* nullable second summand */, const void* y_pool, const uint8_t* idx, void* dx, eve_stream_t stream);
/* Data gradient of the stem convolution back to the patch (autograd of conv1 w.r.t. its input, eye_net.py:48,106):
 *   dx_nchw[n][c][y][x] (float) = sum_{co,ky,kx} dconv[n][oy][ox][co] * W[co][c][ky][kx],  y = 2 oy - 3 + ky, x = 2 ox - 3 + kx,
 * dconv [N][IH/2][IW/2][64] in `dtype` (F32 / BF16 / F16: what eve_stem_bwd_dx, the stem conv's autograd or the generic conv's
 * backward hands over), accumulated in float32 and stored in float32, the patch's own layout and type.  IH, IW even, C <= 4.
 * w_packed is the filter re-packed by eve_stem_dgrad_pack from the float OIHW weight [64][C][7][7]: 1024 x 16 elements of
 * `dtype` (32 KB in 16-bit, 64 KB in float32), 16-byte aligned like dconv.  Both entries added in ABI v10 (additive).   */
int eve_stem_dgrad_pack(int dtype, int C, const float* w_oihw, void* w_packed, eve_stream_t stream);
int eve_stem_dgrad(int dtype, int N, int IH, int IW, int C, const void* dconv, const void* w_packed, float* dx_nchw,
                   eve_stream_t stream);
/* Small float32 linear layers (nn.Linear of the EyeNet tail, eye_net.py:52-90: fc, fc_common, GRU input
 * projection, gaze / pupil heads) with M rows and K, N <= 4096:
 *   fwd:   y[M][N]   = act(x[M][K] . w_in_out[K][N] + bias)
 *   dgrad: dx[M][K]  = (dy * act'(y))[M][N] . w_out_in[N][K]          (y may be NULL when act is NONE)
 *   wgrad: dw[N][K] += (dy * act'(y))^T . x ;  db[N] += column sums    (db nullable; float atomics)          */
int eve_linear_fwd(int M, int K, int N, const float* x, const float* w_in_out, const float* bias, int act,
                   float* y, eve_stream_t stream);
int eve_linear_dgrad(int M, int K, int N, const float* dy, const float* y, int act, const float* w_out_in,
                     float* dx, eve_stream_t stream);
int eve_linear_wgrad(int M, int K, int N, const float* dy, const float* y, int act, const float* x,
                     float* dw_out_in, float* db, eve_stream_t stream);
/* ... with row strides (a column range of a wider matrix on either side), a bias shorter than N (padded heads) and an
 * accumulating data gradient (dx += ...): what lets the tail run without cat / pad / slice / add launches (round 4).            */
int eve_linear_fwd_ex(int M, int K, int N, const float* x, int ldx, const float* w_in_out, const float* bias, int n_bias,
                      int act, float* y, int ldy, eve_stream_t stream);
int eve_linear_dgrad_ex(int M, int K, int N, const float* dy, int lddy, const float* y, int act, const float* w_out_in,
                        float* dx, int lddx, int accumulate, eve_stream_t stream);
/* gaze [M][2] = pi/2 * g2[:, :2] and pupil [M] = p2[:, 0] of the heads' 4-wide last layers (eye_net.py:139-146), and back:
 * d_g2 / d_p2 [2*BT][4] from the loss kernel's per-side unit gradients (rows: left clips, then right), scaled by
 * coeff * *g_full (device scalar, NULL = 1).                                                                                  */
/* cat[m][col .. col+3] = (h[m][0], h[m][1], 0, 0), rows 0 .. BT-1 from h_left [BT][2], BT .. 2BT-1 from h_right (eye_net.py:113-114's
 * torch.cat of fc's output and the head pose, written behind the 128 columns eve_linear_fwd_ex filled; ld, col multiples of 4).   */
int eve_tail_head_pose(int BT, const float* h_left, const float* h_right, float* cat, int ld, int col, eve_stream_t stream);
int eve_tail_outputs_fwd(int M, const float* g2, const float* p2, float* gaze, float* pupil, eve_stream_t stream);
int eve_tail_outputs_bwd(int BT, const float* dg_l, const float* dg_r, const float* dp_l, const float* dp_r, const float* g_full,
                         float coeff_ang, float coeff_l1, float* d_g2, float* d_p2, eve_stream_t stream);
/* The EyeNet train-step losses and their gradients in one launch (losses/angular.py:33-38, losses/l1.py,
 * losses/base_loss_with_validity.py:64-73; weighted sum of eve.py:234-265).  Every pointer argument is an array of
 * two device pointers {left, right}: g_pred/g_tgt [B][T][2] (pitch, yaw), p_pred/p_tgt [B][T], validity bytes [B][T].
 * terms[5] (zeroed by the caller) += {ang_l, l1_l, ang_r, l1_r, coeff_ang*(ang_l+ang_r) + coeff_l1*(l1_l+l1_r)};
 * dg/dp receive d(term of that side)/d(prediction).                                                     */
int eve_eye_losses(int B, int T, const float* const* g_pred, const float* const* g_tgt, const uint8_t* const* g_val,
                   const float* const* p_pred, const float* const* p_tgt, const uint8_t* const* p_val,
                   float coeff_ang, float coeff_l1, float* terms, float* const* dg, float* const* dp,
                   eve_stream_t stream);
/* Every validity-masked term of EVE.calculate_losses_and_metrics over [B][T][D <= 3] predictions (eve.py:286-439: the gaze /
 * PoG / pupil losses and metrics; src/losses/{mse,euclidean,l1,angular}.py with the clip reduction of
 * base_loss_with_validity.py:64-73) in ONE launch (ABI v7).  terms[i]: pred, tgt [B][T][D] float, valid [B][T] bytes, kind
 * 0 MSE | 1 Euclidean distance | 2 L1 | 3 angular error in degrees (D = 2: pitch, yaw), dpred = NULL or [B][T][D] <-
 * d term_i / d pred for a unit upstream gradient (kinds 0, 2, 3).  out[i] = term i.  n <= EVE_VEC_TERMS_MAX.                */
#define EVE_VEC_TERMS_MAX 32
typedef struct eve_vec_term { const float* pred; const float* tgt; const unsigned char* valid; float* dpred; int D; int kind; } eve_vec_term;
int eve_vector_terms(const eve_vec_term* terms, int n, int B, int T, float* out, eve_stream_t stream);
/* ------------------------------------------------------------------------------------------------
 * Gaze geometry, heat-maps and soft-argmax: the per-frame glue of EVE.forward either side of the two networks
 * (eve.py:114-166, 545-601).  Flat batches of N = B*T frames, float32, row-major small matrices.
 * ------------------------------------------------------------------------------------------------ */
/* to_screen_coordinates (models/common.py:157-187), optionally preceded by apply_offset_augmentation (:190-229) when
 * kappa/head_R are given.  g [N][2] (pitch, yaw), origin [N][3] mm (camera frame), R [N][3][3], inv_cam [N][4][4],
 * ppm [N][2] pixels per mm.  Outputs: g_out [N][2] (the augmented angles; optional without kappa), pog_mm [N][2],
 * pog_px [N][2] clamped to [0, screen], jac [N][6][2] = d(g_out, pog_mm, pog_px) / d(pitch, yaw) for the backward. */
int eve_gaze_to_pog(long long N, const float* g, const float* origin, const float* R, const float* inv_cam,
                    const float* ppm, const float* head_R, const float* kappa, float screen_w, float screen_h,
                    float* g_out, float* pog_mm, float* pog_px, float* jac, eve_stream_t stream);
/* dg [N][2] = jac^T (dg_out, dmm, dpx); any of the three incoming gradients may be null.                       */
int eve_gaze_to_pog_bwd(long long N, const float* jac, const float* dg_out, const float* dmm, const float* dpx,
                        float* dg, eve_stream_t stream);
/* calculate_combined_gaze_direction (common.py:136-154): g [N][2] from the mean eye origin to a screen point.     */
int eve_combined_gaze(long long N, const float* origin, const float* pog_mm, const float* R, const float* cam,
                      float* g, eve_stream_t stream);
/* batch_make_heatmaps (common.py:236-255): out [N][H][W] = 1e-8 + exp(-|p - c|^2 / (2 sigma^2)), c = centre_px * (W/screen_w,
 * H/screen_h); multiplied by validity[n] (bytes) when given (the label maps of eve.py:503-520).                  */
int eve_make_heatmaps(long long N, int H, int W, const float* centres_px, const uint8_t* validity, float sigma,
                      float screen_w, float screen_h, float* out, eve_stream_t stream);
int eve_make_heatmaps_bwd(long long N, int H, int W, const float* centres_px, float sigma, float screen_w, float screen_h,
                          const float* dout, float* dcentres, eve_stream_t stream);
/* soft_argmax (common.py:304-333): pog_px [N][2] = clamp(screen * E_softmax(100 h)[(x/(W-1), y/(H-1))]); stats [N][4] =
 * (lx, ly, max, sum exp) feed the backward.                                                                    */
int eve_soft_argmax_fwd(long long N, int H, int W, const float* heat, float screen_w, float screen_h, float* pog_px,
                        float* stats, eve_stream_t stream);
int eve_soft_argmax_bwd(long long N, int H, int W, const float* heat, const float* stats, const float* dpog,
                        float screen_w, float screen_h, float* dheat, eve_stream_t stream);
/* db[C] (float, accumulated) += sum over the M = N*OH*OW rows of dy[M][C]                         */
int eve_bias_grad(int dtype, long long M, int C, const void* dy, float* db, eve_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Instance normalisation (+ optional affine, residual add, activation).  Replaces
 * nn.InstanceNorm2d inside the ResNet (norm_layer at eye_net.py:50: eps 1e-5, biased variance, no
 * affine, no running stats) with the following ReLU / residual add of BasicBlock.forward, and the
 * affine InstanceNorm2d + activation pairs of refine_net.py:46-47,50-51,59-60,215-216.
 * ------------------------------------------------------------------------------------------------ */
/* mean_rstd[n][c] = (mean, 1/sqrt(var_biased + eps)) over the HW plane                            */
int eve_instnorm_stats(int dtype, int N, int HW, int C, const void* x, float eps, float* mean_rstd,
                       eve_stream_t stream);
/* y = act(gamma[c] * (x - mean) * rstd + beta[c] + res);  gamma/beta/res may be NULL              */
int eve_instnorm_act_fwd(int dtype, int N, int HW, int C, const void* x, const float* mean_rstd,
                         const float* gamma, const float* beta, const void* res, int act, void* y,
                         eve_stream_t stream);
/* g = dy * act'(y);  dx = gamma*rstd*(g - mean_hw(g) - xhat*mean_hw(g*xhat));  dres = g (if != NULL);
 * sums[n][c] = (sum_hw g, sum_hw g*xhat)  (reduce over n for dbeta / dgamma).
 * y may be NULL when there was no residual: act'(.) is then recomputed from x with the forward's own scale / shift
 * (beta is needed for that when gamma is given) -- one tensor less to read in both passes.                    */
int eve_instnorm_act_bwd(int dtype, int N, int HW, int C, const void* dy, const void* y,
                         const void* x, const float* mean_rstd, const float* gamma, const float* beta, int act,
                         void* dx, void* dres, float* sums, const void* dx_add, eve_stream_t stream);
/* dx_add (nullable, like x): a second gradient of the normalised tensor's INPUT, added to dx in the epilogue -- the identity-skip
 * blocks of RefineNet (refine_net.py:35-67: x feeds `layers` and the block's final add) then need no gradient-fork add launch. */

/* Two affine + activation heads over ONE normalised input: RefineNet's pre-activation BasicBlock feeds the block input to
 * `layers` (refine_net.py:46-47) and to `skip_layer` (:59-60), each starting with InstanceNorm2d(affine) -> activation.
 * y_h = act(gamma_h * (x - mean) * rstd + beta_h);  x is read once.  y_a / y_b are [N][HW][ldy] tensors (16-byte aligned).
 * The input may be the channel-concatenation of TWO sources (the decoder's torch.cat([upsampled, encoder_output]),
 * refine_net.py:125-126): x [N][HW][C] owns channels [0, C) of the heads, x2 [N][HW][C2] (nullable) channels [C, C + C2);
 * InstanceNorm statistics are per channel, so each source is normalised on its own (mean_rstd / mean_rstd2 from
 * eve_instnorm_stats) straight into the concatenated layout and the concatenation is never materialised un-normalised.
 * gamma_h / beta_h: C + C2 floats.  ldy >= C + C2.  y_b / gamma_b / beta_b may be NULL (one head).                     */
int eve_instnorm_act2_fwd(int dtype, int N, int HW, int C, const void* x, const float* mean_rstd,
                          const float* gamma_a, const float* beta_a, const float* gamma_b, const float* beta_b,
                          int act, void* y_a, void* y_b, int ldy, int C2, const void* x2, const float* mean_rstd2,
                          eve_stream_t stream);
/* g_h = dy_h * act'(y_h) (y_h recomputed from x);  dx = sum_h gamma_h*rstd*(g_h - mean_hw(g_h) - xhat*mean_hw(g_h*xhat)):
 * the gradient sum of the fork is formed in registers.  dy_a / dy_b: [N][HW][lddy] gradients of the heads; dx / dx2: dense
 * gradients of the sources.  sums_h[n][c] = (sum_hw g_h, sum_hw g_h*xhat) for the C + C2 channels.
 * dy_b (with gamma_b, beta_b, sums_b) and the second source (x2, mean_rstd2, dx2) may be NULL.                         */
int eve_instnorm_act2_bwd(int dtype, int N, int HW, int C, const void* dy_a, const void* dy_b, int lddy,
                          const void* x, const float* mean_rstd, const float* gamma_a, const float* beta_a,
                          const float* gamma_b, const float* beta_b, int act, void* dx, float* sums_a,
                          float* sums_b, int C2, const void* x2, const float* mean_rstd2, void* dx2, eve_stream_t stream);

/* Single-pass variants for planes that fit one workgroup's registers (HW*C <= 64 Ki elements): statistics and
 * apply in one launch (also writes mean_rstd), and the whole backward in one read of dy / y / x.
 * Same arithmetic as the three entry points above.  Return -1 (no error text) when the plane does not fit;
 * the caller then uses the multi-pass entry points.                                                 */
/* sign_mask (nullable, N*HW*C/vec bytes, vec = 16 / sizeof(element)): bit e of byte v = (element e of 16-byte vector v
 * of y is > 0) -- all a ReLU backward needs of y, at 1/16 of its bytes (the trunk's block-output InstanceNorm).   */
int eve_instnorm_fwd_fused(int dtype, int N, int HW, int C, const void* x, const float* gamma,
                           const float* beta, const void* res, int act, float eps, void* y,
                           float* mean_rstd, unsigned char* sign_mask, eve_stream_t stream);
/* dy2 (nullable): a second summand of the incoming gradient, added on load -- the residual fork of a ResNet
 * block delivers d(block input) as two tensors and the sum is never materialised.                      */
/* sign_mask (nullable; act == EVE_ACT_RELU): the forward's mask, read INSTEAD of y.                          */
/* beta (nullable): with gamma and no y, act'(.) is recomputed from x with the forward's own scale / shift
 * (act(x * rstd*gamma + (beta - mean*rstd*gamma))) -- no residual: one tensor less to read and to keep.       */
int eve_instnorm_bwd_fused(int dtype, int N, int HW, int C, const void* dy, const void* dy2, const void* y,
                           const void* x, const float* mean_rstd, const float* gamma, const float* beta, int act,
                           void* dx, void* dres, float* sums, const unsigned char* sign_mask, const void* dx_add, eve_stream_t stream);

/* out[j] = sum_r in[r][j] (float32, fixed summation order): the batch reduction of the per-plane partials `sums` above into
 * d(beta) / d(gamma) of an affine InstanceNorm2d (refine_net.py:46,50,59,215).                                          */
int eve_sum_rows(int rows, int cols, const float* in, float* out, eve_stream_t stream);
/* in [rows][C][2] (per-plane (d beta, d gamma) partials of an affine InstanceNorm backward) -> out0[c] += sum_r in[r][c][0],
 * out1[c] += sum_r in[r][c][1], fixed order (ABI v7): the two parameter gradients land in the caller's gradient buffer.  */
int eve_sum_rows_pairs(int rows, int C, const float* in, float* out0, float* out1, eve_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Element-wise activation gradient: dx = dy * act'(y)  (for Linear/conv epilogue activations).
 * ------------------------------------------------------------------------------------------------ */
int eve_act_bwd(int dtype, long long n, const void* dy, const void* y, int act, void* dx,
                eve_stream_t stream);
/* out = a + b (same dtype), used for gradient fan-in of the residual / skip branches.             */
int eve_add(int dtype, long long n, const void* a, const void* b, void* out, eve_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Pooling / resampling.  nn.MaxPool2d(3,2,1) and AdaptiveAvgPool2d(1) of the torchvision ResNet
 * (eye_net.py:48,106); nn.AdaptiveMaxPool2d (refine_net.py:93) and nn.Upsample(bilinear,
 * align_corners=False) (refine_net.py:101).
 * ------------------------------------------------------------------------------------------------ */
/* 3x3 / stride 2 / pad 1 max-pool; idx[n][oh][ow][c] (uint8) = kh*3+kw of the first maximum       */
int eve_maxpool3x3s2_fwd(int dtype, int N, int IH, int IW, int C, const void* x, void* y,
                         uint8_t* idx, eve_stream_t stream);
int eve_maxpool3x3s2_bwd(int dtype, int N, int IH, int IW, int C, const void* dy,
                         const uint8_t* idx, void* dx, eve_stream_t stream);
/* ResNet stem tail fused: y = maxpool3x3s2(relu(IN(x))) with no affine, given mean_rstd of x (statistics
 * from eve_instnorm_stats); the normalised full-resolution tensor is never written.  idx as above.
 * Backward: dx = d(loss)/dx through pool, ReLU and the instance norm, from the pooled tensors and x.  */
int eve_in_relu_maxpool_fwd(int dtype, int N, int IH, int IW, int C, const void* x,
                            const float* mean_rstd, void* y, uint8_t* idx, eve_stream_t stream);
int eve_in_relu_maxpool_bwd(int dtype, int N, int IH, int IW, int C, const void* dy_pool,
                            const void* y_pool, const uint8_t* idx, const void* x,
                            const float* mean_rstd, void* dx, eve_stream_t stream);
/* mean over the HW plane: y[N][C]; and its gradient dx[n][hw][c] = dy[n][c] / HW                  */
int eve_avgpool_fwd(int dtype, int N, int HW, int C, const void* x, void* y, eve_stream_t stream);
int eve_avgpool_bwd(int dtype, int N, int HW, int C, const void* dy, void* dx, eve_stream_t stream);
/* ABI v10: the same with the pooled [N][C] side in FLOAT32 memory (values of format `dtype`, widened): EyeNet's trunk -> tail
 * hand-over (eye_net.py:52-56: avgpool -> flatten -> fc) without the two cast launches; bit-identical to pool + cast.          */
int eve_avgpool_fwd_f32(int dtype, int N, int HW, int C, const void* x, float* y, eve_stream_t stream);
int eve_avgpool_bwd_f32(int dtype, int N, int HW, int C, const float* dy, void* dx, eve_stream_t stream);
/* adaptive max-pool, window i = [floor(i*I/O), ceil((i+1)*I/O)); idx = flat ih*IW+iw (int32)       */
int eve_adaptive_maxpool_fwd(int dtype, int N, int IH, int IW, int OH, int OW, int C, const void* x,
                             void* y, int32_t* idx, eve_stream_t stream);
/* add (nullable, [N][IH][IW][C]): a second gradient of the pooled tensor's INPUT, added in the epilogue -- the encoder output
 * feeds the pool AND the decoder's skip connection (refine_net.py:103-126), autograd's fork add is then not launched.            */
int eve_adaptive_maxpool_bwd(int dtype, int N, int IH, int IW, int OH, int OW, int C,
                             const void* dy, const int32_t* idx, const void* add, void* dx, eve_stream_t stream);
/* bilinear resize, align_corners=False, and its adjoint                                            */
int eve_bilinear_fwd(int dtype, int N, int IH, int IW, int OH, int OW, int C, const void* x, void* y,
                     eve_stream_t stream);
int eve_bilinear_bwd(int dtype, int N, int IH, int IW, int OH, int OW, int C, const void* dy,
                     void* dx, eve_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Layout / dtype plumbing at the module boundary (the reference hands NCHW float tensors:
 * eye_net.py:100-103, refine_net.py:239-248).
 * ------------------------------------------------------------------------------------------------ */
/* dst[n][h][w][c < Cpad] = c < C ? src[n][c][h][w] : 0                                             */
int eve_nchw_to_nhwc(int dtype_dst, int N, int C, int H, int W, int Cpad, const float* src_nchw,
                     void* dst_nhwc, eve_stream_t stream);
int eve_nhwc_to_nchw(int dtype_src, int N, int C, int H, int W, int Cpad, const void* src_nhwc,
                     float* dst_nchw, eve_stream_t stream);
/* float <-> dtype casts of flat buffers (weights to the compute dtype)                             */
int eve_cast(int dtype_src, int dtype_dst, long long n, const void* src, void* dst,
             eve_stream_t stream);
/* OHWI float master weights -> OHWI and IHWO copies in the compute dtype (one pass)                */
int eve_pack_weights(int dtype_dst, int Cout, int taps, int Cin, const float* w_ohwi, void* dst_ohwi,
                     void* dst_ihwo, eve_stream_t stream);
/* The same for up to EVE_PACK_BATCH_MAX weights in one launch (a model's conv weights after an optimiser step). */
#define EVE_PACK_BATCH_MAX 48
typedef struct eve_pack_item {
    const float* w_ohwi; void* dst_ohwi; void* dst_ihwo;      /* either destination may be NULL */
    int Cout, taps, Cin;
    int src_Cout, src_Cin;   /* ABI v10: the SOURCE is [src_Cout][taps][src_Cin] (0 = Cout / Cin); the destinations' extra output /
                              * input channels are written as zeros -- conv1's 3 -> 4/8 input channels, the 130 -> 132 wide
                              * fc_common.0, the 2- and 1-wide heads padded to 4 were a fill + a copy launch each, every step */
} eve_pack_item;
int eve_pack_weights_batch(int dtype_dst, int count, const eve_pack_item* items /* host array */, eve_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Recurrent cells.
 * GRU scan: torch.nn.GRUCell applied over T steps (eye_net.py:69,125; state hand-over :116-133).
 *   gi  : float [S][T][3H]  = W_ih x_t + b_ih for every step (batched GEMM done by the caller)
 *   whh : float [3H][H] (the forward scan takes its transpose whh_t [H][3H]); bhh float [3H];
 *   h0 float [S][H] or NULL (= zeros, eye_net.py:120-122)
 *   hs  : float [S][T][H] all hidden states;  work: float [S][T][3H] (r, z, n) + [S][T][H] (hn) saved
 *   H   : up to 256 (one workgroup per sequence), or a multiple of 16 up to 1024 (recurrent_wide.hip: one workgroup per
 *         tile of 16 sequences, float32 MFMA); the same rule holds for the RNN / LSTM scans below; other widths are refused
 * ------------------------------------------------------------------------------------------------ */
int eve_gru_scan_fwd(int S, int T, int H, const float* gi, const float* whh_t, const float* bhh,
                     const float* h0, float* hs, float* gates, float* hn_pre, eve_stream_t stream);
/* given dhs [S][T][H] (gradient on every h_t): dgi [S][T][3H], dgh [S][T][3H] (for dW_hh/db_hh by
 * GEMM), dh0 [S][H] (may be NULL)                                                                  */
int eve_gru_scan_bwd(int S, int T, int H, const float* dhs, const float* whh, const float* h0,
                     const float* hs, const float* gates, const float* hn_pre, float* dgi, float* dgh,
                     float* dh0, eve_stream_t stream);
/* nn.RNNCell (tanh) and nn.LSTMCell over T -- the other recurrent variants of eye_net.py:60-67.  gi = W_ih x + b_ih
 * for all steps ([S][T][G*H], G = 1 / 4 gate blocks in torch order i,f,g,o), whh_t = W_hh^T [H][G*H], whh = W_hh.
 * The backward returns dpre = d(pre-activation) [S][T][G*H] (the gradient of gi, and the operand of dW_hh, db_hh). */
int eve_rnn_scan_fwd(int S, int T, int H, const float* gi, const float* whh_t, const float* bhh, const float* h0,
                     float* hs, eve_stream_t stream);
int eve_rnn_scan_bwd(int S, int T, int H, const float* dhs, const float* whh, const float* hs, float* dpre,
                     float* dh0, eve_stream_t stream);
int eve_lstm_scan_fwd(int S, int T, int H, const float* gi, const float* whh_t, const float* bhh, const float* h0,
                      const float* c0, float* hs, float* cs, float* gates, eve_stream_t stream);
int eve_lstm_scan_bwd(int S, int T, int H, const float* dhs, const float* dcs, const float* whh, const float* c0,
                      const float* hs, const float* cs, const float* gates, float* dpre, float* dh0, float* dc0,
                      eve_stream_t stream);

/* conv-GRU gate math of CGRUCell.forward (common.py:409-414), NHWC, C = hidden size:
 *   step 1: (r, u) = sigmoid(g1[..., 0:C], g1[..., C:2C]);  rh = r * h
 *   step 2: o = tanh(g2);  h' = (1 - u) * o + u * h                                                */
/* CGRUCell over all T frames of a clip in ONE persistent launch (the 5x8x64 bottleneck of refine_net.py:132-176):
 * hidden state resident in LDS, both gate GEMMs on MFMA with the filter banks streamed through an LDS-DMA ring,
 * sigmoid / tanh / blend as epilogues.  dtype bf16 / f16: cgru_scan.hip (three sequences per workgroup, 16-bit MFMA);
 * dtype f32 (ABI v7): cell_scan_f32.hip (one workgroup per sequence, float state, v_mfma_f32_16x16x4_f32 -- the parity
 * mode's 1e-4 rad runs on one launch per clip as well).  xs [B][T][5][8][64]; h0 [B][5][8][64] or NULL; w1 = gates_1 OHWI
 * [128][3][3][128] (inputs x|h), w2 = gate_2 OHWI [64][3][3][128] (inputs r*h|x); outputs: hs [B][T][5][8][64]
 * (state, caller's order) and, TIME-major [T][B][5][8][.] for the frame-reversed backward: hs_tm, ru (both sigmoid
 * gates, 128 ch), rh (r*h), og (tanh gate).                                                               */
int eve_cgru_scan_fwd(int dtype, int B, int T, const void* xs, const void* h0, const void* w1, const float* b1, const void* w2,
                      const float* b2, void* hs, void* hs_tm, void* ru, void* rh, void* og, eve_stream_t stream);
/* Backward of eve_cgru_scan_fwd in ONE persistent launch (bf16 / f16 / f32; common.py:400-415 differentiated): frames last to first, the
 * gradient into the previous hidden state carried in registers.  Time-major inputs [T][B][5][8][.]: dhs_tm (d hs), and the
 * forward's ru / og / hs_tm; h0 or NULL; w1t = gates_1 bank IHWO [128][3][3][128], w2t = gate_2 bank IHWO [128][3][3][64].
 * Outputs (time-major): dg1_all [..][128], dg2_all [..][64] (pre-activation gradients: the operands of the batched weight /
 * bias gradients), dxs_tm [..][64]; dh0 [B][5][8][64] or NULL.                                                             */
int eve_cgru_scan_bwd(int dtype, int B, int T, const void* dhs_tm, const void* ru, const void* og, const void* hs_tm, const void* h0,
                      const void* w1t, const void* w2t, void* dg1_all, void* dg2_all, void* dxs_tm, void* dh0,
                      eve_stream_t stream);
/* CRNNCell (common.py:331-352: h_t = tanh(conv3x3([x_t | h_{t-1}]) + b)) over all T frames of a clip in ONE launch, float32
 * (ABI v7; 16-bit callers convert the 5x8x64 bottleneck tensors).  xs [B][T][5][8][64]; h0 [B][5][8][64] or NULL; w OHWI
 * [64][3][3][128]; bias [64].  Outputs hs [B][T][5][8][64] and its time-major copy hs_tm [T][B][5][8][64].                 */
int eve_crnn_scan_fwd(int B, int T, const float* xs, const float* h0, const float* w, const float* bias, float* hs,
                      float* hs_tm, eve_stream_t stream);
/* Backward of eve_crnn_scan_fwd, one launch: time-major dhs_tm / hs_tm; wt = the bank IHWO [128][3][3][64].  Outputs
 * (time-major) dpre_all [T][B][5][8][64] = gradient of the pre-activation (operand of the batched weight / bias gradient),
 * dxs_tm; dh0 [B][5][8][64] or NULL.                                                                                       */
int eve_crnn_scan_bwd(int B, int T, const float* dhs_tm, const float* hs_tm, const float* wt, float* dpre_all, float* dxs_tm,
                      float* dh0, eve_stream_t stream);
/* CLSTMCell (common.py:355-385; gates in / forget / out / cell) over all T frames of a clip in ONE launch, float32, forward
 * only -- the reference's Bottleneck stores the (h, c) tuple and never feeds it on (refine_net.py:168-174), so no gradient
 * reaches the cell.  w OHWI [256][3][3][128]; bias [256]; h0 / c0 or NULL.  Outputs hs, cs [B][T][5][8][64].               */
int eve_clstm_scan_fwd(int B, int T, const float* xs, const float* h0, const float* c0, const float* w, const float* bias,
                       float* hs, float* cs, eve_stream_t stream);
/* The five clip scans above with the bottleneck width C (refine_net_num_features) as an argument after T (additive: ABI v10).
 * Operand shapes are the ones documented above with 64 -> C and 128 -> 2C:
 *   cgru:  xs [B][T][5][8][C]; h0 [B][5][8][C] or NULL; w1 OHWI [2C][3][3][2C], b1 [2C]; w2 OHWI [C][3][3][2C], b2 [C];
 *          hs [B][T][5][8][C]; time-major hs_tm, rh, og [T][B][5][8][C], ru [T][B][5][8][2C];
 *          backward: w1t IHWO [2C][3][3][2C], w2t IHWO [2C][3][3][C]; dg1_all [T][B][5][8][2C]; dg2_all, dxs_tm [T][B][5][8][C];
 *          dh0 [B][5][8][C] or NULL.
 *   crnn:  w OHWI [C][3][3][2C], bias [C]; wt IHWO [2C][3][3][C]; hs, hs_tm, dpre_all, dxs_tm as above with C channels.
 *   clstm: w OHWI [4C][3][3][2C], bias [4C]; h0 / c0 [B][5][8][C] or NULL; hs, cs [B][T][5][8][C].
 * Widths: C in {32, 64, 128} for every entry and format.  float32 (cgru with dtype f32, crnn, clstm): one workgroup per
 * sequence at every B (cell_scan_f32.hip, kernel names "<base>" at 64 and "<base><32>" / "<base><128>" otherwise).  cgru with
 * dtype bf16 / f16: C = 64 on the 16-bit MFMA kernels; C = 32 / 128 on the 16-bit-storage instantiation of the float32 scan
 * (values rounded to the format where the 16-bit kernels round them, products on the float32 MFMA; names
 * "cgru_scan_f32_{fwd,bwd}_kernel<C, eve::bf16_t>").  Any other C returns non-zero with a message in eve_last_error() and
 * launches nothing.  The entry points without `_c` are these with C = 64. */
int eve_cgru_scan_fwd_c(int dtype, int B, int T, int C, const void* xs, const void* h0, const void* w1, const float* b1,
                        const void* w2, const float* b2, void* hs, void* hs_tm, void* ru, void* rh, void* og, eve_stream_t stream);
int eve_cgru_scan_bwd_c(int dtype, int B, int T, int C, const void* dhs_tm, const void* ru, const void* og, const void* hs_tm,
                        const void* h0, const void* w1t, const void* w2t, void* dg1_all, void* dg2_all, void* dxs_tm, void* dh0,
                        eve_stream_t stream);
int eve_crnn_scan_fwd_c(int B, int T, int C, const float* xs, const float* h0, const float* w, const float* bias, float* hs,
                        float* hs_tm, eve_stream_t stream);
int eve_crnn_scan_bwd_c(int B, int T, int C, const float* dhs_tm, const float* hs_tm, const float* wt, float* dpre_all,
                        float* dxs_tm, float* dh0, eve_stream_t stream);
int eve_clstm_scan_fwd_c(int B, int T, int C, const float* xs, const float* h0, const float* c0, const float* w, const float* bias,
                         float* hs, float* cs, eve_stream_t stream);
/* The CLSTM clip scan for a cell whose output IS used (eve_amd's opt-in config key refine_net_clstm_feeds_features; the
 * reference drops it, see eve_clstm_scan_fwd).  Float32, C in {32, 64, 128}, one workgroup per sequence (cell_scan_f32.hip,
 * kernels "clstm_scan_f32_fwd_train_kernel" / "clstm_scan_f32_bwd_kernel", "<32>" / "<128>" appended off 64).
 * fwd_train: operands and hs / cs of eve_clstm_scan_fwd_c, bit for bit, plus what the backward reads, time-major:
 *   gates_tm [T][B][5][8][4C] = sigmoid(in), sigmoid(forget), sigmoid(out), tanh(cell); cs_tm, hs_tm [T][B][5][8][C].
 * bwd: dhs_tm [T][B][5][8][C]; dcs_tm = gradient arriving at the stored cell states, or NULL; gates_tm / cs_tm of the forward;
 *   c0 as in the forward or NULL; wt = the bank IHWO [2C][3][3][4C].  Outputs (time-major) dpre_all [T][B][5][8][4C] = gradient
 *   of the gate pre-activations (operand of the batched weight / bias gradient), dxs_tm [T][B][5][8][C]; dh0 / dc0 [B][5][8][C]
 *   or NULL.  Weight and bias gradients are not formed here.                                                                */
int eve_clstm_scan_fwd_train_c(int B, int T, int C, const float* xs, const float* h0, const float* c0, const float* w,
                               const float* bias, float* hs, float* cs, float* gates_tm, float* cs_tm, float* hs_tm,
                               eve_stream_t stream);
int eve_clstm_scan_bwd_c(int B, int T, int C, const float* dhs_tm, const float* dcs_tm, const float* gates_tm, const float* cs_tm,
                         const float* c0, const float* wt, float* dpre_all, float* dxs_tm, float* dh0, float* dc0,
                         eve_stream_t stream);
int eve_cgru_gates1(int dtype, long long P, int C, const void* g1, const void* h, void* ru, void* rh,
                    eve_stream_t stream);
int eve_cgru_gates2(int dtype, long long P, int C, const void* g2, const void* ru, const void* h,
                    void* o, void* hnew, eve_stream_t stream);
/* backward of step 2: given dh' -> dg2 (pre-tanh, [P][C]); dru [P][2C] = (0, gradient on the
 * post-sigmoid update gate); dh [P][C] = direct path u * dh'                                        */
int eve_cgru_gates2_bwd(int dtype, long long P, int C, const void* dhnew, const void* ru,
                        const void* h, const void* o, void* dg2, void* dru, void* dh,
                        eve_stream_t stream);
/* backward of step 1: given d(rh) [P][C], dru [P][2C] and saved ru, h -> dg1 (pre-sigmoid, [P][2C])
 * and dh [P][C] = d(rh) * r                                                                         */
int eve_cgru_gates1_bwd(int dtype, long long P, int C, const void* drh, const void* dru,
                        const void* ru, const void* h, void* dg1, void* dh, eve_stream_t stream);

/* conv-LSTM gate math of CLSTMCell.forward (common.py:376-385), forward only: gates [P][4C] in the
 * reference's chunk order (in, forget, out, cell); c' = sig(f)*c + sig(i)*tanh(g); h' = sig(o)*tanh(c').
 * The reference never back-propagates through it (refine_net.py:168-174 drops tuple states).         */
int eve_clstm_gates_fwd(int dtype, long long P, int C, const void* gates, const void* c_prev, void* h,
                        void* c, eve_stream_t stream);
/* Adjoint of eve_clstm_gates_fwd (for a cell whose output is used: refine_net_clstm_feeds_features): dh, dc_in [P][C] =
 * gradients arriving at h' and c' (dc_in or NULL), gates [P][4C] = the forward's pre-activations, c_prev [P][C]
 * -> dgates [P][4C] (gradient of the pre-activations) and dc_prev [P][C] = dc' * sig(f).                    */
int eve_clstm_gates_bwd(int dtype, long long P, int C, const void* dh, const void* dc_in, const void* gates,
                        const void* c_prev, void* dgates, void* dc_prev, eve_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * RefineNet output head and the heat-map losses (csrc/heatmap_loss.hip).
 * ------------------------------------------------------------------------------------------------ */
/* nn.Sigmoid of `final` (src/models/refine_net.py:221-223) evaluated in float: logits = channel 0 of the last 1x1
 * convolution's NHWC output [pixels][Cpad] (compute dtype) -> out float [pixels] (= heatmap_final [N][1][H][W]).   */
int eve_heatmap_head_fwd(int dtype, long long pixels, int Cpad, const void* logits, float* out, eve_stream_t stream);
/* dlogits[pixel][c] = c == 0 ? dy * y * (1 - y) : 0, compute dtype                                                   */
int eve_heatmap_head_bwd(int dtype, long long pixels, int Cpad, const float* dy, const float* y, void* dlogits,
                         eve_stream_t stream);
/* loss_ce_heatmap_* (kind 0: F.binary_cross_entropy per frame, src/losses/cross_entropy.py:27-35) or
 * loss_mse_heatmap_final (kind 1, src/losses/mse.py) with the validity reduction of
 * src/losses/base_loss_with_validity.py:64-73.  pred, gt float [B][T][HW]; validity uint8 [B][T]; outputs:
 * per_map float [B*T] (per-frame means), loss float [1], w float [B*T] = d loss / d per_map.                        */
int eve_heatmap_loss_fwd(int kind, int B, int T, int HW, const float* pred, const float* gt, const uint8_t* validity,
                         float* per_map, float* loss, float* w, eve_stream_t stream);
/* dpred = upstream[0] * w[frame] / HW * d(element loss)/d pred  (upstream: device scalar, no host sync)             */
int eve_heatmap_loss_bwd(int kind, int BT, int HW, const float* pred, const float* gt, const float* w,
                         const float* upstream, float* dpred, eve_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Round 4: the EyeNet tail (src/models/eye_net.py:109-146): all its weight / bias gradients in one launch:
 * dW[N][K] += (dY * act'(Y))^T . [X | X2], db[N] += column sums.                                                      */
#define EVE_WGRAD_BATCH_MAX 12
typedef struct eve_wgrad_problem {
    const float* dY;         /* [M][N]                                                                                        */
    const float* Y;          /* [M][N] or NULL (act == EVE_ACT_NONE)                                                          */
    const float* X;          /* [M][K1]                                                                                       */
    const float* X2;         /* [M][K2] or NULL: the input is the concatenation (K1 + K2 <= K; the rest of K is zero padding) */
    float* dW;               /* [N][K] accumulated                                                                            */
    float* db;               /* [N] accumulated, or NULL                                                                      */
    int M, N, K, K1, K2, act, rows_per_split /* set by the library */;
    int ldY;                 /* row stride of dY and Y in floats (0 = N): the first N columns of a wider matrix                  */
    int ldX, ldW;            /* row strides of X (0 = K1) and dW (0 = K): K1 leading columns of a wider X, an unpadded dW        */
    int x_shift_T;           /* > 0: X row m is replaced by row m - 1, zero where m % x_shift_T == 0 (the previous hidden state   */
    int reserved;            /*      of a scan over sequences of x_shift_T steps: dW_hh = dpre^T . h_prev)                        */
} eve_wgrad_problem;
typedef struct eve_wgrad_batch { int n; int first_block[EVE_WGRAD_BATCH_MAX]; eve_wgrad_problem p[EVE_WGRAD_BATCH_MAX]; } eve_wgrad_batch;
int eve_linear_wgrad_batch(const eve_wgrad_problem* problems, int n, eve_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Optimiser step over flat float buffers.  torch.optim.Adam with coupled L2 weight decay
 * (src/train.py:49-55) after nn.utils.clip_grad_norm_ (src/core/training.py:492-498).
 * ------------------------------------------------------------------------------------------------ */
/* Stream gates (ABI v7) -- how a hipGraph replay of forward + backward releases each gradient bucket's all-reduce on the
 * communication stream the moment the bucket's last gradient has been written, with the RCCL calls left OUTSIDE the graph
 * (north_star: "RCCL all-reduce of gradients ... overlapped with backward"; the reference's backward -> clip -> step sequence is
 * src/core/training.py:489-502).  eve_gate_signal: a one-thread kernel (capturable: it becomes a node of the graph behind the
 * weight-gradient kernel that completes the bucket) that releases and increments *flag.  eve_gate_wait: a one-wave kernel on the
 * OTHER stream that polls *flag until it has reached `value` (the replay count) -- or *value_ref when value_ref != NULL: a
 * device word, which is what lets the wait itself be a node of the graph (the replay's first node counts the replays there, and
 * the graph's clip + Adam nodes sit behind gate-waits for the "bucket reduced" words the communication stream signals) --
 * bounded: after max_polls polls (0: eve_dispatch_config.gate_wait_polls, ~seconds) it increments *timeouts, writes +inf to
 * *poison (when not NULL) and returns, so a missing signal cannot hang the device -- and cannot be trained on either (ABI v9):
 * `poison` is a float the caller keeps INSIDE the last gradient bucket it all-reduces, so after the collectives every rank
 * holds a non-zero value there and eve_adam_step(.., poison) skips the update on every rank alike (the all-reduce that ran on
 * the half-written bucket is discarded with it).  flag / timeouts / value_ref: device words, zeroed by the caller.           */
int eve_gate_signal(unsigned* flag, eve_stream_t stream);
int eve_gate_wait(const unsigned* flag, unsigned value, const unsigned* value_ref, unsigned* timeouts, float* poison,
                  unsigned max_polls, eve_stream_t stream);

/* out[0] += sum g^2 (caller zeroes out[0]; take sqrt on the host or in eve_adam_step).  Fixed summation order: the
 * result is bit-reproducible, so data-parallel replicas clip by the identical factor.  workspace: EVE_SUMSQ_WORKSPACE
 * floats of scratch owned by the caller.                                                            */
#define EVE_SUMSQ_WORKSPACE 1024
int eve_sumsq(long long n, const float* g, float* out, float* workspace, eve_stream_t stream);
/* Optimiser state that must live on the device (a replayed hipGraph cannot change kernel arguments, and the decision to skip
 * a step is taken on the device): 48 bytes, caller-owned, zero-initialised except loss_scale (1 = no scaling).            */
typedef struct eve_adam_guard {
    int step;             /* optimiser steps TAKEN so far = Adam's bias-correction exponent                                  */
    int skipped_total;    /* calls that left weights and moments untouched because the gradient norm was not finite         */
    int skipped_run;      /* ... consecutive ones (two in a row halve loss_scale)                                           */
    int good_run;         /* consecutive taken steps since the loss scale last changed (2 000 double it)                     */
    float loss_scale;     /* the factor the caller multiplied the loss by before backward; divided out of the gradient here */
    float applied;        /* 1 if the last call updated the weights, 0 if it skipped                                        */
    float clip;           /* factor the last taken step applied to the stored gradient (1/loss_scale and the norm clip)     */
    float bc1, bc2_sqrt;  /* bias corrections of the last taken step                                                        */
    int skipped_gate;     /* calls skipped because *poison != 0: a gradient bucket's stream gate timed out (ABI v9); also in skipped_total */
    float reserved[2];
} eve_adam_guard;
/* clip factor c = min(1, max_norm / (sqrt(*sumsq) * gscale' + 1e-6)) if sumsq != NULL and max_norm > 0, else 1;
 * g' = c * gscale' * g + wd * p;  m,v Adam moments;  p -= lr * mhat / (sqrt(vhat) + eps).
 * guard == NULL: gscale' = gscale, bias-correction step t = `step` (host value), no overflow handling.
 * guard != NULL: gscale' = gscale / guard->loss_scale, t = ++guard->step; with check_finite a non-finite *sumsq (an
 *   overflowed float16 gradient) SKIPS the step: weights, moments and guard->step stay, guard->skipped_* count it and the
 *   loss scale backs off (see eve_adam_guard).  The learning rate is `lr`, or *lr_dev (device float) when lr_dev != NULL: the
 *   LR schedule of src/core/training.py:382-418,436-442 writes *lr_dev before each (possibly replayed) step.
 *   poison != NULL (guard required): *poison != 0 (or NaN) -- a stream gate of this step's gradient exchange timed out,
 *   eve_gate_wait -- SKIPS the step like a non-finite norm does, counted in guard->skipped_gate; the loss scale is left alone. */
int eve_adam_step(long long n, float* p, const float* g, float* m, float* v, const float* sumsq,
                  float max_norm, float gscale, float lr, float beta1, float beta2, float eps,
                  float weight_decay, int step, eve_adam_guard* guard, int check_finite, const float* lr_dev,
                  const float* poison, eve_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Streaming inference (eve_amd/stream.py: EVEStream carries both networks' recurrent states across calls; forward only).
 * ------------------------------------------------------------------------------------------------ */
/* The float32 packs of the EyeNet tail (eye_net.py:109-146 of the shipped configuration: GRU, one cell, H = 128, head-pose
 * input), each weight as [in][out] (the PackedWeight IHWO of a 1x1 layer).                                                   */
typedef struct eve_eye_tail_weights {
    const float* fc_w;  const float* fc_b;   /* cnn_layers.fc  [512][128], [128]                                             */
    const float* c0_w;  const float* c0_b;   /* fc_common.0    [>= 130][128] (rows 128, 129: head pose), [128]               */
    const float* c2_w;  const float* c2_b;   /* fc_common.2    [128][128], [128]                                             */
    const float* ih_w;  const float* ih_b;   /* rnn_cells.0    W_ih^T [128][384], b_ih [384] (gate order r, z, n)            */
    const float* hh_w;  const float* hh_b;   /*                W_hh^T [128][384], b_hh [384]                                 */
    const float* g0_w;  const float* g0_b;   /* fc_to_gaze.0   [128][128], [128]                                             */
    const float* g2_w;                       /* fc_to_gaze.2   [128][4] (columns 2, 3 unused), no bias                       */
    const float* p0_w;  const float* p0_b;   /* fc_to_pupil.0  [128][128], [128]                                             */
    const float* p2_w;  const float* p2_b;   /* fc_to_pupil.2  [128][4] (column 0), [1]                                      */
} eve_eye_tail_weights;
/* The whole EyeNet tail forward in ONE launch, the GRU state read and written in place: fc -> [. | head pose] -> fc_common
 * (SELU) -> GRU input projection -> the recurrence -> fc_to_gaze (SELU, tanh, x pi/2) and fc_to_pupil (SELU, ReLU).
 * feats [S][T][512] float32 (eve_avgpool_fwd_f32's output; 16-byte aligned), head_pose [S][T][2]; h [S][128] in/out: the state
 * before the first frame, overwritten with the state after the last; reset int [S] or NULL: rows with reset[s] != 0 start
 * from zero instead.  Outputs gaze [S][T][2] (rad), pupil [S][T], hs [S][T][128] or NULL.  Any T (sub-chunks of 16 frames
 * inside the kernel).  One workgroup per sequence.                                                                          */
int eve_eye_tail_stream_fwd(int S, int T, const float* feats, const float* head_pose, const eve_eye_tail_weights* weights,
                            float* h, const int* reset, float* gaze, float* pupil, float* hs, eve_stream_t stream);
/* Per-stream state hand-over: dst[s][i] = (reset && reset[s]) ? 0 : src[s][i] for s < S, i < row_elems; row strides in
 * elements (>= row_elems); dtype f32 / bf16 / f16 (bit copies).  In place (src == dst) it applies resets before a step; from
 * a scan's last frame (hs + (T-1) * row) into a state buffer it commits the step.  src and dst are equal or disjoint.        */
int eve_stream_state_rows(int dtype, int S, long long row_elems, long long src_stride, long long dst_stride, const void* src,
                          void* dst, const int* reset, eve_stream_t stream);
/* Ragged steps (EVEStream.step(lengths=...)): sequence s consumes only its first lengths[s] frames of the chunk.
 * eve_eye_tail_stream_fwd with per-sequence lengths, int [S] on the device or NULL (= every sequence T frames, the call
 * above, which runs the same kernel): h[s] is overwritten with the state after frame lengths[s] - 1, or left as it is for
 * lengths[s] == 0 -- zeroed all the same when reset[s] != 0.  A length outside 0..T is clamped.  Every frame is still
 * computed; gaze, pupil and hs at t >= lengths[s] hold unspecified (finite-input-dependent) values.                          */
int eve_eye_tail_stream_fwd_len(int S, int T, const float* feats, const float* head_pose, const eve_eye_tail_weights* weights,
                                float* h, const int* reset, const int* lengths, float* gaze, float* pupil, float* hs,
                                eve_stream_t stream);
/* Per-stream commit at a per-stream frame: for s < S with lengths[s] > 0,
 * dst[s][i] = src[s * src_stride + (lengths[s] - 1) * frame_stride + i], i < row_elems; rows with lengths[s] == 0 keep what
 * they hold.  src: S sequences of T frames (a scan's per-frame states), strides in elements, each >= row_elems
 * (sequence-major or time-major); lengths int [S] on the device, read by the kernel and clamped to T there, so
 * one captured graph serves every length pattern and no value reads outside src; dtype f32 / bf16 / f16 (bit copies).
 * Refused without a launch: NULL src / dst / lengths, T < 1, src and dst overlapping (resets stay with the in-place
 * eve_stream_state_rows call before the step).                                                                              */
int eve_stream_state_rows_at(int dtype, int S, int T, long long row_elems, long long frame_stride, long long src_stride,
                             long long dst_stride, const void* src, void* dst, const int* lengths, eve_stream_t stream);
/* Masked steps (EVEStream.step(eye_mask=..., skip_invalid_pose=...); both entries additive: ABI v10): a sequence skips frames
 * in the MIDDLE of a chunk.  No scan takes a mask; instead every sequence's usable frames are moved to the front of the chunk,
 * the sequences run through the ragged entry points above with their usable counts as lengths, and the per-frame outputs are
 * moved back.  The plan, one launch per step, for B streams of T frames:
 *   eye (b, t, e) is usable iff t < clamp(lengths[e*B + b], 0, T) && mask[b][t][e] != 0 && pose_valid[b][t][e] != 0
 * e = 0 left, 1 right; mask, pose_valid uint8 (or bool) [B][T][2] on the device, lengths int [2B] in the ragged layout; each of
 * the three may be NULL and then does not restrict.  There are 3B sequences: the eye sequences s = e*B + b < 2B (EyeNet's row
 * order), whose frame t is usable iff eye (b, t, e) is, and the frame sequences s = 2B + b (RefineNet's), whose frame t is
 * usable iff either eye of (b, t) is.  Written for every s:
 *   count[s]      the number of usable frames
 *   perm[s][T]    a STABLE PARTITION of 0..T-1: the usable t ascending, then the unusable t ascending -- always a permutation,
 *                 so a gather through it writes every destination row and reads only rows of its own sequence
 *   inv[s][T]     its inverse: inv[s][perm[s][j]] = j
 * and eye_valid [B][T][2], valid [B][T] uint8 (1 / 0): the effective eye mask and whether either eye of the frame is usable.
 * One thread per sequence walks its T frames serially (no ballot or prefix scan: nothing depends on the wave size).  Refused
 * without a launch: a NULL output, B outside 1..2^20, T < 1, 3*B*T >= 2^31.                                                  */
int eve_stream_mask_plan(int B, int T, const uint8_t* mask, const uint8_t* pose_valid, const int* lengths, int* count, int* perm,
                         int* inv, uint8_t* eye_valid, uint8_t* valid, eve_stream_t stream);
/* Row gather that applies a plan: dst[s][j] = src[s][index[s][j]] for s < S, j < T -- through perm it compacts a sequence's
 * usable frames to the front, through inv it puts per-frame results back.  Rows are row_bytes bytes (a multiple of 4), bit
 * copies; src: frame and sequence strides in bytes (multiples of 4, each >= row_bytes: a view into wider rows works); dst is
 * dense [S][T][row_bytes]; index int [S][T] on the device, clamped to 0..T-1 by the kernel, so no value reads outside src (a
 * plan's perm / inv need no clamping; a stray value costs a wrong row, not a fault).  16-byte vector copies when both base
 * pointers, both strides and row_bytes are multiples of 16, dword copies otherwise (pointers must be 4-byte aligned).
 * Refused without a launch: NULL src / dst / index, T < 1, S < 1 or S*T >= 2^31, row_bytes <= 0 or not a multiple of 4, a
 * stride below row_bytes or a stride or pointer that is no multiple of 4, src and dst overlapping (never in place).         */
int eve_stream_permute_rows(int S, int T, long long row_bytes, long long frame_stride_bytes, long long seq_stride_bytes,
                            const void* src, void* dst, const int* index, eve_stream_t stream);
/* Live screen captures: exact area (box) down-sampling of uint8 frames src [N][IH][IW][C] (C = 3, or 4 with the fourth channel
 * ignored: the alpha of BGRA capture APIs; the channel order is kept, a BGR -> RGB swap stays with the caller) to RefineNet's
 * screen input dst [N][3][OH][OW] float in [0, 1], OH <= IH and OW <= IW.  The reference never sees a full-resolution screen:
 * its loader opens screen.128x72.mp4, scaled offline by ffmpeg (datasources/eve_sequences.py:243-245), and normalises it with
 * preprocess_screen_frames (:205-211); this entry point stands where a live caller has the desktop itself, and is NOT a
 * reproduction of that (bicubic, lossy) file.  Contract, per frame and channel:
 *   wy = |[iy*OH, (iy+1)*OH) n [oy*IH, (oy+1)*IH)|   integer overlap of source row iy and output row oy (sums to IH over iy)
 *   wx = |[ix*OW, (ix+1)*OW) n [ox*IW, (ox+1)*IW)|   the same along the row (sums to IW)
 *   S  = sum wy * wx * src[iy][ix][c]                 an integer <= 255 * IH * IW, exact in 32 unsigned bits
 *   dst[c][oy][ox] = (float)((double)S / (double)(IH * IW)) * (float)(1.0 / 255)
 * so a frame already at the target size gives eve_frames_u8_to_nchw(scale 1/255)'s bits, an integer ratio (1920 x 1080 ->
 * 128 x 72: 15 x 15) the plain box mean kept in float, and a fractional ratio (1366 x 768) true fractional-overlap weights, not
 * adaptive_avg_pool2d's floor / ceil windows.  One launch, every source byte loaded once (rows that two output rows share, at
 * fractional ratios, by both).  Refused without a launch: C other than 3 or 4, upscaling in either direction, IH * IW >
 * 16 843 009 (covers 3840 x 2160; beyond it S could exceed 32 bits), IW * C > 40 960 bytes (one row of sums is kept in LDS). */
int eve_screen_u8_area_to_nchw(long long N, int IH, int IW, int C, const uint8_t* src_nhwc, int OH, int OW, float* dst_nchw,
                               eve_stream_t stream);
/* The same for a BGR(A) capture (what capture APIs and OpenCV deliver): dst[c] is taken from source channel 2 - c, so the result
 * equals eve_screen_u8_area_to_nchw on the channel-reversed capture bit for bit, without that copy.  Kernel names:
 * screen_u8_area_bgr_kernel<true | false>.  Same limits and refusals.                                                       */
int eve_screen_u8_area_bgr_to_nchw(long long N, int IH, int IW, int C, const uint8_t* src_nhwc, int OH, int OW, float* dst_nchw,
                                   eve_stream_t stream);
/* Live camera frames: one eye patch per call cut from whole uint8 frames [N][IH][IW][C] (C = 3, or 4 with the fourth channel
 * ignored; the channel order is kept; IH, IW <= 16384) through a per-frame homography warps [N][3][3] float, row-major m, that
 * maps a PATCH pixel to a CAMERA pixel -- the matrix cv2.warpPerspective takes with WARP_INVERSE_MAP; a caller who holds the
 * perspective-normalisation matrix W (camera -> patch) passes inv(W).  Integer coordinates are pixel centres; the patch is
 * OH x OW, both <= 4096.  The reference reads such patches pre-cut from *_eyes.mp4 and normalises them on the host
 * (datasources/eve_sequences.py:196-203); its config names whole frames (camera_frame_type = 'full') but no model-side code
 * consumes them.  Contract, bit-exact, for output pixel (oy, ox):
 *   X  = (m00*ox + m01*oy) + m02      Y = (m10*ox + m11*oy) + m12      Wd = (m20*ox + m21*oy) + m22        in float64
 *        (each product of a float and an integer <= 4096 is exact in float64, so fused multiply-adds give the same bits; only
 *        this association must be kept, and the coordinate is never stepped incrementally along a row)
 *   u = X / Wd, v = Y / Wd            the correctly rounded float64 division
 *   inside iff Wd > 0 && u > -1 && u < IW && v > -1 && v < IH       tested in float64 before any conversion to an integer; a
 *        NaN makes its comparison false, so such a pixel is outside
 *   fu = floor(u*256 + 0.5), x0 = fu >> 8, ax = fu & 255;  fv, y0, ay the same from v
 *   taps p00 = (y0, x0), p01 = (y0, x0+1), p10 = (y0+1, x0), p11 = (y0+1, x0+1); a tap outside [0, IH) x [0, IW) reads 0
 *   S = (256-ax)(256-ay) p00 + ax(256-ay) p01 + (256-ax)ay p10 + ax ay p11      an integer <= 255 * 65536 < 2^24; 0 outside
 *   value = (float(S) * 2^-16) * float(2/255) + (-1.0f)             the first product exact, then one rounded multiply and one
 *        rounded add with no contraction: eve_frames_u8_to_nchw(scale 2/255, shift -1) on the sample
 * Hence an integer translation gives eve_frames_u8_to_nchw / _to_stem's bits on the crop, and everything outside the frame is
 * -1.0.  eve_eye_warp_u8_to_nchw writes dst [N][3][OH][OW] float; eve_eye_warp_u8_to_stem the stem kernels' packed
 * x_padded [N][OH+6][OW+8][4] bf16 / f16 (pixel at (y+3, x+4), the pad ring and the fourth channel zero, values rounded to
 * nearest even as eve_stem_pack_input rounds).  No alignment is asked of `frames`.  Refused without a launch: a null pointer,
 * N < 1, C other than 3 or 4, IH or IW > 16384, OH or OW > 4096, a dtype other than bf16 / f16 for the packed form.        */
int eve_eye_warp_u8_to_nchw(long long N, int IH, int IW, int C, const uint8_t* frames_nhwc, const float* warps, int OH, int OW,
                            float* dst_nchw, eve_stream_t stream);
int eve_eye_warp_u8_to_stem(int dtype /* EVE_DT_BF16 | EVE_DT_F16 */, long long N, int IH, int IW, int C, const uint8_t* frames_nhwc,
                            const float* warps, int OH, int OW, void* x_padded, eve_stream_t stream);
/* The same pair for RAW frames of a camera with lens distortion: the networks were trained on undistorted video, and the
 * normalisation matrix W is defined on the undistorted image, so inv(W) now points into an image that is never made -- the
 * coordinate goes through the camera's distortion model before the taps are read, in the same single launch.  lens [N][12] float,
 * one row per patch, widened to float64 on the device:
 *   L = (fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6)
 * OpenCV's pinhole + radial / tangential / rational model, in OpenCV's coefficient order behind the four intrinsics (a 4- or
 * 5-coefficient calibration leaves the rest zero).  Contract, bit-exact: X, Y, Wd, u = X / Wd, v = Y / Wd as above; then in
 * float64, every operation rounded on its own (no contraction) and in exactly this association
 *   x  = (u - cx) / fx            y  = (v - cy) / fy
 *   xx = x*x   yy = y*y   xy = x*y   r2 = xx + yy
 *   num = ((k3*r2 + k2)*r2 + k1)*r2 + 1.0
 *   den = ((k6*r2 + k5)*r2 + k4)*r2 + 1.0
 *   rad = num / den               a = xy + xy
 *   xd = (x*rad + p1*a) + p2*(r2 + (xx + xx))
 *   yd = (y*rad + p1*(r2 + (yy + yy))) + p2*a
 *   ud = fx*xd + cx               vd = fy*yd + cy
 *   inside iff Wd > 0 && den > 0 && ud > -1 && ud < IW && vd > -1 && vd < IH        (a NaN fails its comparison)
 * and from (ud, vd) on the plain contract: floor(ud*256 + 0.5), the four integer-weighted taps with zeros outside the frame,
 * S * 2^-16 * float(2/255) + (-1), -1.0 outside.  Further:
 *   - a row whose eight coefficients k1..k6, p1, p2 are all +-0 takes the plain path for its patch and gives eve_eye_warp_u8_to_*'s
 *     bits whatever its intrinsics say (fx*((u - cx)/fx) + cx is not u in floating point), so a calibrated and an uncalibrated
 *     camera can share a batch; the decision is per patch;
 *   - degenerate rows are not refused: a NaN among the values used, or fx == 0 / fy == 0 with coefficients, falls out of the
 *     comparisons as an all-black (-1.0) patch; a negative focal length is a mirrored camera and works;
 *   - den > 0 blacks everything at and beyond the rational model's pole, where rad would change sign and land inside the frame;
 *   - far outside the calibrated field a barrel polynomial folds back into the image, as it does in OpenCV: not guarded;
 *   - not offered: thin-prism and tilt coefficients (OpenCV's 12- and 14-element forms), skew, fisheye models, gradients.
 * Layouts, limits and refusals are the plain pair's, plus a null `lens`; messages carry the entry point's name.             */
int eve_eye_warp_lens_u8_to_nchw(long long N, int IH, int IW, int C, const uint8_t* frames_nhwc, const float* warps, const float* lens,
                                 int OH, int OW, float* dst_nchw, eve_stream_t stream);
int eve_eye_warp_lens_u8_to_stem(int dtype /* EVE_DT_BF16 | EVE_DT_F16 */, long long N, int IH, int IW, int C, const uint8_t* frames_nhwc,
                                 const float* warps, const float* lens, int OH, int OW, void* x_padded, eve_stream_t stream);
/* The same patches from frames in the layouts cameras and decoders deliver, converted tap by tap inside the same launch: no RGB
 * frame is ever made.  `frames` holds N frames back to back, each byte-linear (no row pitch, one pointer):
 *   EVE_PIX_BGR    [IH][IW][3]          channel 2 is red, channel 0 blue
 *   EVE_PIX_BGRA   [IH][IW][4]          the same, a fourth channel ignored
 *   EVE_PIX_NV12   [IH*3/2][IW]         IH rows of luma, then IH/2 rows of interleaved U, V: for pixel (y, x), U is byte
 *                                       IH*IW + (y>>1)*IW + (x & ~1) of the frame and V the next byte
 *   EVE_PIX_I420   [IH*3/2][IW]         luma, then the U plane of (IH/2)*(IW/2) bytes, then the V plane: U is byte
 *                                       IH*IW + (y>>1)*(IW/2) + (x>>1), V is (IH/2)*(IW/2) bytes further
 *   EVE_PIX_YUYV   [IH][IW][2]          Y is [y][x][0], U is [y][x & ~1][1], V is [y][x | 1][1]
 * NV12 and I420 need IH and IW even, YUYV IW even; IH, IW <= 16384 as before.  Chroma is the NEAREST sample, replicated over its
 * 2 x 2 block (YUYV: its pair), as OpenCV's cvtColor replicates it.  Conversion, bit-exact, per tap and BEFORE the blend, in
 * int32 with arithmetic shifts (every intermediate is below 2^30 in magnitude):
 *   yy = max(0, Y - y0) * CY;   u = U - 128;   v = V - 128
 *   R = clamp((yy + 2^19 + CVR*v)         >> 20, 0, 255)
 *   G = clamp((yy + 2^19 - CVG*v - CUG*u) >> 20, 0, 255)
 *   B = clamp((yy + 2^19 + CUB*u)         >> 20, 0, 255)
 * with each constant floor(c * 2^20 + 0.5) of its coefficient:
 *   matrix          y0   CY       CVR      CUG     CVG     CUB
 *   EVE_YUV_BT601   16   1220542  1673527  409993  852492  2116026    limited range; OpenCV's COLOR_YUV2RGB_NV12 numbers
 *   EVE_YUV_BT709   16   1220542  1880097  223347  558891  2214593    limited range
 *   EVE_YUV_JFIF     0   1048576  1470104  360853  748826  1858077    full range (MJPEG)
 * `matrix` is ignored for BGR(A).  A tap outside the frame adds 0 to all three sums (it is NOT the conversion of Y = U = V = 0).
 * From the three 8-bit values on, everything is the contract above: hence, for every format F and matrix M,
 *   warp_F(buf) == eve_eye_warp_u8_to_*(to_rgb_F,M(buf))        bit for bit, in the float form and in both packed forms,
 * with to_rgb the per-pixel conversion applied to the whole frame (tests/pixel_format_ref.py).  lens: NULL for the plain
 * contract, or [N][12] rows for the lens contract (eve_eye_warp_lens_u8_to_*).  No alignment is asked of `frames`.  Kernel names:
 * eye_warp_fmt_kernel<F,L,T> with F in bgr, bgra, nv12, i420, yuyv; L plain or lens; T float, eve::bf16_t or eve::f16_t.
 * Refused without a launch: an unknown format, an unknown matrix with a YUV format, odd dimensions as above, and what the
 * plain pair refuses.  Row pitches, crops, UYVY / NV21 / YV12 and P010's high bytes go through eve_eye_warp_surface_to_nchw
 * below.  Not offered: planes in separate allocations, 10-bit arithmetic, bilinear chroma up-sampling, gradients.            */
enum { EVE_PIX_BGR = 0, EVE_PIX_BGRA = 1, EVE_PIX_NV12 = 2, EVE_PIX_I420 = 3, EVE_PIX_YUYV = 4 };
enum { EVE_YUV_BT601 = 0, EVE_YUV_BT709 = 1, EVE_YUV_JFIF = 2 };
int eve_eye_warp_fmt_to_nchw(int format, int matrix, long long N, int IH, int IW, const uint8_t* frames, const float* warps,
                             const float* lens /* may be NULL */, int OH, int OW, float* dst_nchw, eve_stream_t stream);
int eve_eye_warp_fmt_to_stem(int dtype /* EVE_DT_BF16 | EVE_DT_F16 */, int format, int matrix, long long N, int IH, int IW,
                             const uint8_t* frames, const float* warps, const float* lens /* may be NULL */, int OH, int OW,
                             void* x_padded, eve_stream_t stream);
/* Live screen captures as decoders and capture paths deliver them: eve_screen_u8_area_to_nchw's area average of a frame in one of
 * the layouts above, converted pixel by pixel inside the same launch -- no RGB frame is ever made, and an NV12 / I420 capture is
 * half of RGB's bytes to read (YUYV two thirds).  src holds N frames back to back, byte-linear as for eve_eye_warp_fmt_to_nchw
 * (no pitches, one pointer); NV12 and I420 need IH and IW even, YUYV IW even.  Contract, for F in NV12, I420, YUYV and every
 * matrix M:
 *   screen_area_F(buf) == eve_screen_u8_area_to_nchw(to_rgb_F,M(buf))          bit for bit
 * with to_rgb the per-pixel integer conversion stated above (chroma the nearest sample) and the area average the one stated at
 * eve_screen_u8_area_to_nchw: S = sum wy * wx * v over the CONVERTED 8-bit values, an exact 32-bit integer, then
 * (float)((double)S / (double)(IH * IW)) * (float)(1.0 / 255).  The order is convert, then average: the clamps make the
 * conversion non-linear, so averaging Y, U and V first gives other bits (tests/screen_format_ref.py).  EVE_PIX_BGR and
 * EVE_PIX_BGRA are handed to eve_screen_u8_area_bgr_to_nchw's kernel (`matrix` ignored): one entry point serves every code.
 * A workgroup takes one (frame, output row); a thread owns 8 luma columns (one 8-byte load per row, the chroma bytes under
 * them once per row pair) and keeps 24 column sums in registers; a width that is no multiple of 8 or a base that is not
 * 16-byte aligned takes a byte-column form with the same bits.  Kernel names: screen_area_fmt_kernel<F,true | false> with F in
 * nv12, i420, yuyv (true: the vector form), screen_u8_area_bgr_kernel<true | false> for BGR(A).  Refused without a launch,
 * the message beginning "screen_area_fmt_to_nchw:": bad arguments, an unknown format, an unknown matrix with a YUV format, odd
 * dimensions as above, upscaling in either direction, IH * IW > 16 843 009, IW * 12 > 163 840 bytes (one row of three 32-bit
 * column sums is kept in LDS; BGR(A): IW * C * 4), N * OH >= 2^31.  Row pitches, crops, UYVY / NV21 / YV12 and P010's high
 * bytes go through eve_screen_area_surface_to_nchw below.  Not offered: planes in separate allocations, 10-bit arithmetic,
 * bilinear chroma up-sampling.                                                                                              */
int eve_screen_area_fmt_to_nchw(int format, int matrix, long long N, int IH, int IW, const uint8_t* src, int OH, int OW,
                                float* dst_nchw, eve_stream_t stream);
/* Surfaces: frames as a hardware decoder or a capture API leaves them in memory -- rows with a pitch, more coded rows than visible
 * ones, chroma planes at aligned offsets, a window of a larger texture -- addressed through one small descriptor, so that no
 * de-pitch, crop or byte-shuffle copy runs before the step.  The address rule is the whole contract: component c of pixel (x, y)
 * of the visible region is the single byte at
 *   frame + offset[c] + (y >> ys) * pitch[c] + (x >> xs) * step[c]
 * with xs = ys = 0 for component 0 and for EVE_SURF_RGB, xs = xshift and ys = yshift for components 1 and 2 of EVE_SURF_YUV, all in
 * 64-bit arithmetic; frame n begins n * frame_stride bytes behind the pointer.  That covers packed and planar RGB / BGR / RGBA /
 * BGRA / ARGB with a pitch (for BGRA: offset = {2, 1, 0}, step 4); NV12, NV21, I420, YV12, YUYV, UYVY, YVYU, NV16, I422, I444; any
 * crop (a crop is other offsets; on a subsampled axis its origin must be even, or the chroma phase shifts); and P010 / P016 read
 * as their most significant byte (offset + 1 within the little-endian word, step 2 for luma and 4 for chroma): that sample is the
 * 16-bit word >> 8, a TRUNCATION to 8 bits, not a rounding.  Chroma is the nearest sample.  From the three 8-bit values on --
 * the integer matrix for EVE_SURF_YUV, everything behind it -- the contracts are those of the format entry points above, so with
 * linear() the gather of the visible region into the byte-linear layout (tests/surface_ref.py),
 *   eye_warp_surface(buf, S)    == eve_eye_warp_fmt_to_* (or _u8_to_*) on linear(buf, S)
 *   screen_area_surface(buf, S) == eve_screen_area_fmt_to_nchw (or eve_screen_u8_area_to_nchw) on linear(buf, S)
 * bit for bit.  No byte outside the addresses the rule names is read: padding, coded rows below the picture and a fourth channel
 * never reach a result.  All planes lie inside one frame's byte range [0, frame_bytes).                                         */
enum { EVE_SURF_RGB = 0, EVE_SURF_YUV = 1 };
typedef struct eve_surface {
    int struct_bytes;        /* sizeof(eve_surface); a mismatch is refused                                    */
    int kind;                /* EVE_SURF_RGB: components are R, G, B.  EVE_SURF_YUV: Y, U, V                     */
    int width, height;       /* the VISIBLE region, IW x IH; pixel (0, 0) is its top-left                      */
    long long frame_stride;  /* bytes from one frame to the next                                               */
    long long frame_bytes;   /* bytes of a frame that may be read: the limit of the bound check                */
    long long offset[3];     /* byte, within its frame, of component c's sample for pixel (0, 0)               */
    int pitch[3];            /* bytes from a row of component c to the next, >= 1                              */
    int step[3];             /* bytes from a sample of component c to the next along a row, >= 1               */
    int xshift, yshift;      /* YUV only, 0 or 1: components 1, 2 are read at (x >> xshift, y >> yshift)        */
} eve_surface;
/* The eye-patch warp from a surface: eve_eye_warp_fmt_to_nchw / _to_stem with the four taps of an output pixel read through the
 * address rule; coordinates, lens model (lens NULL or [N][12]), weights, blend, value and both output layouts are the same code.
 * The descriptor travels by value in the kernel's arguments.  matrix: EVE_YUV_* for EVE_SURF_YUV, ignored for EVE_SURF_RGB.
 * Kernel names: eye_warp_surface_kernel<K,L,T> with K rgb or yuv; L plain or lens; T float, eve::bf16_t or eve::f16_t.  Refused
 * without a launch, the message beginning with the entry point's name: a null descriptor, a wrong struct_bytes, an unknown kind, an
 * unknown matrix with EVE_SURF_YUV, shifts outside 0..1 or non-zero for EVE_SURF_RGB, a pitch or step < 1, a negative offset, any
 * component whose last addressed byte offset + ((height-1) >> ys) * pitch + ((width-1) >> xs) * step is >= frame_bytes,
 * frame_bytes > frame_stride with N > 1, and what the plain pair refuses (width, height <= 16384).                             */
int eve_eye_warp_surface_to_nchw(const eve_surface* surface, int matrix, long long N, const uint8_t* frames, const float* warps,
                                 const float* lens /* may be NULL */, int OH, int OW, float* dst_nchw, eve_stream_t stream);
int eve_eye_warp_surface_to_stem(int dtype /* EVE_DT_BF16 | EVE_DT_F16 */, const eve_surface* surface, int matrix, long long N,
                                 const uint8_t* frames, const float* warps, const float* lens /* may be NULL */, int OH, int OW,
                                 void* x_padded, eve_stream_t stream);
/* The screen area resize from a surface, in eve_screen_area_fmt_to_nchw's order: convert every visible pixel, the exact integer
 * area sum, one division.  8-bit 4:2:0 with luma step 1 and chroma either interleaved in one plane (NV12, NV21) or in two planes
 * (I420, YV12) keeps the wide loads: 8 luma bytes per row and 8 (4 + 4) chroma bytes per row pair when width is a multiple of 8
 * and base pointer, offsets, pitches and frame_stride put every such load on its own size; otherwise a byte form with the same
 * bits.  Every other descriptor (packed YUV, RGB kinds, P010, 4:2:2, 4:4:4) takes a generic form of three byte loads per pixel.
 * Kernel names: screen_area_surface_kernel<yuv420,true | false> (true: the vector form) and screen_area_surface_kernel<generic,false>.
 * One row of three 32-bit column sums is kept in LDS (width * 12 <= 163 840 bytes) and width * height <= 16 843 009, as above.
 * Refused without a launch, the message beginning "screen_area_surface_to_nchw:": what eve_eye_warp_surface_to_nchw refuses of
 * the descriptor, bad arguments, upscaling in either direction, those two limits, N * OH >= 2^31.                              */
int eve_screen_area_surface_to_nchw(const eve_surface* surface, int matrix, long long N, const uint8_t* src, int OH, int OW,
                                    float* dst_nchw, eve_stream_t stream);
/* The tracking overlay: one launch that turns N full-resolution captures into the annotated frames an encoder or a display reads.
 * src: N frames back to back in `in_format`, byte-linear as above (EVE_PIX_RGB / _RGBA: [IH][IW][3 | 4], channel 0 red; these two
 * codes are taken here only).  dst: `out_format` EVE_PIX_RGB or _BGR ([IH][IW][3]), EVE_PIX_NV12 or _I420 ([IH*3/2][IW], IH and IW
 * even).  `matrix` serves both directions.  Per output pixel (X, Y), in 8-bit RGB, the layers in this order
 * (tests/overlay_ref.py is the contract in numpy; the result equals it bit for bit -- after the three float32 quantisations
 * below everything is integer arithmetic):
 *   1. source   the capture pixel converted exactly as eve_eye_warp_fmt_to_nchw converts a tap (chroma the nearest sample).
 *   2. heat     heat float [N][HH][HW] (NULL: no layer), colour heat_rgb = 0xRRGGBB, amax in 0..255, HH, HW <= 1024:
 *                 q = (int)rint(min(max(h, 0), 1) * 255) in float32, NaN -> 0;
 *                 nx = (2X+1)*HW - IW;  fx = max(nx, 0)*128 / IW;  x0 = min(fx >> 8, HW-1);  x1 = min(x0+1, HW-1);  wx = fx & 255
 *                 (the same in y: bilinear, align_corners = false, 8 fractional bits);
 *                 a = (q00*(256-wx)*(256-wy) + q01*wx*(256-wy) + q10*(256-wx)*wy + q11*wx*wy + 32768) >> 16;
 *                 alpha = (a*amax + 127) / 255;   per channel v = (v*(255-alpha) + c*alpha + 127) / 255.
 *   3. inset    inset uint8 [N][ih][iw][3] RGB (NULL: no layer): an opaque replace of the zoom*ih x zoom*iw rectangle whose top-left
 *               pixel is (ix0, iy0) by inset[(Y-iy0)/zoom][(X-ix0)/zoom] (mirror != 0: column iw-1-j); zoom in 1..4.
 *   4. markers  M <= 8, in index order: centres float [N][M][2] in the caller's pixel units, marker_valid uint8 [N][M] (NULL: all
 *               valid), marker_table int [M][4] = (r_fill, r_outline, fill 0xRRGGBB, outline 0xRRGGBB), radii in output pixels,
 *               0..255.  qx = rint((x * sx) * 8) in float32, each product rounded (qy with sy), ties to even: sx = IW / (the width
 *               the centres refer to).  Not drawn: marker_valid == 0, a coordinate that is not finite, |q| > 2^20.  A disc of
 *               radius r covers n = #{(i, j) in 0..3 : (8X+2i+1-qx)^2 + (8Y+2j+1-qy)^2 <= 64 r^2} of a pixel's 4 x 4 sub-samples
 *               and v = (v*(16-n) + c*n + 8) >> 4; the outline disc first (r_outline > 0 only), then the fill disc.
 *   5. output   EVE_PIX_RGB / _BGR: the three bytes.  NV12 / I420, with K = sign(c) * floor(|c| * 2^20 + 0.5) of each coefficient:
 *                 Y = clamp((KYR*R + KYG*G + KYB*B + (y0 << 20) + 2^19) >> 20, 0, 255) per pixel (arithmetic shift);
 *                 U, V likewise with offset 128 from the 2 x 2 block's (sum of four + 2) >> 2 per channel.
 *                 matrix          y0   Y row                    U row                           V row
 *                 EVE_YUV_BT601   16   0.257  0.504  0.098      -0.148    -0.291    0.439       0.439  -0.368    -0.071
 *                 EVE_YUV_BT709   16   0.183  0.614  0.062      -0.101    -0.339    0.439       0.439  -0.399    -0.040
 *                 EVE_YUV_JFIF     0   0.299  0.587  0.114      -0.168736 -0.331264 0.5         0.5    -0.418688 -0.081312
 *               A round trip through eve_eye_warp_fmt_to_nchw's inverse is off by at most (2, 1, 2) in (R, G, B) under BT601 and
 *               BT709 and by at most (1, 1, 1) under JFIF, over all 2^24 colours.
 * frame_valid uint8 [N] (NULL: all valid): a 0 gives layers 1 and 5 alone, the converted capture.
 * One launch; a workgroup takes a (frame, row pair), a thread 2 rows x 8 columns in registers (csrc/overlay.hip).  Kernel names:
 * overlay_kernel<I,O,true | false> with I in rgb, rgba, bgr, bgra, nv12, i420, yuyv and O in rgb, bgr, nv12, i420; true is the vector
 * form (IW a multiple of 8, IH even, src and dst 16-byte aligned), false the byte form with the same bits.  No address is computed
 * from a marker coordinate.  Refused without a launch, the message beginning "overlay_render:": bad arguments, unknown formats or
 * matrix, IH or IW > 16384, odd sizes of a YUV side, N * ceil(IH/2) >= 2^31, M outside 0..8, markers without centres or table,
 * sx or sy not finite, HH or HW outside 1..1024, amax or heat_rgb out of range, zoom outside 1..4, an inset rectangle that does
 * not lie inside the frame.  Not offered: the reference's residual lines from an estimate to the ground truth, its legend text,
 * gaze-ray arrows on the eye image, row pitches, 10-bit surfaces, a gradient.                                                 */
enum { EVE_PIX_RGB = 5, EVE_PIX_RGBA = 6 };
int eve_overlay_render(int in_format, int out_format, int matrix, long long N, int IH, int IW, const uint8_t* src, uint8_t* dst,
                       int M, const float* centres, const uint8_t* marker_valid, const int* marker_table, float sx, float sy,
                       const float* heat /* may be NULL */, int HH, int HW, int heat_rgb, int amax,
                       const uint8_t* inset /* may be NULL */, int ih, int iw, int ix0, int iy0, int zoom, int mirror,
                       const uint8_t* frame_valid /* may be NULL */, eve_stream_t stream);
/* Eye normalisation derived from the head pose, one launch for both eyes of N frames: everything the pipeline reads per frame and
 * eye follows from the face tracker's solvePnP result and the camera matrix.  pose [N][18] float, widened to float64:
 *   (fx, fy, cx, cy,  r0, r1, r2,  t0, t1, t2,  l0, l1, l2,  q0, q1, q2,  focal_norm, distance_norm)
 * fx..cy: the camera matrix of the UNDISTORTED image (the image the warps refer to); r, t: the head's rvec and tvec; l, q: the left
 * and right eye centres in head-model coordinates, in t's length unit; focal_norm (f, patch pixels) and distance_norm (dn): the
 * virtual camera of the OH x OW patch, whose principal point is (OW/2, OH/2).  The procedure is the published one the reference
 * cites for the values it ships precomputed (Zhang et al. 2018, "Revisiting data normalization for appearance-based gaze
 * estimation").  Contract: float64, every operation rounded on its own (no contraction), in exactly this association; every stage
 * is rounded to float32 and the NEXT STAGE CONTINUES FROM THE FLOAT32 VALUES JUST WRITTEN:
 *   1. head_R   th = sqrt((r0*r0 + r1*r1) + r2*r2); th == 0 or an r that is not finite: head_R = I; else k = r / th,
 *               c = cos(th), s = sin(th), v = 1.0 - c, vk_i = v*k_i, sk_i = s*k_i,
 *                   head_R = [[c + vk0*k0, vk0*k1 - sk2, vk0*k2 + sk1], [vk1*k0 + sk2, c + vk1*k1, vk1*k2 - sk0],
 *                             [vk2*k0 - sk1, vk2*k1 + sk0, c + vk2*k2]]                                  -> float32: H
 *   2. o_e      o_i = ((H[i][0]*c0 + H[i][1]*c1) + H[i][2]*c2) + t_i, c = l for the left eye, q for the right   -> float32: o
 *   3. R_e      d = sqrt((o0*o0 + o1*o1) + o2*o2), fw = o / d, hx = H[:, 0]; dn_ = cross(fw, hx), nd = its norm (as d),
 *               down = dn_ / nd; rt_ = cross(down, fw), nr = its norm, right = rt_ / nr;
 *               cross(a, b) = (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0); R_e = rows (right, down, fw)       -> float32: R
 *   4. warp_e   = inv(W) = K R^T diag(1, 1, d / dn) Kn^-1 in closed form (no general inverse): z = d / dn, g = 1.0 / f,
 *               px = (OW * 0.5) / f, py = (OH * 0.5) / f, A[i] = (R[0][i], R[1][i], R[2][i]*z),
 *               B[0] = fx*A[0] + cx*A[2], B[1] = fy*A[1] + cy*A[2], B[2] = A[2] (per column),
 *               warp[i] = (B[i][0]*g, B[i][1]*g, (B[i][2] - B[i][0]*px) - B[i][1]*py)                           -> float32
 *               Not rescaled: its third row times a patch pixel is positive for a head in front of the camera, which the eye
 *               warp kernels require (their Wd > 0).
 *   5. h_e      m_i = (R[i][0]*H[0][2] + R[i][1]*H[1][2]) + R[i][2]*H[2][2] (third column of R_e head_R);
 *               h_e = (asin(min(max(m_1, -1.0), 1.0)), atan2(m_0, m_2))                                         -> float32
 *               SIGN CONVENTION: head_R = Rx(a) seen on the optical axis gives h = (-a, 0), head_R = Ry(b) gives h = (0, b).
 *   6. valid_e  = every one of the 18 inputs finite && fx, fy, f, dn > 0 && o_2 > 0 && d > 0 && nd > 0 && nr > 0 (a NaN fails
 *               its comparison).  An invalid eye gets warp = 0 (the warp kernels then give a black patch), R = I, o = 0, h = 0.
 * o, R, warp and valid are bit-exact functions of the head_R written (only + - * / sqrt remain, each correctly rounded); head_R
 * and h go through sin / cos / asin / atan2 and may sit one float32 ulp from another libm's result.  Layout, eye-major (left, then
 * right), so that each side is a contiguous [N][...] array the next launch reads without a copy: head_R [N][9], o [2][N][3],
 * R [2][N][9], warp [2][N][9], h [2][N][2] float; valid [2][N] uint8.  One thread per (frame, eye); the left eye's thread also
 * writes head_R.  Not offered: gradients, the inverse (rotation matrix -> rvec), skew.  None of it could be compared with the EVE
 * dataset's own {left,right}_{R,W,h,o} values: the dataset is on no machine this library was built on.  Refused without a
 * launch: a null pointer, N < 1 or N >= 2^30, OH or OW outside 1..4096.                                                         */
int eve_eye_pose_normalize(long long N, const float* pose, int OH, int OW, float* head_R, float* o, float* R, float* warp, float* h,
                           uint8_t* valid, eve_stream_t stream);
/* The stages 2..6 above from a head_R and a translation that exist already (eve_face_pose_solve's, say), N frames, both eyes: frame n
 * reads row n / frames_per_row of `rows` [.][row_stride] float, whose first 12 entries are (fx, fy, cx, cy, l0, l1, l2, q0, q1, q2,
 * focal_norm, distance_norm) -- a face rig's head, or one row per frame with frames_per_row = 1 -- head_R [N][9] and head_t [N][3]
 * float.  H = head_R widened, t = head_t widened, and everything from stage 2 on is the contract above, operation for operation
 * (one device function serves both kernels); no head_R is written.  valid_e additionally needs the 12 row entries, head_R and
 * head_t finite and, where valid_in [N] uint8 is not NULL, valid_in[n] != 0.  Outputs and layout as above (o, R, warp, h, valid).
 * Refused without a launch: a null pointer other than valid_in, N < 1 or N >= 2^30, frames_per_row < 1, row_stride < 12, OH or
 * OW outside 1..4096.  Kernel name eye_pose_normalize_rt_kernel.  (Additive: ABI v10.)                                        */
int eve_eye_pose_normalize_rt(long long N, int frames_per_row, const float* rows, int row_stride, const float* head_R, const float* head_t,
                              const uint8_t* valid_in /* may be NULL */, int OH, int OW, float* o, float* R, float* warp, float* h,
                              uint8_t* valid, eve_stream_t stream);
/* Head pose from face landmarks: a weighted perspective-n-point solve for S sequences of T frames, in place of one cv2.solvePnP per
 * frame on the host.  One wavefront per sequence walks its frames in time order, each warm-started from the one before.
 *   landmarks [S][T][L][landmark_cols] float, landmark_cols 2 or 3: pixel (u, v[, w]) in the UNDISTORTED image that fx..cy describe;
 *             w is a confidence, 1.0 without the column; a point is used iff w > 0.  4 <= L <= 68.
 *   rig       [S][12 + 3L] float, one row per sequence: (fx, fy, cx, cy, left eye centre, right eye centre, focal_norm,
 *             distance_norm, X_0 .. X_{L-1}), the model points X_l in the head model's frame and length unit.  Entries 4..11 are
 *             only checked for being finite here; eve_eye_pose_normalize_rt reads them (rows = rig, row_stride = 12 + 3L).
 *   lengths   NULL or [S] int, clamped to 0..T: frames f >= lengths[s] are not solved, are reported invalid and leave the carried
 *             pose alone.
 *   state     NULL or [S][13] double = (R row-major, t, has_pose), read and written in place: frame 0 starts from it where
 *             has_pose != 0 and reset[s] == 0.  Afterwards (R, t, 1.0) of the last solved frame if that was valid, (I, 0, 0.0) if it
 *             was not or if reset[s] != 0 and no frame was solved; untouched if nothing was solved and no reset was flagged.
 *   reset     NULL or [S] int (read only).
 * Contract: float64, every operation rounded on its own (no contraction), only + - * / sqrt, in exactly this association; every
 * sum over the landmarks is taken in landmark order 0 .. L-1 starting from 0.0 (tests/face_pose_ref.py restates all of it):
 *   x = (u - cx) / fx, y = (v - cy) / fy.
 *   eval(R, t), per used point: q_i = (R[i][0]*X0 + R[i][1]*X1) + R[i][2]*X2, P = q + t, iz = 1.0 / P2, px = P0 / P2, py = P1 / P2,
 *     ex = px - x, ey = py - y, a = px*iz, b = py*iz,
 *     Jx = (-(a*q1), iz*q2 + a*q0, -(iz*q1), iz, 0.0, -a),  Jy = (-(iz*q2 + b*q1), b*q0, iz*q0, 0.0, iz, -b)
 *     -- the derivatives of (px, py) by (d, dt) of the update R <- C(d) R, t <- t + dt at d = 0 -- and the 29 sums of
 *     A_ij = w*(Jx_i*Jx_j + Jy_i*Jy_j) for i <= j row-major (21), g_i = w*(Jx_i*ex + Jy_i*ey) (6), cost = w*(ex*ex + ey*ey),
 *     pix = w*((fx*ex)*(fx*ex) + (fy*ey)*(fy*ey)); an unused point adds 0.0 to each.  behind = a used point with not P2 > 0.
 *   Initial pose: the previous frame's float64 solution if that frame was valid, else the carried state as above, else cold:
 *     sw = sum w, (mx, my, MX, MY, MZ) = sum(w*(x, y, X0, X1, X2)) / sw, sl = sum w*((x-mx)*(x-mx) + (y-my)*(y-my)),
 *     sm = sum w*((X0-MX)*(X0-MX) + (X1-MY)*(X1-MY)); not (sl > 0 && sm > 0): invalid; Z = sqrt(sm / sl), R = I,
 *     t = (mx*Z - MX, my*Z - MY, Z - MZ).
 *   lam = 1e-3, accepted = 0, S = eval(R, t); behind or a cost that is not finite: invalid.  Then, repeated:
 *     M = A with M_ii = A_ii + lam*A_ii; Cholesky, thr = 0: for j: s = M_jj; for k < j: s = s - L_jk*L_jk; not s > thr*M_jj: the
 *     pivot fails (invalid); L_jj = sqrt(s); for i > j: s = M_ij; for k < j: s = s - L_ik*L_jk; L_ij = s / L_jj.
 *     y_i = (-g_i - sum_{k<i} L_ik*y_k) / L_ii, d_i = (y_i - sum_{k>i} L_ki*d_k) / L_ii (subtracted one by one, k rising; i falling).
 *     a = 0.5*d[0:3], s = (a0*a0 + a1*a1) + a2*a2, den = 1.0 + s, e = 1.0 - s, the Cayley map (I - [a]x)^-1 (I + [a]x) in closed form
 *       C = [[(e + 2.0*(a0*a0))/den, (2.0*(a0*a1 - a2))/den, (2.0*(a0*a2 + a1))/den],
 *            [(2.0*(a0*a1 + a2))/den, (e + 2.0*(a1*a1))/den, (2.0*(a1*a2 - a0))/den],
 *            [(2.0*(a0*a2 - a1))/den, (2.0*(a1*a2 + a0))/den, (e + 2.0*(a2*a2))/den]],
 *     Rc[i][j] = (C[i][0]*R[0][j] + C[i][1]*R[1][j]) + C[i][2]*R[2][j], tc = t + d[3:6], Sc = eval(Rc, tc).
 *     small = every d_i finite && max|d_i| < 1e-10 * max(1.0, max|t_i|) (t before the update).
 *     Accepted iff every d_i finite && !behind && cost_c <= cost: (R, t, S) = (Rc, tc, Sc), lam = lam / 10.0, ++accepted; small:
 *     converged; else accepted == 32: invalid.  Rejected: small: converged with the pose as it was; else lam = lam * 10.0,
 *     lam > 1e12: invalid.
 *   Converged: one Cholesky of the undamped A with thr = 1e-10; a failed pivot: invalid -- the landmarks do not determine the pose
 *     (collinear model points, say; damping alone would hide that).  reproj_rms = sqrt(pix / sw), in pixels.
 *   Invalid before any of it: a rig entry or a landmark entry (u, v, w; used or not) that is not finite, fx <= 0 or fy <= 0, fewer
 *     than 4 used points.
 * Outputs per frame: head_R [S][T][9] and head_t [S][T][3] float, rounded ONCE from float64; reproj_rms [S][T] float; valid [S][T]
 * uint8.  An invalid frame has head_R = I, head_t = 0, reproj_rms = 0 and the next frame starts cold.  The carried state stays
 * float64, so T frames in one call and the same frames in several calls through `state` give the same bits.  The Cayley update
 * keeps R orthogonal up to rounding (about 1e-16 per accepted step); it is not re-orthonormalised.  Each frame of a sequence
 * depends on the one before: the launch takes T times one frame's latency, S sequences side by side.  Kernel name
 * face_pose_solve_kernel.  Refused without a launch: S < 1, T < 1, S * T >= 2^31, L outside 4..68, landmark_cols other than 2 or 3,
 * a null landmarks, rig or output pointer.  Landmarks of a distorted image and a loss against outliers: eve_face_pose_solve_ex
 * below.  Not offered: RANSAC, an rvec, gradients, per-frame camera matrices; a planar model runs, but which of its two minima is
 * found is not promised.  (Additive: ABI v10.)                                                                                 */
int eve_face_pose_solve(long long S, int T, int L, int landmark_cols, const float* landmarks, const float* rig,
                        const int* lengths /* may be NULL */, double* state /* may be NULL */, const int* reset /* may be NULL */,
                        float* head_R, float* head_t, float* reproj_rms, uint8_t* valid, eve_stream_t stream);
/* The raw pixels of a camera with lens distortion -> the normalised points (x, y) of the undistorted image, one thread per point:
 * what cv2.undistortPoints does on the host, by Newton's method instead of five fixed-point passes.
 *   points [N][2] float: raw pixel (u, v).   lens: float rows (fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6) as for
 *   eve_eye_warp_lens_u8_to_nchw; lens_stride 12: [N][12], one row per point; 0: [1][12], one row for all.
 *   xy [N][2] double: (x, y); the pixel of the undistorted image is (fx*x + cx, fy*y + cy).   ok [N] uint8.
 * Contract: float64, every operation rounded on its own (no contraction), only + - * /, in exactly this association
 * (tests/face_pose_raw_ref.py restates it):
 *   xd = (u - cx) / fx, yd = (v - cy) / fy.  A row whose eight coefficients are all +-0: x = xd, y = yd, no iteration (the warp
 *   kernels' rule).  Else from (x, y) = (xd, yd), at most 12 times:
 *     xx = x*x, yy = y*y, xy = x*y, r2 = xx + yy,
 *     N = ((k3*r2 + k2)*r2 + k1)*r2 + 1.0, D = ((k6*r2 + k5)*r2 + k4)*r2 + 1.0, rad = N / D, a = xy + xy,
 *     gx = (x*rad + p1*a) + p2*(r2 + (xx + xx)), gy = (y*rad + p1*(r2 + (yy + yy))) + p2*a       -- the warp kernels' forward model --
 *     N' = ((3.0*k3)*r2 + 2.0*k2)*r2 + k1, D' = ((3.0*k6)*r2 + 2.0*k5)*r2 + k4, rp = (N' - rad*D') / D, tw = rp + rp,
 *     j00 = ((rad + xx*tw) + 2.0*(p1*y)) + 6.0*(p2*x), j01 = (xy*tw + 2.0*(p1*x)) + 2.0*(p2*y),
 *     j11 = ((rad + yy*tw) + 6.0*(p1*y)) + 2.0*(p2*x)                                            -- the Jacobian, j10 = j01 --
 *     ex = gx - xd, ey = gy - yd, det = j00*j11 - j01*j01, dx = (j11*ex - j01*ey) / det, dy = (j00*ey - j01*ex) / det;
 *     dx or dy not finite: unusable.  x = x - dx, y = y - dy; max(|dx|, |dy|) <= 4e-15 * max(1.0, |x|, |y|): done.
 *   Twelve steps without that: unusable.  D once more at the result (xx, yy, r2, D as above); not D > 0: unusable.
 * ok = 0 and xy = (0, 0): an unusable point, a point that is not finite, a lens row with an entry that is not finite or fx <= 0 or
 * fy <= 0.  Beyond the fold-back radius of a barrel polynomial the forward model is not injective and which pre-image is found is
 * not promised -- the pixel warp's unguarded case.  Measured on four lenses over +-0.64 x +-0.36: 5 steps at most, 4.4e-16 from
 * the truth.  Kernel name undistort_points_kernel.  Refused without a launch: N < 1, a null pointer, lens_stride other than 0 or 12.
 * Not offered: fisheye, thin-prism and tilt models.  (Additive: ABI v10.)                                                        */
int eve_undistort_points(long long N, const float* points, const float* lens, long long lens_stride, double* xy, uint8_t* ok,
                         eve_stream_t stream);
/* eve_face_pose_solve with two optional additions: landmarks of the RAW frame of a camera with lens distortion, and a Huber loss
 * against landmarks that are confidently wrong.  Arguments, outputs, the carried state and every refusal as there, plus
 *   lens      NULL, or [S*T][12] float, one row per frame as above: landmarks are then raw pixels.  When a frame's landmarks are
 *             loaded each is undistorted by the iteration above and the solve continues from (x, y) directly; the rig's fx .. cy
 *             keep their roles (the pix column, the normalisation that follows).  An unusable point is dropped -- w = 0, x = y =
 *             0.0, not used -- and a row that is not usable makes the frame invalid, like a landmark that is not finite.  `used`,
 *             the count of at least 4 and sw follow from the points that survived.
 *   huber_px  k; <= 0: no loss.  k > 0 (pixels): per used point, from ex, ey, Jx, Jy of eval,
 *               p2 = (fx*ex)*(fx*ex) + (fy*ey)*(fy*ey), r = sqrt(p2), inlier iff not r > k, s = 1.0 for an inlier, else k / r, ws = w*s,
 *               A_ij = ws*(Jx_i*Jx_j + Jy_i*Jy_j), g_i = ws*(Jx_i*ex + Jy_i*ey), cost = w*(inlier ? p2 : k*((r + r) - k)) -- the
 *               Huber cost in pixels^2; the accept test only compares costs -- pix = w*p2, and a 30th sum of 1.0 per inlier.
 *             The iteration, the damping, small, the cap of 32 accepted steps and the observability Cholesky (on the weighted A)
 *             are unchanged; a frame that converges with fewer than 4 inliers is invalid.  Without the loss the 29 sums stand.
 *   inliers   [S][T] uint8: the 30th sum with the loss, the number of used points without, 0 on an invalid frame.
 * reproj_rms keeps its meaning: sqrt(pix / sw) over all used points, weighted by w.  lens NULL and huber_px <= 0 give
 * eve_face_pose_solve's bits; a lens row with zero coefficients and the rig's intrinsics too.  tests/face_pose_raw_ref.py restates
 * the contract.  Measured (k = 3, L = 68, 1 px noise, 7 / 14 landmarks moved 30..80 px, 40 cases each): rotation error 0.35 / 0.39
 * degrees median and 1.17 / 1.05 at most, where the plain solve has 3.06 / 4.02 and 10.4 / 10.8.  Not promised: L = 6 with an
 * outlier.  Kernel name face_pose_solve_ex_kernel.  Refused without a launch, beyond the plain refusals: a null inliers, a NaN
 * huber_px.  Not offered: RANSAC, a gradient, per-frame rigs.  (Additive: ABI v10.)                                               */
int eve_face_pose_solve_ex(long long S, int T, int L, int landmark_cols, const float* landmarks, const float* rig,
                           const float* lens /* may be NULL */, double huber_px, const int* lengths /* may be NULL */,
                           double* state /* may be NULL */, const int* reset /* may be NULL */, float* head_R, float* head_t,
                           float* reproj_rms, uint8_t* valid, uint8_t* inliers, eve_stream_t stream);

/* Per-person gaze calibration: the constant offset kappa = (pitch, yaw) of a person's visual axis against the optical axis EyeNet
 * sees, in the offset model eve_gaze_to_pog applies when it is given a kappa row.  Two launches: collect, fit.  Float64, every
 * operation rounded on its own (no contraction); tests/calib_ref.py restates both in numpy.
 *
 * eve_calib_append: B streams x T frames x E eyes (E = 1, or 2 = left, right).  One THREAD per sequence q = b*E + e walks frames
 * f = 0 .. T-1 in order (n = b*T + f), reduces every usable frame to a row of 16 doubles and appends it to the sequence's store:
 *   g [E][B*T][2], origin [E][B*T][3], R [E][B*T][9] float, eye-major; head_R [B*T][9], inv_cam [B*T][16], ppm [B*T][2], target
 *   [B*T][2] float (the target in screen pixels), shared by the eyes.  valid [B*T] uint8, lengths [B] int (clamped to 0 .. T),
 *   eye_valid [B*T][E] uint8: each may be NULL (all frames, T frames, both eyes).
 *   samples [B*E][C][16] double, count [B*E] int, dropped [B*E] int: read and UPDATED IN PLACE.
 * The row, inputs widened to double first: (p, y) = g; v = (cos p sin y, sin p, cos p cos y); u = Rh^T v, each entry
 * (a*b + c*d) + e*f, divided by sqrt((u0*u0 + u1*u1) + u2*u2); c0 = sqrt(ux*ux + uz*uz), s0 = uy, s1 = ux / c0, c1 = uz / c0;
 * Q = Ry Rx = [[c1, -(s1*s0), s1*c0], [0, c0, s0], [-s1, -(c1*s0), c1*c0]] (the rotation eve_gaze_to_pog applies to the kappa
 * vector); M = T3 (R^T (Rh Q)), T3 the upper-left 3 x 3 of inv_cam, every 3 x 3 product entry (a0*b0 + a1*b1) + a2*b2, the
 * products taken in the order the brackets show; A = -M; e_i = ((T_i0*o0 + T_i1*o1) + T_i2*o2) + T_i3; m = target / ppm.
 *   row = A (9, row-major), e (3), m (2), 1.0 (the weight), 0.0 (reserved)
 * With k(kappa) = (cos kp sin ky, sin kp, cos kp cos ky) and d = A k the modelled point of gaze in millimetres is
 * (e0 - e2*d0/d2, e1 - e2*d1/d2): what eve_gaze_to_pog computes with that kappa, without its 1e-7 guards and its screen clamp.
 * A frame is usable iff valid[n], f < lengths[b], eye_valid[n][e], every input and every entry of the row is finite, c0 > 0 and
 * -e2 / A[8] > 0 (the target lies in front of the eye at kappa = 0).  A usable frame goes to row count[q] and count[q] grows; with
 * count[q] == C the sample is dropped and dropped[q] grows.  No atomics: the store is a deterministic function of the calls.
 * Kernel name calib_append_kernel.  Refused without a launch: a null pointer, B, T or C < 1, E other than 1 or 2, index ranges past
 * 31 bits.
 *
 * eve_calib_fit: S sequences, one wavefront each: Levenberg-Marquardt on kappa from (0, 0), always, over rows 0 .. n-1 of
 * samples [S][C][16], n = count[q] clamped to 0 .. C (count NULL: C).  A row whose weight w (entry 14) is not > 0 is absent.
 *   eval(kappa): k as above, a = dk/dkp = (-(sin kp sin ky), cos kp, -(sin kp cos ky)), (b0, b2) = (cos kp cos ky, -(cos kp sin ky))
 *   (dk/dky; its middle entry is 0).  Per row: d_j = (A_j0*k0 + A_j1*k1) + A_j2*k2, dp_j the same with a, dy_j = A_j0*b0 + A_j2*b2;
 *   z2 = d2*d2; rx = (e0 - e2*(d0/d2)) - m0, ry = (e1 - e2*(d1/d2)) - m1; Jxp = -(e2*((dp0*d2 - d0*dp2)/z2)), Jxy the same with dy,
 *   Jyp, Jyy with index 1 for 0; r2 = rx*rx + ry*ry.  Without a loss ws = w, cost = w*r2, inl = 1.  With huber_mm = h > 0:
 *   r = sqrt(r2), inlier iff not r > h, ws = w*(inlier ? 1 : h/r), cost = w*(inlier ? r2 : h*((r + r) - h)), inl = inlier.
 *   The 9 contributions: ws*(Jxp*Jxp + Jyp*Jyp), ws*(Jxp*Jxy + Jyp*Jyy), ws*(Jxy*Jxy + Jyy*Jyy), ws*(Jxp*rx + Jyp*ry),
 *   ws*(Jxy*rx + Jyy*ry), cost, w*r2, inl, 1.0.
 *   SUMMATION ORDER: lane l starts 9 partial sums at 0.0 and adds its rows l, l + 64, l + 128, ... in that order; then column j is
 *   summed from 0.0 over the partial sums of lanes 0, 1, .. 63 in that order.  -> S[0..8], the same bits in every lane; nothing
 *   depends on timing, so two launches on one store give the same bits.
 *   used = S[8].  Fails at once when used < min_samples or the first cost is not finite.  lam = 1e-3; then, at most 64 evaluations
 *   in all: factor [[S0 + lam*S0, S1], [S1, S2 + lam*S2]] by Cholesky (l00 = sqrt(m00), l10 = m01/l00, s = m11 - l10*l10, l11 =
 *   sqrt(s); fails unless m00 > 0 and s > 0), y0 = -S3/l00, y1 = (-S4 - l10*y0)/l11, d1 = y1/l11, d0 = (y0 - l10*d1)/l00;
 *   small = d finite and max(|d0|, |d1|) <= 1e-12; evaluate at kappa + d; if d is finite and its cost <= the current cost: accept,
 *   lam /= 10, converged if small, failed at the 32nd accepted step otherwise; else converged if small; else lam *= 10, failed
 *   when lam > 1e12.  After convergence the undamped matrix must factor with m00 > 0 and s > 1e-10*m11, and sqrt(kp*kp + ky*ky)
 *   must not exceed 0.35 rad (20 degrees, four times any physiological offset: a divergence guard).
 * Outputs per sequence: kappa [S][2] double, rms_mm [S] double = sqrt(S6 / S8), used [S] int, inliers [S] int = S7, ok [S] uint8.
 * Where ok is 0, kappa, rms_mm and inliers are 0 and used is still reported.  select [S] uint8 or NULL: a sequence with select[q]
 * == 0 is not fitted (ok = 0, used = 0).  kappa_store [S][2] float and ok_store [S] uint8 (both or neither): where ok, and only
 * there, kappa_store[q] = (float)kappa and ok_store[q] = 1 -- a failed fit leaves what that eye had.  A stream counts as
 * calibrated where the flags of both its eyes are set.  Kernel name calib_fit_kernel.  Refused without a launch: a null pointer,
 * S or C < 1, min_samples < 1, a NaN huber_mm, one store without the other.  Not offered: per-sample weights (entry 14 is 1.0, or
 * 0.0 for an absent row), a gradient; the residual that depends on the position on the screen is eve_screen_calib_*'s, below.
 * (Additive: ABI v10.)                                                                                                            */
int eve_calib_append(long long B, int T, int E, const float* g, const float* head_R, const float* origin, const float* R,
                     const float* inv_cam, const float* ppm, const float* target, const uint8_t* valid /* may be NULL */,
                     const int* lengths /* may be NULL */, const uint8_t* eye_valid /* may be NULL */, int C, double* samples, int* count,
                     int* dropped, eve_stream_t stream);
int eve_calib_fit(long long S, int C, const double* samples, const int* count /* may be NULL */, const uint8_t* select /* may be NULL */,
                  double huber_mm, int min_samples, double* kappa, double* rms_mm, int* used, int* inliers, uint8_t* ok,
                  float* kappa_store /* may be NULL */, uint8_t* ok_store /* may be NULL */, eve_stream_t stream);

/* Screen-space gaze calibration: the residual that depends on the position on the screen -- a camera-to-screen transform a little
 * off, a head-pose dependent bias, a cornea that is not the average one: what a tracker's five- or nine-dot procedure removes --
 * as a low-order map of the pipeline's OUTPUT point.  With W x H the screen in pixels and (x, y) the output point in pixels:
 *   u = (x + x) / W - 1, v = (y + y) / H - 1, phi = (1, u, v, u*u, u*v, v*v) cut to K terms
 *   kind 0: no map; 1 'offset' K = 1; 2 'affine' K = 3; 3 'quadratic' K = 6 (any other kind byte is read as 0)
 *   the correction in MILLIMETRES on the screen, axis a = x, y:  s_a = C[a][0];  s_a = s_a + phi_k * C[a][k], k = 1 .. K-1
 *   the corrected pixel  x' = x + s_x * ppm_x, clamped by x' < 0 ? 0 : (x' > W ? W : x') (a NaN stays a NaN), rounded to float
 * Coefficients are double [2][6] per stream (axis, term), unused terms 0.  Three launches: collect, fit (or evaluate), apply.
 * Float64, every operation rounded on its own (no contraction); tests/screen_calib_ref.py restates all three in numpy.
 *
 * eve_screen_calib_append: B streams x T frames.  One THREAD per stream walks frames f = 0 .. T-1 in order (n = b*T + f), reduces
 * every usable frame to a row of 12 doubles and appends it to the stream's store (eve_calib_append's scheme without the eye axis):
 *   pog [B*T][2] (the output point BEFORE this map, pixels), origin [B*T][3] (o), inv_cam [B*T][16], ppm [B*T][2], target [B*T][2]
 *   (pixels) float.  valid [B*T] uint8, lengths [B] int (clamped to 0 .. T), frame_valid [B*T] uint8 (a masked step's valid): each
 *   may be NULL.  samples [B][C][12] double, count [B] int, dropped [B] int: read and UPDATED IN PLACE.
 * The row, inputs widened to double first:
 *   u, v as above; xm = x / ppm_x, ym = y / ppm_y; tmx = tx / ppm_x, tmy = ty / ppm_y;
 *   e_i = ((T_i0*o0 + T_i1*o1) + T_i2*o2) + T_i3, i = 0 .. 2 (the eye in screen coordinates); 1.0 (the weight); 0.0, 0.0 (reserved)
 * A frame is usable iff valid[n], f < lengths[b], frame_valid[n], every input and every entry of the row is finite, both ppm > 0
 * and e_2 != 0.  A usable frame goes to row count[b] and count[b] grows; with count[b] == C it is dropped and dropped[b] grows.
 * Kernel name screen_calib_append_kernel.  Refused without a launch: a null pointer, B, T or C < 1, W or H not > 0, index ranges
 * past 31 bits.
 *
 * eve_screen_calib_fit: S streams, one wavefront each, over rows 0 .. n-1 of samples [S][C][12], n = count[q] clamped to 0 .. C
 * (count NULL: C).  A row whose weight w (entry 9) is not > 0 is absent.  mode 0 fits a map of `kind` (1 .. 3); mode 1 evaluates
 * the STORED map (coef_store, kind_store) and solves nothing.
 *   One pass at coefficients C, per row: p_a by the sum above; ex = tmx - xm, ey = tmy - ym; rx = p_x - ex, ry = p_y - ey;
 *   r2 = rx*rx + ry*ry, r = sqrt(r2).  Without a loss ws = w, cost = w*r2, inl = 1.  With huber_mm = h > 0: inlier iff not r > h,
 *   ws = w*(inlier ? 1 : h/r), cost = w*(inlier ? r2 : h*((r + r) - h)), inl = inlier (eve_calib_fit's definitions).
 *   The contributions: (ws*phi_i)*phi_j for i = 0 .. K-1, j = 0 .. i (the lower triangle of G); (ws*phi_i)*ex (bx); (ws*phi_i)*ey
 *   (by); cost, w*r2, w*r, inl, 1.0.
 *   SUMMATION ORDER: lane l starts its partial sums at 0.0 and adds its rows l, l + 64, l + 128, ... in that order; then every
 *   column is summed from 0.0 over the partial sums of lanes 0, 1, .. 63 in that order: the same bits in every lane.
 *   Solve: Cholesky of G row by row -- for j = 0 .. K-1: s = G_jj; s = s - L_jk*L_jk, k = 0 .. j-1; the pivot fails unless
 *   G_jj > 0 and s > 1e-10*G_jj; L_jj = sqrt(s); for i > j: t = G_ij; t = t - L_ik*L_jk, k = 0 .. j-1; L_ij = t / L_jj.  Per axis:
 *   y_i = (b_i - sum_{k<i} L_ik*y_k) / L_ii for i = 0 .. K-1, then C_i = (y_i - sum_{k>i} L_ki*C_k) / L_ii for i = K-1 .. 0, each
 *   sum subtracted term by term in ascending k.
 *   Schedule: used = the sum of 1.0.  From C = 0: pass, solve -> the solution without a loss.  With huber_mm > 0 repeat (pass at
 *   the current C, solve) until every new coefficient is finite and max |C_new - C_old| <= 1e-6 mm; failed after the 64th solve.
 *   The final pass at the solution takes, per present row: w*r2, w*r, inl, 1.0 and w*deg as ordered sums; the maxima of r and of
 *   the correction's length sqrt(p_x*p_x + p_y*p_y) (each from 0.0 by m = r > m ? r : m, so independent of the order); and the
 *   same sums and maximum at C = 0 (p_x = p_y = 0.0): the error of the uncorrected point.  deg is the angle at the eye between
 *   a = ((xm + p_x) - e0, (ym + p_y) - e1, -e2), towards the corrected point, and b = (tmx - e0, tmy - e1, -e2), towards the target:
 *     a x b = (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0), |a x b| = sqrt((c0*c0 + c1*c1) + c2*c2), a . b = (a0*b0 + a1*b1) + a2*b2,
 *     deg = atan2(|a x b|, a . b) * 57.29577951308232
 *   The fit fails (ok = 0) when used < max(min_samples, K), the first cost is not finite, a pivot fails (dots on one line for
 *   'affine'; fewer than six distinct dot positions, or a 5 x 1 row, for 'quadratic'), no convergence, or the longest correction
 *   over the present rows exceeds max_shift_mm (a divergence guard, as 0.35 rad is for kappa).  Mode 1 is the final pass alone
 *   (no loss; inliers = used; ok iff used >= 1); a stored map of kind 0 has p = 0 and reports the raw numbers in both sets.
 * Outputs per stream: coef [S][2][6] double; report [S][8] double = rms_mm = sqrt(sum w*r2 / used), mean_mm = sum w*r / used,
 * max_mm, mean_deg = sum w*deg / used, then the same four at C = 0 (rms_mm_raw, mean_mm_raw, max_mm_raw, mean_deg_raw); used,
 * inliers, solves [S] int; ok [S] uint8.  Where ok is 0 every output but used is 0.  select [S] uint8 or NULL: a stream with
 * select[q] == 0 is not touched (ok = 0, used = 0).  coef_store [S][2][6] double and kind_store [S] uint8 (both or neither; mode 1
 * needs them): in mode 0, where ok and only there, coef_store[q] = coef and kind_store[q] = kind -- a failed fit leaves the map
 * the stream had; mode 1 reads them and writes neither.  The two degree outputs go through atan2, whose last bits belong to the
 * maths library; everything else is fixed to the bit.  Kernel name screen_calib_fit_kernel.  Refused without a launch: a null
 * pointer, S or C < 1, a mode other than 0 or 1, one store without the other, mode 1 without stores, and in mode 0 a kind outside
 * 1 .. 3, min_samples < 1, a NaN huber_mm, max_shift_mm not > 0.
 *
 * eve_screen_calib_apply: one thread per frame n of B*T; stream b = n / T reads coef [B][2][6] and kind [B]: px_out [B*T][2] float
 * from px_in [B*T][2] and ppm [B*T][2] float by the expressions at the top; a stream of kind 0 gets its input BITS.  Kernel name
 * screen_calib_apply_kernel.  Refused without a launch: a null pointer, B or T < 1, W or H not > 0, index ranges past 31 bits.
 * Not offered: per-sample weights from the caller (entry 9 is 1.0, or 0.0 for an absent row), cubic or higher models, automatic
 * recalibration, a gradient.  (All three additive: ABI v10.)                                                                      */
int eve_screen_calib_append(long long B, int T, const float* pog, const float* origin, const float* inv_cam, const float* ppm,
                            const float* target, const uint8_t* valid /* may be NULL */, const int* lengths /* may be NULL */,
                            const uint8_t* frame_valid /* may be NULL */, double W, double H, int C, double* samples, int* count,
                            int* dropped, eve_stream_t stream);
int eve_screen_calib_fit(long long S, int C, const double* samples, const int* count /* may be NULL */,
                         const uint8_t* select /* may be NULL */, int mode, int kind, double huber_mm, int min_samples, double max_shift_mm,
                         double* coef, double* report, int* used, int* inliers, int* solves, uint8_t* ok,
                         double* coef_store /* may be NULL */, uint8_t* kind_store /* may be NULL */, eve_stream_t stream);
int eve_screen_calib_apply(long long B, int T, const float* px_in, const float* ppm, const double* coef, const uint8_t* kind, double W,
                           double H, float* px_out, eve_stream_t stream);

/* Gaze filtering and fixation / saccade events: the post-processing every consumer of an eye tracker runs on the per-frame point of
 * gaze -- a one-euro filter (Casiez et al. 2012), the angular velocity of the gaze vector, velocity-threshold labels (I-VT), the
 * running fixation and a store of completed fixations -- for B streams x T frames, with the state carried in `state` from one call
 * to the next.  Float64, every operation rounded on its own (no contraction), in the order written here; tests/gaze_events_ref.py
 * restates it in numpy.  One wavefront per stream, passes of 64 frames; the bits do not depend on that structure.
 *   pog [B*T][2] (the source point of gaze, screen pixels), origin [B*T][3], inv_cam [B*T][16], ppm [B*T][2] float;
 *   frame_time [B*T] double seconds or NULL (then t = ticks / fps); valid [B*T] uint8, lengths [B] int (clamped to 0 .. T), reset [B]
 *   int, flush [B] int: each may be NULL (all frames, T frames, no reset, no flush).
 *   state [B][32] double, store [B][F][8] double, count [B] and dropped [B] int: read and UPDATED IN PLACE.
 * The state row: 0 ticks (the delivered frames since the last reset), 1 has_prev, 2 t_prev (the last sample's time), 3-4 its raw
 * (x, y), 5-6 its filtered (x, y), 7-8 the filtered derivative (px/s), 9-11 its gaze vector, 12 fix_open, 13 the open fixation's id,
 * 14 next_id (the ids handed out so far), 15-16 the open fixation's first sample (x0, y0), 17 n, 18 sum(x - x0), 19 sum(y - y0),
 * 20 sum((x - x0)^2 + (y - y0)^2), 21 t_start, 22 t_last, 23-31 reserved (0).
 * A stream with reset[b] != 0 first closes its open fixation (below) and zeroes its row except entry 14.  Then frames f = 0 ..
 * lengths[b] - 1 are walked in order.  t = frame_time[b][f], or (ticks + f) / fps.  With (x, y) = pog, (sx, sy) = ppm widened to double
 * and e_i = ((T_i0*o0 + T_i1*o1) + T_i2*o2) + T_i3 the frame is a SAMPLE iff valid[b][f], t, x, y, sx, sy, o and all 16 entries of
 * inv_cam are finite, e_2 != 0, and (has_prev == 0 or t > t_prev).  Any other frame changes nothing: event 0, id -1, velocity NaN,
 * PoG_px_filtered = pog as it came, the rest 0 (so do the frames from lengths[b] on).  For a sample, dt = t - t_prev and
 *   restart = has_prev == 0 or dt > max_gap_s: the filtered value is (x, y) itself, the derivative 0, no velocity (NaN), event 0, and
 *   the open fixation is closed;
 *   otherwise, with alpha(fc) = 1 / (1 + (1 / (6.283185307179586*fc)) / dt): ad = alpha(d_cutoff_hz); dxh = ad*((x - x_prev)/dt) +
 *   (1 - ad)*dxh_prev (x_prev the previous sample's RAW x, as in the authors' implementation); ax = alpha(min_cutoff_hz +
 *   beta*fabs(dxh)); xh = ax*x + (1 - ax)*xh_prev; y alike and on its own.
 *   v = (p_x/sx - e_0, p_y/sy - e_1, -e_2) with p the filtered point, or the raw one with velocity_from_raw; the state takes t, (x, y),
 *   (xh, yh), (dxh, dyh) and v.  Unless restart: c = v_prev x v (c0 = p1*v2 - p2*v1, ...), angle = atan2(sqrt((c0*c0 + c1*c1) + c2*c2),
 *   (p0*v0 + p1*v1) + p2*v2), velocity = angle * 57.29577951308232 / dt (deg/s).  velocity > saccade_deg_s: event 2, and the open
 *   fixation is closed (at its previous sample).  Otherwise event 1: where none is open one opens -- id = next_id, next_id += 1, (x0, y0)
 *   = the raw (x, y), the sums 0, t_start = t -- and then n += 1, the three sums take dx = x - x0 and dy = y - y0 (the third dx*dx +
 *   dy*dy), t_last = t; fixation_id = id, fixation_px = (x0 + sdx/n, y0 + sdy/n), fixation_ms = 1000*(t - t_start), fixating = t -
 *   t_start >= min_fixation_s.
 * Closing: fix_open = 0, and where t_last - t_start >= min_fixation_s the row (id, t_start, t_last, n, x0 + mx, y0 + my, rms_px, 0.0),
 * mx = sdx/n, my = sdy/n, rms_px = sqrt of sd2/n - (mx*mx + my*my) where that is > 0, else 0, goes to store[b][count[b]] and count[b]
 * grows; with count[b] == F it is dropped and dropped[b] grows.  After the frames ticks += lengths[b], and a stream with flush[b] != 0
 * closes its open fixation.  T = 0 is a call that only resets and flushes (the frame pointers may then be NULL).
 * Outputs per frame, float values rounded from double once: filtered [B*T][2] float, velocity [B*T] float, event [B*T] uint8,
 * fixation_id [B*T] int, fixation_px [B*T][2] float, fixation_ms [B*T] float, fixating [B*T] uint8.  Kernel name gaze_events_kernel.
 * Refused without a launch: a null state, store or counter, with T > 0 a null frame input or output, B or F < 1, T < 0, index ranges
 * past 31 bits, fps not a finite number > 0 where frame_time is NULL and T > 0, a cutoff, threshold or time that is not a finite
 * number > 0, a beta that is not a finite number >= 0.  Not offered: dispersion (I-DT) classifiers, windowed velocity, merging of
 * adjacent fixations, a blink class, per-eye events, a gradient (smooth pursuit: eve_gaze_pursuits).  (Additive: ABI v10.)        */
int eve_gaze_events(long long B, int T, const float* pog, const float* origin, const float* inv_cam, const float* ppm,
                    const double* frame_time /* may be NULL */, const uint8_t* valid /* may be NULL */, const int* lengths /* may be NULL */,
                    const int* reset /* may be NULL */, const int* flush /* may be NULL */, double fps, double min_cutoff_hz, double beta,
                    double d_cutoff_hz, int velocity_from_raw, double saccade_deg_s, double min_fixation_s, double max_gap_s, double* state,
                    int F, double* store, int* count, int* dropped, float* filtered, float* velocity, uint8_t* event, int* fixation_id,
                    float* fixation_px, float* fixation_ms, uint8_t* fixating, eve_stream_t stream);

/* The same launch, which also hands out what it computes on the way: eve_gaze_events' arguments, arithmetic, state row and store,
 * bit for bit (both entries launch gaze_events_kernel), plus three outputs, each of which may be NULL, written for every frame f < T:
 *   sample [B*T] uint8: 0 the frame is no sample (the frames from lengths[b] on included), 1 a sample that restarts the chain (the
 *   first after a reset, or more than max_gap_s after the last), 2 a sample chained to the one before (it has a velocity and a label);
 *   sample_time [B*T] double: the t the launch used for the frame; gaze_vector [B*T][3] double: v, the vector behind the velocity.
 *   Both are 0.0 where sample is 0.
 * What eve_gaze_saccades consumes.  (Additive: ABI v10.)                                                                            */
int eve_gaze_events_ex(long long B, int T, const float* pog, const float* origin, const float* inv_cam, const float* ppm,
                       const double* frame_time /* may be NULL */, const uint8_t* valid /* may be NULL */, const int* lengths /* may be NULL */,
                       const int* reset /* may be NULL */, const int* flush /* may be NULL */, double fps, double min_cutoff_hz, double beta,
                       double d_cutoff_hz, int velocity_from_raw, double saccade_deg_s, double min_fixation_s, double max_gap_s, double* state,
                       int F, double* store, int* count, int* dropped, float* filtered, float* velocity, uint8_t* event, int* fixation_id,
                       float* fixation_px, float* fixation_ms, uint8_t* fixating, uint8_t* sample /* may be NULL */,
                       double* sample_time /* may be NULL */, double* gaze_vector /* may be NULL */, eve_stream_t stream);

/* Saccades as events: the runs of saccade frames that eve_gaze_events labels, cut into events with amplitude, duration, peak and mean
 * velocity and the fixations on either side, for B streams x T frames, with the state carried in `state`, the tallies in `table` and
 * the accepted saccades in `store` from one call to the next.  Float64, every operation rounded on its own (no contraction), in the
 * order written here; tests/saccade_ref.py restates it in numpy.  One wavefront per stream, passes of 64 frames, the closings'
 * atan2 across the lanes; the bits do not depend on that structure.
 *   sample [B*T] uint8, sample_time [B*T] double, gaze_vector [B*T][3] double: eve_gaze_events_ex's outputs of the same frames;
 *   point [B*T][2] float: the point the velocity is from (the filtered point, or the source with velocity_from_raw), widened to
 *   double; event [B*T] uint8, velocity [B*T] float, fixation_id [B*T] int: that launch's labels; lengths [B] int (clamped to 0 ..
 *   T) and reset [B] int: each may be NULL (T frames, no reset).
 *   state [B][32] double, table [B][16] double, store [B][S][16] double, count [B] and dropped [B] int: read and UPDATED IN PLACE.
 * The state row, an all-zero row being a fresh stream: 0 has_prev, 1-8 the carried previous sample -- 1 its time, 2-4 its gaze
 * vector, 5-6 its point, 7 its event, 8 its fixation_id --, 9 open, 10 the open saccade's id, 11 next_id (the ids handed out so far),
 * 12 t_onset, 13-15 the onset's gaze vector, 16-17 the onset's point, 18 n (its saccade frames), 19 peak, 20 missing, 21
 * prev_fixation_id, 22-31 reserved (0).
 * A stream with reset[b] != 0 first aborts its open saccade (table.aborted += 1, nothing stored) and zeroes its row except entry 11;
 * the table stays.  Then frames f = 0 .. lengths[b] - 1 are walked in order (the later ones: id -1, ms 0, nothing moves).
 *   sample 0: where a saccade is open, missing += 1.  Nothing else moves; id -1, ms 0.
 *   sample 1, or sample 2 with an event other than 1 and 2 (which eve_gaze_events never writes): an open saccade is aborted.
 *   sample 2, event 2: where none is open, has_prev != 0 and the carried sample's event is not 2 (it is only after a reset of this row
 *   alone: nothing opens in the middle of a run), one opens -- id = next_id, next_id += 1 (accepted later or not), t_onset, the
 *   onset's vector and point = the carried sample's, prev_fixation_id = its fixation_id where its event was 1, else -1, n = peak =
 *   missing = 0.  Where one is open: n += 1, peak = velocity (widened) where that is > peak, saccade_id = id, saccade_ms = 1000 * (t -
 *   t_onset).
 *   sample 2, event 1: an open saccade closes.  Its landing is the carried sample (the last saccade frame): with p the onset's vector
 *   and v the landing's, c = p x v (c0 = p1*v2 - p2*v1, ...), amplitude = atan2(sqrt((c0*c0 + c1*c1) + c2*c2), (p0*v0 + p1*v1) + p2*v2)
 *   * 57.29577951308232 (deg), duration = t_landing - t_onset, mean = amplitude / duration, next_fixation_id = this frame's
 *   fixation_id.  The first that holds decides: missing > max_missing: table.interrupted += 1; duration > max_duration_s: long;
 *   duration < min_duration_s: short; not (amplitude >= min_amplitude_deg): small; else it is accepted: table.accepted += 1, sum_amp
 *   += amplitude, sum_amp2 += amplitude*amplitude, sum_peak += peak, sum_amp_peak += amplitude*peak, sum_dur += duration, sum_amp_dur
 *   += amplitude*duration, max_amp and max_peak take a larger value, and the row (id, t_onset, t_landing, n, x0, y0, x1, y1,
 *   amplitude_deg, peak_deg_s, mean_deg_s, prev_fixation_id, next_fixation_id, missing, 0, 0) goes to store[b][count[b]] and count[b]
 *   grows; with count[b] == S it is dropped and dropped[b] grows.
 *   After every sample (1 or 2) it becomes the carried sample: has_prev = 1, its time, vector, point, event (0 for sample 1) and id.
 * The table row: 0 accepted, 1 sum_amp, 2 sum_amp2, 3 sum_peak, 4 sum_amp_peak, 5 sum_dur, 6 sum_amp_dur, 7 max_amp, 8 max_peak,
 * 9 aborted, 10 small, 11 short, 12 long, 13 interrupted, 14-15 reserved (0).  There is no flush: an open saccade has no landing.
 * T = 0 is a call that only resets (the frame pointers may then be NULL).
 * Outputs per frame: saccade_id [B*T] int (-1 outside a saccade), saccade_ms [B*T] float (rounded from double once; 0 outside).
 * Kernel name gaze_saccades_kernel.  Refused without a launch: a null carried buffer, B < 1, T < 0, S < 1, with T > 0 a null frame
 * input or output, index ranges past 31 bits, a threshold that is not finite, min_amplitude_deg < 0, max_duration_s <= 0,
 * min_duration_s < 0, max_missing < 0.  Not offered: direction angles (the endpoints are there), curvature or path length, glissades
 * and post-saccadic oscillation, microsaccades, per-eye saccades, retroactive merging, a gradient (smooth pursuit:
 * eve_gaze_pursuits).  (Additive: ABI v10.)                                                                                         */
int eve_gaze_saccades(long long B, int T, const uint8_t* sample, const double* sample_time, const double* gaze_vector, const float* point,
                      const uint8_t* event, const float* velocity, const int* fixation_id, const int* lengths /* may be NULL */,
                      const int* reset /* may be NULL */, double min_amplitude_deg, double min_duration_s, double max_duration_s,
                      int max_missing, double* state, double* table, int S, double* store, int* count, int* dropped, int* saccade_id,
                      float* saccade_ms, eve_stream_t stream);

/* Smooth pursuit, the third gaze class: among the frames that eve_gaze_events labels fixations, those in which the gaze turned
 * steadily and straight over a window of the chained samples before them are promoted to the pursuit class and cut into episodes with
 * amplitude, direction, mean and peak velocity, path length and, with a target, gain and position error, for B streams x T frames,
 * with the state carried in `state`, the tallies in `table` and the accepted episodes in `store` from one call to the next.  Float64,
 * every operation rounded on its own (no contraction), in the order written here; tests/pursuit_ref.py restates it in numpy.  One
 * wavefront per stream, passes of 64 frames, the windows' and the closings' atan2 across the lanes; the bits do not depend on that
 * structure.
 *   sample, sample_time, gaze_vector, point, event, velocity, fixation_id, lengths, reset: as for eve_gaze_saccades; target [B*T][2]
 *   float, may be NULL: the pursued object's screen position in the point's pixels, NaN where there is none (NULL: none anywhere),
 *   widened to double.
 *   state [B][320] double, table [B][16] double, store [B][S][20] double, count [B] and dropped [B] int: read and UPDATED IN PLACE.
 * The state row, an all-zero row being a fresh stream: 32 scalars -- 0 ring_n, 1 seen_saccade (a saccade frame since the last
 * restart), 2 t_saccade (the last one's time), 3 open, 4 the open episode's id, 5 next_id (the ids handed out so far), 6 t_onset,
 * 7-9 the onset's gaze vector, 10-11 its point, 12 its cum, 13 n (the episode's pursuit frames), 14 peak, 15 missing, 16 fixation_id,
 * 17 t_last, 18-20 the last sample's gaze vector, 21-22 its point, 23 its cum, 24 gain_sum, 25 gain_n, 26 err_sum, 27 has_end, 28
 * t_end (the last closed episode's end, while has_end), 29-31 reserved (0) -- then the ring: 32 entries of 9 doubles (t, v0, v1, v2,
 * cum, x, y, tx, ty), the first ring_n of them the run's last samples, oldest first, the others 0.  The RUN is the chained
 * fixation-labelled samples since the last break; cum is the path length along it in degrees.
 * A stream with reset[b] != 0 first aborts its open episode (table.aborted += 1, nothing stored) and zeroes its row except entry 5;
 * the table stays.  Then frames f = 0 .. lengths[b] - 1 are walked in order (the later ones: class 0, id -1, ms 0, the rest NaN).
 *   sample 0: where an episode is open, missing += 1.  Nothing else moves; class 0.
 *   sample 1 (or sample 2 with an event other than 1 and 2, which eve_gaze_events never writes): an open episode is aborted, the run
 *   is emptied, seen_saccade = has_end = 0, and the sample becomes the run's first entry with cum = 0.  Class 0.
 *   sample 2, event 2: an open episode CLOSES (below); the run is emptied, has_end = 0, seen_saccade = 1, t_saccade = t.  Class 2.
 *   sample 2, event 1: class 1 unless promoted.  With seen_saccade and t - t_saccade < settle_s the sample is not admitted to the run
 *   (the one-euro filter's creep after a landing stays out of the windows).  Else it is appended with cum = cum_last + (double)
 *   velocity * (t - t_last) (last: the run's entry before it; 0 for a first entry), and the ring keeps the last 32.  Its WINDOW
 *   starts at entry j, found by stepping back from this entry while the entry before is in the ring (this one included: at most 31
 *   steps) and t - t_that <= window_s.  With t - t_j < min_window_s there is no window: no promotion, the three window outputs NaN.
 *   Else A = atan2(sqrt((c0*c0 + c1*c1) + c2*c2), (p0*v0 + p1*v1) + p2*v2) * 57.29577951308232 with p entry j's vector, v this
 *   one's and c = p x v (eve_gaze_saccades' expression), w = A / (t - t_j), path = cum - cum_j, s = path > 0 ? A / path : 0, and the
 *   frame is a CANDIDATE iff w >= pursuit_deg_s && s >= min_straightness.  Where tx, ty, tx_j, ty_j are all finite: dt = (tx - tx_j,
 *   ty - ty_j), dg = (x - x_j, y - y_j), den = dtx*dtx + dty*dty, and where den > 0 the gain is defined: gain = (dgx*dtx + dgy*dty) /
 *   den, err = sqrt((x - tx)*(x - tx) + (y - ty)*(y - ty)).
 *   A candidate with no episode open opens one: id = next_id, next_id += 1 (accepted later or not); the onset is entry j -- with
 *   has_end, the first entry from j on whose t > t_end (this entry if none), so that episodes never overlap --: t_onset, the onset's
 *   vector, point and cum are that entry's; fixation_id is this frame's; n = peak = missing = gain_sum = gain_n = err_sum = 0.  Every
 *   candidate then: n += 1, peak = w where that is > peak, the episode's last sample (t_last, vector, point, cum) = this one, with a
 *   defined gain gain_sum += gain, err_sum += err, gain_n += 1; class 3, pursuit_id = id, pursuit_ms = 1000 * (t - t_onset).
 *   A run sample that is no candidate CLOSES an open episode at its last sample.
 *   Closing: has_end = 1, t_end = t_last, dur = t_last - t_onset, amplitude = the angle A between the onset's and the last vector,
 *   direction = atan2(y1 - y0, x1 - x0) * 57.29577951308232 (screen axes, y down), path = cum_last - cum_onset.  The first that holds
 *   decides: missing > max_missing: table.interrupted += 1; dur < min_duration_s: short; not (amplitude >= min_amplitude_deg): small;
 *   else it is accepted: mean = amplitude / dur, table.accepted += 1, sum_dur += dur, sum_amp += amplitude, sum_path += path,
 *   sum_mean_v += mean, max_peak takes a larger peak, sum_gain += gain_sum, gain_n += gain_n, and the row (id, t_onset, t_end, n, x0,
 *   y0, x1, y1, amplitude_deg, direction_deg, mean_deg_s, peak_deg_s, path_deg, fixation_id, missing, gain_n, mean_gain = gain_sum /
 *   gain_n, mean_error_px = err_sum / gain_n (both NaN with gain_n 0), 0, 0) goes to store[b][count[b]] and count[b] grows; with
 *   count[b] == S it is dropped and dropped[b] grows.
 * The table row: 0 accepted, 1 sum_dur, 2 sum_amp, 3 sum_path, 4 sum_mean_v, 5 max_peak, 6 sum_gain, 7 gain_n, 8 aborted, 9 small,
 * 10 short, 11 interrupted, 12-15 reserved (0).  An episode open at the end of the frames stays open across calls; there is no flush.
 * T = 0 is a call that only resets (the frame pointers may then be NULL).
 * Outputs per frame, written for every f < T: gaze_class [B*T] uint8 (0 none, 1 fixation, 2 saccade, 3 pursuit), pursuit_id [B*T]
 * int (-1 outside an episode), pursuit_ms [B*T] float (0 outside), gaze_velocity_windowed [B*T] float (w), gaze_straightness [B*T]
 * float (s; both NaN without a window), pursuit_gain [B*T] float (NaN without a defined gain); each rounded from double once.
 * Kernel name gaze_pursuits_kernel.  Refused without a launch: a null carried buffer, B < 1, T < 0, S < 1, with T > 0 a null frame
 * input (target excepted) or output, index ranges past 31 bits, a parameter that is not finite, window_s <= 0, min_window_s <= 0 or
 * > window_s, pursuit_deg_s <= 0, min_straightness outside (0, 1], settle_s < 0, min_duration_s < 0, min_amplitude_deg < 0,
 * max_missing < 0.  Not offered: hysteresis, or merging episodes across catch-up saccades (the rows carry what a host merge needs);
 * retroactive relabelling of the frames before a window fills; per-eye pursuit; vestibulo-ocular compensation; a gradient.  Pursuit
 * wants the filtered point: with velocity_from_raw, jitter lowers the straightness and fragments episodes at high frame rates.
 * (Additive: ABI v10.)                                                                                                              */
int eve_gaze_pursuits(long long B, int T, const uint8_t* sample, const double* sample_time, const double* gaze_vector, const float* point,
                      const uint8_t* event, const float* velocity, const int* fixation_id, const float* target /* may be NULL */,
                      const int* lengths /* may be NULL */, const int* reset /* may be NULL */, double window_s, double min_window_s,
                      double pursuit_deg_s, double min_straightness, double settle_s, double min_duration_s, double min_amplitude_deg,
                      int max_missing, double* state, double* table, int S, double* store, int* count, int* dropped, uint8_t* gaze_class,
                      int* pursuit_id, float* pursuit_ms, float* gaze_velocity_windowed, float* gaze_straightness, float* pursuit_gain,
                      eve_stream_t stream);

/* The eye gate: per frame and eye, is the eye usable?  One launch between the pose derivation and eve_stream_mask_plan turns the
 * results of the same step -- the pose flags, the solve's reprojection error and inlier count, the derived warps and head angles --
 * and the tracker's eyelid points into the mask the masked step consumes, and detects blinks with state carried in `state` from one
 * call to the next.  B streams x T frames.  Float64, every operation rounded on its own (no contraction), in the order written
 * here; tests/eye_gate_ref.py restates it in numpy.  One wavefront per stream, passes of 64 frames; the bits do not depend on that.
 *   pose_valid [B*T][2] uint8, reproj_rms [B*T] float, inliers [B*T] uint8, warp [2][B*T][9] float (inv(W), what the eye-warp kernels
 *   take), h [2][B*T][2] float (pitch, yaw of the head in each eye's normalised space, eve_eye_pose_normalize's convention),
 *   contours [B*T][2][6][C] float, C = 2 or 3: pixel (u, v[, w]) of the six eyelid points p1 .. p6 of the (left, right) eye in
 *   eye-aspect-ratio order -- p1, p4 the corners, p2, p3 on the upper lid, p6, p5 below them; lengths [B] int (clamped to 0 .. T),
 *   reset [B] int.  EACH MAY BE NULL, which turns its criterion off (all T frames, no reset).
 *   state [B][2][8] double, blinks [B][capacity][4] double, count [B] and dropped [B] int: read and UPDATED IN PLACE.
 * The state row of (stream, eye): 0 has_base, 1 base (the open eye's aspect ratio), 2 closed, 3 run (the closed frames so far),
 * 4 min_open, 5 start (the tick of the first closed frame), 6 hold (frames still withheld), 7 tick (the stream's delivered frames
 * since its last reset; both eyes' rows hold it).  A stream with reset[b] != 0 first zeroes both rows; an eye closed then stores
 * nothing.  Frames f >= lengths[b]: usable 0, reason 0, openness NaN, blink 0, and no state moves.  For the others, per eye e:
 *   reason bits (a NaN fails every comparison, towards unusable):
 *      1 pose         pose_valid[f][e] == 0
 *      2 reprojection not (rms <= max_reproj_px)
 *      4 inliers      not (inliers >= min_inliers)
 *      8 coverage     the 8 x 8 lattice of patch pixels ox_i = ((2i+1)*OW) >> 4, oy_j = ((2j+1)*OH) >> 4 goes through the eye's warp
 *                     as in eve_eye_warp_u8_to_nchw: X = (m00*ox + m01*oy) + m02, Y, Wd alike, u = X/Wd, v = Y/Wd; a point is inside
 *                     iff Wd > 0 && u > -1 && u < IW && v > -1 && v < IH; the bit is set iff fewer than min_inside points are.  (With
 *                     camera_lens upstream the test is made in the undistorted coordinates inv(W) refers to.)
 *     16 head angle   not (pitch_lo <= h[e][f][0] <= pitch_hi && yaw_lo[e] <= h[e][f][1] <= yaw_hi[e]); an open side is +-infinity
 *     32 closed, 64 hold-off: the blink machine below (contours != NULL), one walk per eye over the delivered frames in order, with
 *        tick = state tick + f:
 *      d(a, b) = sqrt(dx*dx + dy*dy) of the widened pixels; ear = (d(p2,p6) + d(p3,p5)) / (2*d(p1,p4)); KNOWN iff all twelve
 *      coordinates are finite, every w > 0 (C = 3) and d(p1,p4) != 0.
 *      known and has_base == 0: base = ear, has_base = 1.  open = ear / base where known, NaN else.
 *      closed != 0: run += 1; known and open < min_open: min_open = open; then
 *         known and open > open_ratio: the blink ends -- the row (e, start, tick - 1, min_open) goes to blinks[b][count[b]] and
 *            count[b] grows, or with count[b] == capacity dropped[b] grows; closed = 0, run = 0, hold = hold_frames;
 *         else run > max_closed_frames (a wrong baseline): has_base = known, base = ear where known (0 else), closed = 0, run = 0,
 *            open = ear / base again where known; no row, no hold-off.
 *      closed == 0: known and open < close_ratio: closed = 1, run = 1, min_open = open, start = tick;
 *         else known and open >= open_ratio: base = base + r*(ear - base), r = baseline_rise if ear > base else baseline_rate (a peak
 *            follower: a first frame taken in the middle of a blink does not keep the baseline down).
 *      Then: closed != 0 sets bit 32 and blink = 1; else hold > 0 sets bit 64 and hold -= 1 (so hold_frames frames from the reopening
 *      one on are withheld).  Rows of one frame are stored left eye first.  After the frames tick += lengths[b].
 * Outputs [B*T][2]: usable uint8 (1 iff reason == 0), reason uint8, openness float (open rounded once; NaN where unknown or contours is
 * NULL), blink uint8.  Kernel name eye_gate_kernel.  Refused without a launch: a null params, state, store, counter or output; B, T or
 * capacity < 1; contours with C other than 2 or 3; warp without sizes in 1 .. 16384; B*T*36 or B*capacity*4 past 31 bits; a NaN among
 * the floating-point parameters; with warp, min_inside outside 1 .. 64; with contours, open_ratio <= close_ratio, hold_frames < 0 or
 * max_closed_frames < 1.  Not offered: thresholds learnt per person, a closure announced before its first closed frame, blink times in
 * seconds, coverage through the lens model, a gradient.  (Additive: ABI v10.)                                                      */
typedef struct eve_eye_gate_params {
    double max_reproj_px;                       /* read where reproj_rms != NULL */
    double pitch_lo, pitch_hi, yaw_lo[2], yaw_hi[2];   /* read where h != NULL; yaw per eye (left, right) */
    double close_ratio, open_ratio, baseline_rate, baseline_rise;   /* read where contours != NULL */
    int min_inliers;                            /* read where inliers != NULL */
    int min_inside;                             /* read where warp != NULL: ceil(min_coverage * 64) */
    int hold_frames, max_closed_frames;         /* read where contours != NULL */
} eve_eye_gate_params;
int eve_eye_gate(long long B, int T, const uint8_t* pose_valid /* may be NULL */, const float* reproj_rms /* may be NULL */,
                 const uint8_t* inliers /* may be NULL */, const float* warp /* may be NULL */, const float* h /* may be NULL */,
                 const float* contours /* may be NULL */, int C, const int* lengths /* may be NULL */, const int* reset /* may be NULL */,
                 int IW, int IH, int OW, int OH, const eve_eye_gate_params* params, double* state, int capacity, double* blinks, int* count,
                 int* dropped, uint8_t* usable, uint8_t* reason, float* openness, uint8_t* blink, eve_stream_t stream);

/* The time-decayed gaze history: per stream a float32 map m [MH][MW] that follows M_t = decay^(dt_ms) * M_{t-1} + w_t * G_t, G_t the
 * Gaussian around the frame's point of gaze or a heat map handed in, for B streams x T frames, with the time chain carried in `state`
 * and the map in `map` from one call to the next.  Two launches: the plan walks the time chain and writes one coefficient row per
 * frame, the update applies the rows to the map (no workgroup of the map launch reads and writes the state row).  Float64, every
 * operation rounded on its own (no contraction), in the order written here; tests/gaze_history_ref.py restates it in numpy, and the
 * device equals it bit for bit because the contract owns its exp:
 *   gh_exp(x), x <= 0: xc = x < -104 ? -104 : x; k = rint(xc * 1.4426950408889634); r = (xc - k * 6.93147180369123816490e-01) -
 *   k * 1.90821492927058770002e-10; p = Horner of sum_{j = 0..13} r^j / j! from 1/13! downwards (p = p*r + c_j, the c_j the correctly
 *   rounded doubles 1/j!); the result is ldexp(p, (int)k), and exactly 0 where x < -104.
 * eve_gaze_history_plan: pog [B*T][2] float (screen pixels; NULL for the heat source), frame_time [B*T] double seconds or NULL (then
 *   t = ticks / fps), valid and valid_key [B*T] uint8, lengths [B] int (clamped to 0 .. T), reset [B] int: each may be NULL.  state
 *   [B][8] double: 0 has_prev, 1 t_prev, 2 ticks (the delivered frames since the last reset), 3-7 reserved (0); UPDATED IN PLACE.
 *   coef [B*T][4] double and clear [B] int are written.  A stream with reset[b] != 0 zeroes its row and gets clear[b] = 1 (else 0),
 *   also with no frame.  For f < lengths[b] in order: tt = frame_time[b][f], or ticks / fps; ticks += 1 either way.  tt not finite, or
 *   has_prev and tt < t_prev: the frame is IGNORED, coef row (-1, 0, ., .) -- so are the frames from lengths[b] on.  Otherwise delta =
 *   has_prev ? tt - t_prev : 0, d = gh_exp((delta * 1000.0) * ln_decay); usable = valid && valid_key && (pog == NULL or both
 *   coordinates finite); w = gain * (weight_seconds == 0 ? 1 : has_prev ? min(delta, max_gap_s) : (fps > 0 ? 1 / fps : 0)); then
 *   has_prev = 1, t_prev = tt.  The row is (d, usable ? w : -1, cx, cy), cx = ((double)MW / screen_w) * (double)pog_x, cy likewise.
 *   fps = 0 means "not given".  Kernel name gaze_history_plan_kernel, one wavefront per stream.
 * eve_gaze_history_update: coef and clear as the plan wrote them; heat NULL or [B*T][MH][MW] float; map [B][MH][MW] float UPDATED IN
 *   PLACE; frames NULL or [B*T][MH][MW] float, the map after every frame.  A stream with clear[b] != 0 starts from a zero map.  Per
 *   frame in order and per pixel (x, y), pixel centres at integer coordinates: d < 0 leaves the map as it stands; else with ex =
 *   gh_exp(alpha * ((x - cx) * (x - cx))) and ey likewise, v = (double)m * d + w * (ex * ey + floor), or with heat v = (double)m * d +
 *   w * (double)heat[b][f][y][x], or with w < 0 v = (double)m * d alone (no multiplication by a zero weight: a NaN point never
 *   reaches the map); m = fabs(v) < 2^-100 ? 0 : (float)v -- rounded to float after EVERY frame, so the bits do not depend on how a clip
 *   is cut into chunks, and no float denormal is produced.  T = 0 is legal: a set clear flag zeroes the map, nothing else is written.
 *   Kernel name gaze_history_update_kernel, grid (tiles of 64 x 32, B), 16-byte loads and stores where MW % 4 == 0 and the buffers
 *   are 16-byte aligned.
 * Refused without a launch: a null state, clear or map, with T > 0 a null coef, B < 1 (update: B > 65535), T < 0, a map axis outside
 * 1 .. 2048, B*T*4 past 31 bits, a screen size, max_gap_s or gain that is not a finite number > 0, fps not a finite number > 0 where
 * frame_time is NULL and T > 0, ln_decay not a finite number <= 0, alpha not a finite number < 0, floor not a finite number >= 0.
 * Not offered: per-eye maps, a windowed history, anisotropic sigmas, a gradient.  (Additive: ABI v10.)                            */
int eve_gaze_history_plan(long long B, int T, const float* pog /* may be NULL */, const double* frame_time /* may be NULL */,
                          const uint8_t* valid /* may be NULL */, const uint8_t* valid_key /* may be NULL */,
                          const int* lengths /* may be NULL */, const int* reset /* may be NULL */, double fps, double ln_decay,
                          int weight_seconds, double max_gap_s, double gain, int MW, int MH, double screen_w, double screen_h, double* state,
                          double* coef, int* clear, eve_stream_t stream);
int eve_gaze_history_update(long long B, int T, int MH, int MW, const double* coef, const int* clear, const float* heat /* may be NULL */,
                            double alpha, double floor, float* map, float* frames /* may be NULL */, eve_stream_t stream);

/* Areas of interest: which region of the screen the point of gaze is in, for how long, how often and in which order -- per frame a
 * hit test against up to 64 shapes, and per stream a state machine that turns the sequence of hits into visits, a dwell table and a
 * transition matrix -- for B streams x T frames, with the state carried in `state` and the tallies in `table`, `trans` and `visits`
 * from one call to the next.  Float64, + - * / and comparisons only, every operation rounded on its own (no contraction), in the
 * order written here; tests/aoi_ref.py restates it in numpy, and the device equals it bit for bit.  One wavefront per stream, passes
 * of 64 frames, (frame, AOI) pairs tiled over the lanes for the hit tests; the bits do not depend on that structure.
 *   pog [B*T][2] float (screen pixels); shapes [B][A][36] float, or with shapes_per_frame != 0 [B*T][A][36] (one table per frame:
 *   moving regions); frame_time [B*T] double seconds or NULL (then t = ticks / fps); valid and valid_key [B*T] uint8, fixation_id
 *   [B*T] int with fixating [B*T] uint8 (both or neither), lengths [B] int (clamped to 0 .. T), reset [B] int, flush [B] int: each may
 *   be NULL (all frames, no fixation tallies, T frames, no reset, no flush).
 *   state [B][16] double, table [B][A+1][8] double, trans [B][A+1][A] int, visits [B][visit_capacity][8] double, count [B] and
 *   dropped [B] int: read and UPDATED IN PLACE.
 * An AOI row: 0 kind (0 disabled, 1 rectangle, 2 ellipse, 3 polygon), 1 the polygon's vertex count n, 2-3 reserved (0), 4 .. the
 * coordinates.  The point (x, y) and the coordinates are widened to double.  Rectangle (x0, y0, x1, y1): x0 <= x && x < x1 && y0 <= y &&
 * y < y1.  Ellipse (cx, cy, rx, ry), rx > 0 && ry > 0: u = (x - cx) / rx, v = (y - cy) / ry, u*u + v*v <= 1.  Polygon (x_i, y_i), i < n, n
 * an integer in 3 .. 16, even-odd: for i = 0 .. n - 1 and j = i == 0 ? n - 1 : i - 1, toggle iff ((y_i > y) != (y_j > y)) && x < (x_j -
 * x_i) * (y - y_i) / (y_j - y_i) + x_i.  A row contains nothing where a coordinate it uses is not finite, for any other kind or n, and
 * for an ellipse without rx > 0 && ry > 0.  mask has bit a set iff row a contains the point; the frame's AOI is the lowest set bit
 * (the order of the rows is the z-order), or -1.
 * The state row, an all-zero row being a fresh stream (AOI indices and fixation ids are held as value + 1, 0 = none): 0 ticks (the
 * delivered frames since the last reset), 1 has_prev, 2 t_prev (the last sample's time), 3 the last sample's AOI + 1 (0: outside),
 * 4 visit_open, 5 the open visit's AOI + 1, 6 its t_enter, 7 its t_last, 8 its samples, 9 its fixations, 10 its visit_index, 11
 * next_visit_index (the visits opened so far), 12 last_aoi + 1 (the AOI of the visit closed last; 0: none since the reset), 13-14 the
 * (fixation_id + 1, AOI + 1) pair counted last, 15 reserved (0).
 * A table row: (dwell_s, samples, visits, t_first_entry, t_last, fixations, t_first_fixation, 0); row A is "no AOI".  trans[from][to]
 * counts visits opened; row A is "first visit since reset", trans[a][a] a revisit.  A visit row: (aoi, t_enter, t_last, samples,
 * fixations, visit_index, 0, 0).
 * A stream with reset[b] != 0 first closes its open visit (below) and zeroes its row except entry 11; the tallies stay.  Then frames
 * f = 0 .. lengths[b] - 1 are walked in order.  tt = frame_time[b][f], or (ticks + f) / fps.  The frame is a SAMPLE iff valid[b][f] and
 * valid_key[b][f], x, y and tt are finite, and (has_prev == 0 or tt > t_prev).  Any other frame changes nothing: id -2, mask 0,
 * visit_ms 0 (so do the frames from lengths[b] on).  For a sample: dt = tt - t_prev; restart = has_prev == 0 || dt > max_gap_s; a = the
 * frame's AOI.  On restart the open visit is closed; otherwise, where one is open and a is not its AOI, it is closed.  a >= 0 and no
 * visit open: one opens -- t_enter = tt, samples = fixations = 0, visit_index = next_visit_index++, table[a].visits += 1 (at the first,
 * t_first_entry = tt), trans[last_aoi, or A][a] += 1; a >= 0 and the visit continues: table[a].dwell_s += dt.  Either way for a >= 0
 * the visit's samples += 1 and t_last = tt, table[a].samples += 1, table[a].t_last = tt, visit_ms = 1000 * (tt - t_enter).  a == -1:
 * table[A].samples += 1, and where !restart and the last sample was outside too, table[A].dwell_s += dt.  With fixation_id: where a >=
 * 0, fixating != 0, fixation_id >= 0 and (fixation_id, a) is not the pair counted last, table[a].fixations += 1 (at the first,
 * t_first_fixation = tt), the visit's fixations += 1 and the pair is remembered.  Finally t_prev = tt, has_prev = 1, entry 3 = a + 1.
 * Closing: visit_open = 0, last_aoi = the visit's AOI, and its row goes to visits[b][count[b]] and count[b] grows; with count[b] ==
 * visit_capacity it is dropped and dropped[b] grows.  After the frames ticks += lengths[b], and a stream with flush[b] != 0 closes its
 * open visit.  T = 0 is a call that only resets and flushes (the frame pointers may then be NULL).
 * Outputs per frame: id [B*T] int, mask [B*T] int64, visit_ms [B*T] float (rounded from double once).  Kernel name gaze_aoi_kernel.
 * Refused without a launch: a null carried buffer, B < 1, T < 0, A outside 1 .. 64, visit_capacity < 1, with T > 0 a null frame input or
 * output, fixation_id without fixating or the reverse, index products past 31 bits, max_gap_s not a finite number > 0, fps not a
 * finite number > 0 where frame_time is NULL and T > 0.  Not offered: label-map AOIs, minimum visit durations or border hysteresis,
 * per-eye AOIs, polygon margins, a gradient.  (Additive: ABI v10.)                                                                  */
int eve_gaze_aoi(long long B, int T, int A, const float* pog, const float* shapes, int shapes_per_frame,
                 const double* frame_time /* may be NULL */, const uint8_t* valid /* may be NULL */, const uint8_t* valid_key /* may be NULL */,
                 const int* fixation_id /* may be NULL */, const uint8_t* fixating /* may be NULL */, const int* lengths /* may be NULL */,
                 const int* reset /* may be NULL */, const int* flush /* may be NULL */, double fps, double max_gap_s, double* state,
                 double* table, int* trans, int visit_capacity, double* visits, int* count, int* dropped, int* id, long long* mask,
                 float* visit_ms, eve_stream_t stream);

/* Pupillometry: EyeNet's two pupil sizes per frame become one validated, binocularly fused, low-passed, light- and baseline-corrected
 * trace per stream, with a table of tallies and a store of dilation / constriction episodes -- for B streams x T frames, with the
 * state carried in `state`, the tallies in `table`, the light response in `light` and the episodes in `store` from one call to the
 * next.  Float64, + - * /, fabs and comparisons only, every operation rounded on its own (no contraction), in the order written
 * here; tests/pupil_ref.py restates it in numpy, and the device equals it bit for bit.  One wavefront per stream, passes of 64
 * frames loaded across the lanes, the walk in one lane; the bits do not depend on that structure.
 *   size [2][B*T] float (left, right; mm as EyeNet gives them), widened to double; eye_valid [B*T][2] uint8 or NULL (every eye
 *   delivered); frame_time [B*T] double seconds or NULL (then t = (ticks + f) / fps); lengths [B] int (clamped to 0 .. T), reset [B]
 *   int, flush [B] int, luminance [B*T] float, baseline_mark [B*T] uint8: each may be NULL (T frames, no reset, no flush, no light
 *   covariate, no marks).
 *   state [B][32] double, table [B][24] double, light [B][4] double, store [B][capacity][8] double, count [B] and dropped [B] int:
 *   read and UPDATED IN PLACE (light is only read).
 * The state row, an all-zero row being a fresh stream: 0 ticks (the delivered frames since the last reset), 1 has_prev, 2 t_prev (the
 * last sample's time), 3 df_prev (its filtered size), 4 idx_prev (its frame index ticks + f), 5-7 left (has, t, size) and 8-10 right
 * (has, t, size): each eye's last accepted size, 11 has_off, 12 off, 13 has_lum, 14 t_lum, 15 Lf (the low-passed luminance), 16
 * has_base, 17 base, 18 the marked samples of the current run, 19 the run's first dc, 20 its sum(dc - first), 21 prev_mark (the mark
 * of the last timed frame), 22 episode_open, 23 its phase, 24 t_start, 25 t_end, 26 d_start, 27 d_end, 28 peak |velocity|, 29 samples,
 * 30 Lf at its start or 0, 31 episodes (those closed with enough amplitude since the stream began: stored or dropped).
 * The table row: 0 covered_s, 1 lost_s, 2 binocular, 3 left-only and 4 right-only samples (the samples are their sum), 5-7 the left
 * eye's rejects for not finite / range / speed, 8-10 the right eye's, 11 d0 (the first sample's dc), 12 sum(dc - d0), 13 sum((dc -
 * d0)^2), 14 min dc, 15 max dc, 16 n, 17 x0, 18 y0, 19 sum(x - x0), 20 sum(y - y0), 21 sum((x - x0)^2), 22 sum((x - x0)(y - y0)), 23
 * sum((y - y0)^2) of the pairs x = Lf, y = df.  (A withheld eye is the withholding stage's tally, not counted here.)  light:
 * (has_gain, gain, ref, 0).  An episode row: (phase +1 dilation / -1 constriction, t_start, t_end, d_start, d_end, peak |velocity|,
 * samples, Lf at the start or 0).
 * A stream with reset[b] != 0 first closes its open episode (below) and zeroes its row except entry 31; table and light stay.  Then
 * frames f = 0 .. lengths[b] - 1 are walked in order.
 * 1 Time.  t = frame_time[b][f], or (ticks + f) / fps.  The frame is TIMED iff t is finite and (has_prev == 0 or t > t_prev); any
 *   other frame, and the frames from lengths[b] on, change nothing and give the outputs of "no sample" with eye_reason 0.
 * 2 Luminance (luminance != NULL, the value finite, and has_lum == 0 or t > t_lum): dtl = t - t_lum; has_lum == 0 or dtl > max_gap_s:
 *   Lf = lum; else al = 1 / (1 + light_tau_s / dtl), Lf = al * lum + (1 - al) * Lf.  Then has_lum = 1, t_lum = t.
 * 3 Acceptance, per eye e, the first test that fails gives the reason: eye_valid[f][e] == 0: 1 (withheld; its size is not read into
 *   any arithmetic); size not finite: 2; !(min_mm <= size && size <= max_mm): 4; where has_e and t - t_e <= max_gap_s:
 *   !(fabs(size - size_e) / (t - t_e) <= max_speed_mm_s): 8 (the dilation-speed criterion of Kret & Sjak-Shie 2019 with a fixed
 *   bound; an eye rejected for longer than max_gap_s is re-admitted untested).  Reasons 2, 4 and 8 count in the table.
 * 4 Fusion.  Both accepted: off = has_off ? off + offset_rate * ((l - r) - off) : l - r, has_off = 1, d = 0.5 * (l + r).  Left only: d
 *   = has_off ? l - 0.5 * off : l.  Right only: d = has_off ? r + 0.5 * off : r.  Neither: no SAMPLE -- mm, raw_mm, velocity and both
 *   changes NaN, valid, eye_used and event 0 -- and nothing moves but what 2, 3 and prev_mark (7) moved.
 * 5 Filter.  dt = t - t_prev; restart = has_prev == 0 || dt > max_gap_s.  Restart: df = d, velocity = NaN, the open episode closes.
 *   Else a = 1 / (1 + (1 / (6.283185307179586 * cutoff_hz)) / dt), df = a * d + (1 - a) * df_prev, velocity = (df - df_prev) / dt
 *   (mm/s), covered_s += dt, and where (ticks + f) - idx_prev != 1 (frames that were no samples lie between) also lost_s += dt.
 * 6 Light (luminance != NULL and has_lum): at n == 0, x0 = Lf and y0 = df; dx = Lf - x0, dy = df - y0; n += 1 and the five sums grow
 *   by dx, dy, dx * dx, dx * dy, dy * dy; where has_gain != 0, dc = df - gain * (Lf - ref).  Otherwise dc = df, its bits untouched.
 * 7 Baseline.  With baseline_mark: a marked sample with prev_mark == 0 starts a run (first = dc, count = sum = 0); every marked sample:
 *   count += 1, sum += dc - first, base = first + sum / count, has_base = 1.  Without marks and with baseline_tau_s > 0: has_base == 0
 *   or has_prev == 0: base = dc; else base = base + (1 / (1 + baseline_tau_s / dt)) * (dc - base); has_base = 1.  With either and
 *   has_base: change_mm = dc - base, change_pct = 100 * (dc - base) / base; else both NaN.  Every TIMED frame, sample or not, ends
 *   with prev_mark = its mark (only with baseline_mark != NULL).
 * 8 Episodes.  phase = velocity > dilate_mm_s ? +1 : velocity < -constrict_mm_s ? -1 : 0.  An open episode of another phase closes.
 *   phase != 0 and none open: one opens at the PREVIOUS sample -- t_start = t_prev, d_start = df_prev, peak = samples = 0, Lf as in
 *   6 or 0.  Then t_end = t, d_end = df, peak = max(peak, fabs(velocity)), samples += 1.  Closing: episode_open = 0, and where
 *   fabs(d_end - d_start) >= min_amplitude_mm, entry 31 += 1 and the row goes to store[b][count[b]] and count[b] grows; with count[b]
 *   == capacity it is dropped and dropped[b] grows.
 * 9 Table and hand-over.  The sample's count (binocular / left / right) += 1; at the table's first sample d0 = min = max = dc; sum
 *   += dc - d0, sum2 += (dc - d0)^2, min and max follow.  Each accepted eye's (has, t, size) = (1, t, its size); has_prev = 1, t_prev =
 *   t, df_prev = df, idx_prev = ticks + f.
 * After the frames ticks += lengths[b], and a stream with flush[b] != 0 closes its open episode.  T = 0 is a call that only resets
 * and flushes (the frame pointers may then be NULL).
 * Outputs per frame, each float rounded from double once: mm (= dc), raw_mm (= d), velocity, change_mm, change_pct float [B*T]; valid
 * uint8 [B*T]; eye_used and eye_reason uint8 [B*T][2]; event uint8 [B*T] (0 none, 1 dilating, 2 constricting).  Kernel name
 * pupil_track_kernel.
 * Refused without a launch: a null carried buffer, B < 1, T < 0, capacity < 1, with T > 0 a null size or output, index products past
 * 31 bits, min_mm or max_mm not a finite number > 0 or min_mm >= max_mm, offset_rate outside (0, 1], max_speed_mm_s, max_gap_s,
 * cutoff_hz, light_tau_s, dilate_mm_s or constrict_mm_s not a finite number > 0, baseline_tau_s or min_amplitude_mm not a finite
 * number >= 0, fps not a finite number > 0 where frame_time is NULL and T > 0.  The covariate comes from the caller; eve_screen_luminance
 * below computes one from the screen capture.  Not offered: non-causal blink padding and interpolation across gaps, foreshortening
 * correction, per-eye filtered traces, wavelet indices (IPA / LHIPA), per-fixation or per-AOI pupil means, a gradient.
 * (Additive: ABI v10.)                                                                                                            */
int eve_pupil_track(long long B, int T, const float* size, const uint8_t* eye_valid /* may be NULL */,
                    const double* frame_time /* may be NULL */, const int* lengths /* may be NULL */, const int* reset /* may be NULL */,
                    const int* flush /* may be NULL */, const float* luminance /* may be NULL */,
                    const uint8_t* baseline_mark /* may be NULL */, double fps, double min_mm, double max_mm, double max_speed_mm_s,
                    double max_gap_s, double offset_rate, double cutoff_hz, double light_tau_s, double baseline_tau_s, double dilate_mm_s,
                    double constrict_mm_s, double min_amplitude_mm, double* state, double* table, double* light, int capacity, double* store,
                    int* count, int* dropped, float* mm, float* raw_mm, float* velocity, float* change_mm, float* change_pct, uint8_t* valid,
                    uint8_t* eye_used, uint8_t* eye_reason, uint8_t* event, eve_stream_t stream);

/* Screen luminance: the mean relative luminance of every delivered screen capture, over the whole visible region and over up to
 * four concentric discs around a per-frame centre (the point of gaze) -- the light covariate of the pupil trace, computed per
 * pixel at capture resolution from the surface where it lies, for B streams x T frames, frame n = b * T + f.  Everything is integer
 * arithmetic up to one float64 division, so the device equals numpy bit for bit (tests/screen_luminance_ref.py) and the grid, the
 * order of the sums and any split into bands do not change the result.
 *   Per visible pixel the three 8-bit values (R, G, B) are read through the surface's address rule (eve_surface above) and, for
 *   EVE_SURF_YUV, converted exactly as eve_screen_area_surface_to_nchw converts a pixel (the integer matrix, nearest chroma sample,
 *   clamps).  Then y = (kr * response[0][R] + kg * response[1][G] + kb * response[2][B] + 32768) >> 16 in 32 unsigned bits, 0 .. 65535:
 *   response [3][256] uint16 on the device is the display's linearisation (sRGB's EOTF scaled to 65535, a power law or a measured
 *   curve), and kr, kg, kb >= 0 with kr + kg + kb == 65536 weigh the channels -- Rec.709: (13933, 46871, 4732) -- so the sum fits.
 *   Frame n is DELIVERED iff lengths == NULL or f < clamp(lengths[b], 0, T).  An undelivered frame has every column 0 (mean NaN), and
 *   its bytes are not read.
 *   Column 0 is every visible pixel: sums[n][0] = sum of y, counts[n][0] = width * height.  Columns 1 .. R are the discs of radius
 *   radii[k] capture pixels (a HOST array [R] read during the call; 1 .. 16384, strictly increasing) around the frame's centre,
 *   quantised the overlay's way, in half pixels: qx = rint((centres[n][0] * sx) * 2) in float32, each product rounded, ties to even,
 *   qy likewise with sy.  Pixel (X, Y) lies in disc k iff (2X + 1 - qx)^2 + (2Y + 1 - qy)^2 <= 4 r_k^2 in 64-bit integers; counts is
 *   the number of VISIBLE pixels in the disc, so a disc that hangs off the edge counts what is on screen.  A frame's disc columns are
 *   0 where centre_valid[n] == 0 (uint8 [B*T], NULL: every centre valid), a coordinate is not finite, or |qx| or |qy| > 2^20.  No
 *   address is ever computed from a centre.
 *   mean[n][k] = (float)((double)sums / ((double)counts * 65535.0)): a zero count gives NaN.
 * The call zeroes sums and counts on the stream (capturable), then one workgroup per (frame, band of 32 rows) adds its 1 + R pairs
 * with integer atomics -- 8-bit 4:2:0 keeps eve_screen_area_surface_to_nchw's wide loads under the same conditions, or its byte
 * form; every other descriptor three byte loads per pixel -- and a second small kernel writes mean.  Kernel names (eve_last_kernel
 * names the form that read the frames): screen_luminance_kernel<yuv420,true | false> and screen_luminance_kernel<generic,false>; the
 * second kernel is screen_luminance_finish_kernel.  Refused without a launch, the message beginning "screen_luminance:": B < 1 or
 * T < 1, R outside 0 .. 4, B * T * (1 + R) >= 2^31, what eve_eye_warp_surface_to_nchw refuses of the descriptor, width or height >
 * 16384, a null src, response or output, weights that are negative or do not sum to 65536, radii outside 1 .. 16384 or not strictly
 * increasing, radii or centres without R > 0 or R > 0 without them, sx or sy not a finite number > 0.  Not offered: continuous
 * (eccentricity-weighted) kernels beyond concentric discs, per-AOI luminance, 10-bit arithmetic (P010 is read as its high byte),
 * ambient light, the camera image's luminance, a gradient.  (Additive: ABI v10.)                                                 */
int eve_screen_luminance(const eve_surface* surface, int matrix, long long B, int T, const uint8_t* src,
                         const uint16_t* response /* device, [3][256] */, int kr, int kg, int kb,
                         const int* lengths /* device [B], may be NULL */,
                         int R, const int* radii /* HOST array [R], read during the call; NULL iff R == 0 */,
                         const float* centres /* device [B*T][2], NULL iff R == 0 */, float sx, float sy,
                         const uint8_t* centre_valid /* device [B*T], may be NULL */,
                         unsigned long long* sums /* [B*T][1+R] */, int* counts /* [B*T][1+R] */, float* mean /* [B*T][1+R] */,
                         eve_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EVE_HIP_H_ */
