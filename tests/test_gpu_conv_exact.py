"""GPU: every convolution kernel, bit for bit, on integer-valued operands (tests/exact_conv.py has the argument and the helpers).

One table row per kernel instantiation: the shape and the eve_dispatch_config fields that reach it (derived from launch_halo,
launch_igemm_dma, launch_wgrad, launch_wgrad_halo and the rungs of csrc/conv_igemm.hip), and for every entry point the row runs the
name eve_last_kernel() must report -- coverage is by construction.  Every row runs in both operand regimes; every output has a guard
plane of 64 rows behind it, is produced twice (torch.equal) and is compared with `==` against the CPU reference rounded once.

Kernels launched without a name (bias_grad_kernel, wgrad_slab_reduce_kernel, s2_dgrad_pack_kernel) are reached through the entry
points that need them; conv3x3_wg8_kernel<.., s2dgrad2> runs in the same call as <.., s2dgrad4>, which is the name that call leaves.
"""
import pytest
import torch

import exact_conv as ec

pytestmark = pytest.mark.gpu

BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
REGIMES = pytest.mark.parametrize('regime', ['exact', 'rounding'])


@pytest.fixture(scope='module')
def calls():
    from eve_amd.kernels import HipKernels
    assert torch.cuda.is_available(), 'GPU suite needs a GPU'
    return ec.HipCalls(HipKernels())


def row(id, shape, ops, override=None, dtypes=ec.HALVES):
    return {'id': id, 'shape': shape, 'ops': ops, 'override': override or {}, 'dtypes': dtypes}


def stream1(ci, co):
    return {'fwd': 'conv1x1_stream_kernel<{T}, %d, %d, false>' % (ci, co), 'fwd_relu': 'conv1x1_stream_kernel<{T}, %d, %d, false>' % (ci, co),
            'fwd_acc': 'conv1x1_stream_kernel<{T}, %d, %d, true>' % (ci, co), 'dgrad': 'conv1x1_stream_kernel<{T}, %d, %d, false>' % (co, ci),
            'dgrad_acc': 'conv1x1_stream_kernel<{T}, %d, %d, true>' % (co, ci)}


def stream3(ci, co, dgrad=True):
    ops = {'fwd': 'conv3x3_stream_kernel<{T}, %d, %d, false>' % (ci, co), 'fwd_relu': 'conv3x3_stream_kernel<{T}, %d, %d, false>' % (ci, co),
           'fwd_acc': 'conv3x3_stream_kernel<{T}, %d, %d, true>' % (ci, co)}
    if dgrad:
        ops.update({'dgrad': 'conv3x3_stream_kernel<{T}, %d, %d, false>' % (co, ci), 'dgrad_acc': 'conv3x3_stream_kernel<{T}, %d, %d, true>' % (co, ci)})
    return ops


def same(name, *ops):
    return {op: name for op in ops}


NO_WG8_FLOOR = {'conv_wg8_min_tiles': 0, 'conv_wg8_s2_min_tiles': 0}

# shape = (N, H, W, Cin, Cout, ks, stride, pad)
CONV_ROWS = [
    # ---- streaming 1x1 (M = 3 x 77 x 71 = 16 401 pixels: ragged against the 16-pixel tile and the 32 / 64-pixel batch)
    row('1x1_stream_narrow', (3, 77, 71, 16, 32, 1, 1, 0), stream1(16, 32)),
    row('1x1_stream_wide', (3, 77, 71, 64, 128, 1, 1, 0), stream1(64, 128)),
    # ---- streaming 1x1 / stride 2 (no bias; the data gradient exists only as the accumulating one): 105 output pixels, odd height
    row('1x1_s2_stream_64_128', (3, 9, 14, 64, 128, 1, 2, 0),
        {'fwd_nobias': 'conv1x1_s2_stream_kernel<{T}, 64, 128, false>', 'dgrad_acc': 'conv1x1_s2_stream_kernel<{T}, 128, 64, true>'}),
    row('1x1_s2_stream_128_256', (3, 9, 14, 128, 256, 1, 2, 0),
        {'fwd_nobias': 'conv1x1_s2_stream_kernel<{T}, 128, 256, false>', 'dgrad_acc': 'conv1x1_s2_stream_kernel<{T}, 256, 128, true>'}),
    # ---- row-streaming 3x3, every channel pair it is built for; 64- and 128-wide rows, odd heights (the kernel takes >= 65 536 pixels)
    row('3x3_stream_16_16', (8, 65, 128, 16, 16, 3, 1, 1), stream3(16, 16)),
    row('3x3_stream_16_32', (28, 37, 64, 16, 32, 3, 1, 1), stream3(16, 32)),
    row('3x3_stream_32_16', (8, 65, 128, 32, 16, 3, 1, 1), stream3(32, 16)),
    row('3x3_stream_32_32', (28, 37, 64, 32, 32, 3, 1, 1), stream3(32, 32)),
    row('3x3_stream_16_64', (8, 65, 128, 16, 64, 3, 1, 1), stream3(16, 64)),
    row('3x3_stream_64_16', (28, 37, 64, 64, 16, 3, 1, 1), stream3(64, 16)),
    row('3x3_stream_32_64', (28, 37, 64, 32, 64, 3, 1, 1), stream3(32, 64, dgrad=False)),      # (64 -> 32 is not on this kernel)
    row('3x3_stream_32_128', (28, 37, 64, 32, 128, 3, 1, 1), stream3(32, 128, dgrad=False)),
    # ---- filter-resident 64 -> 64: 2 tiles per 32 x 32 image, 8 per 64 x 64 image; 262 / 296 tiles on 256 workgroups
    row('ws64_32', (131, 32, 32, 64, 64, 3, 1, 1), same('conv3x3_ws64_kernel<{T}, 32>', 'fwd', 'fwd_relu', 'dgrad')),
    row('ws64_64', (37, 64, 64, 64, 64, 3, 1, 1), same('conv3x3_ws64_kernel<{T}, 64>', 'fwd', 'fwd_relu', 'dgrad')),
    # ---- eight-wave 3x3 / stride 1, tile floor lowered; image counts that leave the last tile partly empty
    row('wg8_4_2_16', (5, 16, 16, 128, 128, 3, 1, 1), same('conv3x3_wg8_kernel<{T}, 4, 2, 16>', 'fwd', 'fwd_relu', 'dgrad'), NO_WG8_FLOOR),
    row('wg8_2_4_16', (3, 16, 16, 256, 256, 3, 1, 1), same('conv3x3_wg8_kernel<{T}, 2, 4, 16>', 'fwd', 'fwd_relu', 'dgrad'), NO_WG8_FLOOR),
    row('wg8_2_4_8', (5, 8, 8, 256, 256, 3, 1, 1), same('conv3x3_wg8_kernel<{T}, 2, 4, 8>', 'fwd', 'fwd_relu', 'dgrad'), NO_WG8_FLOOR),
    row('wg8_2_4_4', (19, 4, 4, 512, 512, 3, 1, 1), same('conv3x3_wg8_kernel<{T}, 2, 4, 4>', 'fwd', 'fwd_relu', 'dgrad'), NO_WG8_FLOOR),
    row('wg8_bands', (3, 32, 32, 128, 128, 3, 1, 1), same('conv3x3_wg8_kernel<{T}, 4, 2, 32, 9, 2>', 'fwd', 'fwd_relu', 'dgrad'), NO_WG8_FLOOR),
    # ---- eight-wave 3x3 / stride 2 and its two-launch data gradient (NT = 2, then NT = 4)
    row('wg8s2_16', (5, 32, 32, 64, 128, 3, 2, 1), dict(same('conv3x3s2_wg8_kernel<{T}, 4, 2, 16>', 'fwd', 'fwd_relu'),
                                                        dgrad='conv3x3_wg8_kernel<{T}, 4, 2, 16, s2dgrad4>'), NO_WG8_FLOOR),
    row('wg8s2_8', (5, 16, 16, 128, 256, 3, 2, 1), dict(same('conv3x3s2_wg8_kernel<{T}, 2, 4, 8>', 'fwd', 'fwd_relu'),
                                                        dgrad='conv3x3_wg8_kernel<{T}, 2, 4, 8, s2dgrad4>'), NO_WG8_FLOOR),
    row('wg8s2_4', (19, 8, 8, 256, 512, 3, 2, 1), dict(same('conv3x3s2_wg8_kernel<{T}, 2, 4, 4>', 'fwd', 'fwd_relu'),
                                                       dgrad='conv3x3_wg8_kernel<{T}, 2, 4, 4, s2dgrad4>'), NO_WG8_FLOOR),
    # ---- four-wave halo kernels: bands of an image (ragged last band) and several images per tile (ragged last tile)
    row('halo_4_1_banded', (3, 18, 32, 64, 64, 3, 1, 1), same('conv3x3_halo_kernel<{T}, 4, 1>', 'fwd', 'fwd_relu', 'fwd_acc', 'dgrad', 'dgrad_acc')),
    row('halo_4_1_images', (5, 8, 8, 64, 48, 3, 1, 1), same('conv3x3_halo_kernel<{T}, 4, 1>', 'fwd', 'fwd_relu', 'fwd_acc')),
    row('halo_2_2_banded', (3, 16, 16, 128, 128, 3, 1, 1), same('conv3x3_halo_kernel<{T}, 2, 2>', 'fwd', 'fwd_relu', 'fwd_acc', 'dgrad', 'dgrad_acc')),
    row('halo_2_2_images', (3, 8, 8, 256, 256, 3, 1, 1), same('conv3x3_halo_kernel<{T}, 2, 2>', 'fwd', 'fwd_relu', 'fwd_acc', 'dgrad', 'dgrad_acc')),
    # ---- persistent halo kernels: 522 tiles on 512 workgroups
    row('halo_p_4_1', (261, 16, 32, 32, 64, 3, 1, 1), same('conv3x3_halo_pkernel<{T}, 4, 1>', 'fwd', 'fwd_relu', 'dgrad')),
    row('halo_p_2_2', (261, 16, 16, 64, 128, 3, 1, 1), same('conv3x3_halo_pkernel<{T}, 2, 2>', 'fwd', 'fwd_relu')),
    # ---- LDS-DMA implicit GEMM (planes the halo kernels do not take: 12 wide; 1x1 beyond the streaming pairs)
    row('dma_4_2', (9, 86, 85, 256, 128, 1, 1, 0), same('igemm_dma_kernel<T, 4, 2>', 'fwd', 'fwd_relu', 'fwd_acc', 'dgrad', 'dgrad_acc'),
        {'conv_tile_big': 1}),
    row('dma_2_2', (3, 9, 12, 64, 128, 3, 1, 1), dict(same('igemm_dma_kernel<T, 2, 2>', 'fwd', 'fwd_relu', 'fwd_acc'),
                                                      **same('igemm_dma_kernel<T, 4, 1>', 'dgrad', 'dgrad_acc'))),
    row('dma_4_1', (3, 9, 12, 128, 64, 3, 1, 1), dict(same('igemm_dma_kernel<T, 4, 1>', 'fwd', 'fwd_relu', 'fwd_acc'),
                                                      **same('igemm_dma_kernel<T, 2, 2>', 'dgrad', 'dgrad_acc'))),
    row('dma_s2_parity', (3, 18, 12, 64, 128, 3, 2, 1), dict(same('igemm_dma_kernel<T, 2, 2>', 'fwd', 'fwd_relu'),
                                                             **same('igemm_dma_kernel<T, 4, 1>', 'dgrad', 'dgrad_acc'))),
    row('dma_f32', (3, 9, 12, 64, 128, 3, 1, 1), dict(same('igemm_dma_kernel<T, 2, 2>', 'fwd', 'fwd_relu', 'fwd_acc'),
                                                      **same('igemm_dma_kernel<T, 4, 1>', 'dgrad', 'dgrad_acc')), dtypes=(F32,)),
    # ---- first-generation gather kernel: float32 channel counts off the K step, the 16-bit formats with conv_impl_v1 = 1, the prologue
    row('igemm_f32_narrow', (3, 9, 12, 24, 40, 3, 1, 1), same('igemm_kernel<T, 2, false>', 'fwd', 'fwd_relu', 'fwd_acc', 'dgrad', 'dgrad_acc'),
        dtypes=(F32,)),
    row('igemm_f32_wide', (3, 9, 12, 72, 136, 3, 2, 1), dict(same('igemm_kernel<T, 4, false>', 'fwd', 'fwd_relu', 'fwd_acc'),
                                                             **same('igemm_kernel<T, 4, false>', 'dgrad', 'dgrad_acc')), dtypes=(F32,)),
    row('igemm_v1_wide', (3, 9, 12, 64, 128, 3, 1, 1), dict(same('igemm_kernel<T, 4, false>', 'fwd', 'fwd_relu', 'fwd_acc'),
                                                            **same('igemm_kernel<T, 2, false>', 'dgrad', 'dgrad_acc')), {'conv_impl_v1': 1}),
    row('igemm_prologue_narrow', (3, 16, 16, 64, 64, 3, 1, 1), same('igemm_kernel<T, 2, true>', 'fwd_ss', 'fwd_ss_relu'), dtypes=(BF, F16, F32)),
    row('igemm_prologue_wide', (3, 16, 16, 64, 128, 3, 1, 1), same('igemm_kernel<T, 4, true>', 'fwd_ss', 'fwd_ss_relu'), dtypes=(BF, F16, F32)),
]


def tr(wco, wk, p2, mt):
    n = 'wgrad_tr_kernel<{T}, %d, %d, %d, mt%d>' % (wco, wk, p2, mt)
    return {'wgrad': n, 'wgrad_bias': n}


def halo_w(mt, ct, ks):
    n = 'wgrad_halo_kernel<{T}, %d, %d, %d>' % (mt, ct, ks)
    return {'wgrad': n, 'wgrad_bias': n}


HALO_FLOOR = {'wgrad_halo_min_m': 0}
SPLITS = {'wgrad_min_rows': 128}            # several pixel ranges per filter tile (float atomics), the last one ragged

WGRAD_ROWS = [
    # ---- band-resident kernel, ten (MT, CT, ks) shapes; odd heights: a partial last band
    row('wgrad_halo_1_1_3', (3, 10, 32, 16, 16, 3, 1, 1), halo_w(1, 1, 3), HALO_FLOOR),
    row('wgrad_halo_1_1_3_persistent', (300, 11, 32, 16, 16, 3, 1, 1), halo_w(1, 1, 3), HALO_FLOOR),     # 900 bands on 768 workgroups
    row('wgrad_halo_2_1_3', (2, 71, 128, 16, 32, 3, 1, 1), halo_w(2, 1, 3), HALO_FLOOR),
    row('wgrad_halo_2_2_3', (2, 35, 64, 32, 32, 3, 1, 1), halo_w(2, 2, 3), HALO_FLOOR),
    row('wgrad_halo_1_4_3', (2, 71, 128, 64, 16, 3, 1, 1), halo_w(1, 4, 3), HALO_FLOOR),
    row('wgrad_halo_1_2_3', (5, 7, 64, 32, 16, 3, 1, 1), halo_w(1, 2, 3), HALO_FLOOR),
    row('wgrad_halo_2_1_1', (2, 71, 128, 16, 32, 1, 1, 0), halo_w(2, 1, 1), HALO_FLOOR),
    row('wgrad_halo_1_4_1', (2, 71, 128, 64, 16, 1, 1, 0), halo_w(1, 4, 1), HALO_FLOOR),
    row('wgrad_halo_1_2_1', (3, 35, 64, 32, 16, 1, 1, 0), halo_w(1, 2, 1), HALO_FLOOR),
    row('wgrad_halo_4_2_1', (3, 35, 64, 32, 64, 1, 1, 0), halo_w(4, 2, 1), HALO_FLOOR),
    row('wgrad_halo_2_4_1', (3, 35, 64, 64, 32, 1, 1, 0), halo_w(2, 4, 1), HALO_FLOOR),
    # ---- 64 -> 64: fixed (32 x 32, 8-row bands; 268 bands on 256 workgroups) and generic (partial last band; 300 bands; forced tilings)
    row('wgrad_halo64_fixed', (67, 32, 32, 64, 64, 3, 1, 1), same('wgrad_halo64_kernel<{T}, fixed>', 'wgrad', 'wgrad_bias'), HALO_FLOOR),
    row('wgrad_halo64_generic_w64', (3, 21, 64, 64, 64, 3, 1, 1), same('wgrad_halo64_kernel<{T}>', 'wgrad', 'wgrad_bias'), HALO_FLOOR),
    row('wgrad_halo64_generic_persistent', (300, 6, 32, 64, 64, 3, 1, 1), same('wgrad_halo64_kernel<{T}>', 'wgrad', 'wgrad_bias'), HALO_FLOOR),
    row('wgrad_halo64_th4_nreg2', (5, 30, 32, 64, 64, 3, 1, 1), same('wgrad_halo64_kernel<{T}>', 'wgrad', 'wgrad_bias'),
        dict(HALO_FLOOR, wg64_th=4, wg64_nreg=2)),
    # ---- eight-wave 256 x 256 tiles, M = 576 pixels: three ranges of 192 (wgrad_min_rows = 256) as slabs + wgrad_slab_reduce_kernel; ONE
    # range (wgrad_min_rows = 2^20 >= M: wgrad_split cannot give more), written straight into dw; three ranges by atomics (no scratch)
    row('wgrad_wg8_slab', (9, 8, 8, 256, 256, 3, 1, 1), {'wgrad': 'wgrad_wg8_kernel<{T}, true>'}, {'wgrad_min_rows': 256}),
    row('wgrad_wg8_one_range', (9, 8, 8, 256, 256, 3, 1, 1), {'wgrad': 'wgrad_wg8_kernel<{T}, false>'}, {'wgrad_min_rows': 1 << 20}),
    row('wgrad_wg8_atomic', (9, 8, 8, 256, 256, 3, 1, 1), {'wgrad_nows': 'wgrad_wg8_kernel<{T}, false>'}, {'wgrad_min_rows': 256}),
    # ---- transposing-read kernel: every tile shape and address mode launch_wgrad picks, with and without the bias sums
    row('wgrad_tr_2_2_1', (19, 4, 4, 128, 128, 3, 1, 1), tr(2, 2, 1, 4), SPLITS),
    row('wgrad_tr_2_2_2', (3, 9, 16, 128, 128, 3, 1, 1), tr(2, 2, 2, 4), SPLITS),
    row('wgrad_tr_2_2_0', (3, 9, 12, 64, 128, 3, 1, 1), tr(2, 2, 0, 4), SPLITS),
    row('wgrad_tr_2_2_1_s2', (5, 16, 16, 64, 128, 3, 2, 1), tr(2, 2, 1, 4)),
    row('wgrad_tr_1_3_1', (19, 4, 4, 64, 64, 3, 1, 1), tr(1, 3, 1, 4), SPLITS),
    row('wgrad_tr_1_4_1', (19, 4, 4, 32, 64, 3, 1, 1), tr(1, 4, 1, 4), SPLITS),
    row('wgrad_tr_1_4_2_mt1', (3, 9, 16, 32, 16, 3, 1, 1), tr(1, 4, 2, 1), SPLITS),
    row('wgrad_tr_1_4_2_mt2', (3, 9, 16, 32, 32, 3, 1, 1), tr(1, 4, 2, 2), SPLITS),
    row('wgrad_tr_1_4_2_mt4', (3, 9, 16, 32, 64, 3, 1, 1), tr(1, 4, 2, 4), SPLITS),
    row('wgrad_tr_1_4_0', (3, 9, 12, 32, 48, 3, 1, 1), tr(1, 4, 0, 4), SPLITS),
    # ---- first-generation kernel: float32, the 16-bit formats with conv_impl_v1 = 1, the prologue; bias_grad_kernel behind it
    row('wgrad_v0_f32_narrow', (3, 9, 12, 24, 40, 3, 1, 1), dict(same('wgrad_kernel<T, 2, false>', 'wgrad', 'wgrad_bias'),
                                                                 bias_grad=None, **same('wgrad_kernel<T, 2, true>', 'wgrad_ss', 'wgrad_ss_relu')),
        dtypes=(F32,)),
    row('wgrad_v0_f32_wide', (5, 9, 12, 72, 136, 3, 2, 1), dict(same('wgrad_kernel<T, 4, false>', 'wgrad', 'wgrad_bias'),
                                                                bias_grad=None, **same('wgrad_kernel<T, 4, true>', 'wgrad_ss', 'wgrad_ss_relu')),
        dtypes=(F32,)),
    row('wgrad_v0_16bit_narrow', (3, 9, 12, 64, 64, 3, 1, 1), dict(same('wgrad_kernel<T, 2, false>', 'wgrad', 'wgrad_bias'), bias_grad=None),
        {'conv_impl_v1': 1}),
    row('wgrad_v0_16bit_wide', (3, 9, 12, 64, 128, 3, 1, 1), dict(same('wgrad_kernel<T, 4, false>', 'wgrad', 'wgrad_bias'), bias_grad=None),
        {'conv_impl_v1': 1}),
    row('wgrad_prologue_narrow', (3, 16, 16, 64, 64, 3, 1, 1), same('wgrad_kernel<T, 2, true>', 'wgrad_ss', 'wgrad_ss_relu')),
    row('wgrad_prologue_wide', (3, 16, 16, 64, 128, 3, 1, 1), same('wgrad_kernel<T, 4, true>', 'wgrad_ss', 'wgrad_ss_relu')),
]


def params(rows):
    return [pytest.param(r, dt, id='%s-%s' % (r['id'], ec.DT_ID[dt])) for r in rows for dt in r['dtypes']]


@REGIMES
@pytest.mark.parametrize('r,dtype', params(CONV_ROWS))
def test_convolution_forward_and_data_gradient_exact(calls, r, dtype, regime):
    ec.run_conv_row(calls, r, dtype, regime)


@REGIMES
@pytest.mark.parametrize('r,dtype', params(WGRAD_ROWS))
def test_convolution_weight_gradient_exact(calls, r, dtype, regime):
    ec.run_wgrad_row(calls, r, dtype, regime)


twice = ec.launch_twice          # guard plane, kernel name, a second launch: for the entry points outside the two tables too


@REGIMES
@pytest.mark.parametrize('hdt', ec.HALVES, ids=['bf16', 'f16'])
@pytest.mark.parametrize('geom', [(8, 65, 128, 16, 32), (28, 37, 64, 32, 64)], ids=['65x128', '37x64'])
def test_convolution_with_statistics_writes_the_exact_output(calls, geom, hdt, regime):
    """eve_conv2d_fwd_stats: y exactly (the statistics are test_gpu_instnorm_conditioning.py's)."""
    N, H, W, cin, cout = geom
    xv, wv, _ = ec.value_sets(regime, hdt, 9 * cin)
    x, w = ec.pick((N, H, W, cin), xv, 21, hdt), ec.pick((cout, 3, 3, cin), wv, 22, hdt)
    bias = ec.gen_bias(cout, regime, hdt, 9 * cin, 23)
    want = ec.ref_fwd(x, w, bias, 1, 1, 'fwd_stats')
    ec.check_regime(want, hdt, regime, 'fwd_stats %dx%d' % (H, W))
    xd, wd, bd = x.cuda(), w.cuda(), bias.cuda()
    mr = torch.zeros((N, cout, 2), device='cuda')

    def fn(y):
        assert calls.fwd_stats(xd, wd, bd, 1, 1, 0, y, mr), 'the statistics were not written'
    y = twice(calls, 'fwd_stats', 'conv3x3_stream_kernel<{T}, %d, %d, false>' % (cin, cout), hdt, (N, H, W, cout), hdt, None, fn)
    ec.check_exact(y, ec.round_once(want, hdt), 'fwd_stats y')
    assert bool(torch.isfinite(mr).all())


@REGIMES
@pytest.mark.parametrize('hdt', ec.HALVES, ids=['bf16', 'f16'])
@pytest.mark.parametrize('N', [3, 35], ids=['N3', 'N35-second-turn'])
def test_stem_kernels_exact(calls, N, hdt, regime):
    """stem7x7_kernel through eve_stem7x7s2_fwd (K = 147, no bias: the larger operands of ec.plain_value_sets carry the rounding regime;
    N = 35: 2 240 wave tiles on 512 workgroups of four, a second turn of the grid), eve_stem_wgrad (float32, onto integers) and
    eve_stem_dgrad with its packing (float32) at C = 3."""
    import ctypes
    hip = calls.hip
    xv, wv, _ = ec.plain_value_sets(regime, hdt, 147)
    src = ec.pick((N, 3, 128, 128), xv, 31)
    w = ec.pick((64, 7, 7, 8), wv, 32, hdt)
    w[..., 3:] = 0
    x_nhwc = src.permute(0, 2, 3, 1).contiguous()
    xp = hip.stem_pack_input(src.cuda(), dtype=hdt)
    assert torch.equal(xp[:, 3:131, 4:132, :3].float().cpu(), x_nhwc), 'the operands must be exact in the storage format'
    want = ec.ref_fwd(x_nhwc, w[..., :3], None, 2, 3, 'stem fwd')
    ec.check_regime(want, hdt, regime, 'stem fwd')
    wd = w.cuda()
    from eve_amd.kernels import dt_code
    got = twice(calls, 'stem fwd', 'stem7x7_kernel<{T}, 2>', hdt, (N, 64, 64, 64), hdt, None,
                lambda y: hip._ck(hip.lib.eve_stem7x7s2_fwd(dt_code(hdt), N, 128, 128, hip._p(xp), hip._p(wd), hip._p(y), hip._stream())))
    ec.check_exact(got, ec.round_once(want, hdt), 'stem fwd')
    # weight gradient from the packed patches: dw [64, 7, 8, 4], column 7 / channel 3 unused
    # (float32 outputs from here on: the bf16 value sets, so that N x 64 x 64 products stay below 2^24 in float16 too)
    xw, dv, _ = ec.value_sets(regime, torch.bfloat16, 147)
    src_w = ec.pick((N, 3, 128, 128), xw, 36)
    xpw = hip.stem_pack_input(src_w.cuda(), dtype=hdt)
    dconv = ec.pick((N, 64, 64, 64), dv, 33, hdt)
    dconvd = dconv.cuda()
    ref_dw, _ = ec.ref_wgrad(src_w.permute(0, 2, 3, 1).contiguous(), dconv, 7, 7, 2, 3, 'stem wgrad')
    dw0 = ec.big_ints((64, 7, 8, 4), 300, 900, 34)
    dw = twice(calls, 'stem wgrad', 'wgrad_tr_kernel<{T}, 1, 4, 1, mt4>', hdt, (64, 7, 8, 4), torch.float32, dw0,
               lambda out: hip.stem_wgrad(xpw, dconvd, out))
    ec.check_exact(dw[:, :, :7, :3], ref_dw + dw0[:, :, :7, :3].double(), 'stem wgrad', ('o', 'kh', 'kw', 'i'))
    # data gradient to the patch: float32 NCHW
    w_oihw = ec.pick((64, 3, 7, 7), dv, 35)
    packed = hip.stem_dgrad_pack(w_oihw.cuda(), hdt)
    want_dx = ec.ref_dgrad(dconv, w_oihw.permute(1, 2, 3, 0).contiguous(), (128, 128), 2, 3, 'stem dgrad').permute(0, 3, 1, 2)
    dx = twice(calls, 'stem dgrad', 'stem_dgrad_kernel', hdt, (N, 3, 128, 128), torch.float32, None,
               lambda out: hip.stem_dgrad(dconvd, packed, 3, out=out))
    ec.check_exact(dx, want_dx, 'stem dgrad', 'nchw')


@REGIMES
@pytest.mark.parametrize('shape', [(1920, 512, 128), (37, 130, 128), (60, 128, 384), (1920, 128, 4), (5, 7, 3)], ids=lambda s: 'x'.join(map(str, s)))
def test_small_linear_kernels_exact(calls, shape, regime):
    """eve_linear_fwd / _dgrad / _wgrad, their _ex forms and eve_linear_wgrad_batch, float32, no activation: exact integers; every
    output caller-owned with a guard plane behind it, every launch twice."""
    hip = calls.hip
    M, K, N = shape
    f32 = torch.float32
    xv, wv, _ = ec.value_sets(regime, torch.bfloat16, 1)
    x, w, dy = ec.pick((M, K), xv, 41), ec.pick((N, K), wv, 42), ec.pick((M, N), xv, 43)
    b = ec.big_ints((N,), 300, 900, 44)
    ec.assert_below_2_24(16.0 * max(M, K, N) + 900 * 2, 'linear')
    wt = w.t().contiguous()
    xd, wd, wtd, dyd, bd = x.cuda(), w.cuda(), wt.cuda(), dy.cuda(), b.cuda()
    y64 = x.double() @ wt.double() + b.double()
    y = twice(calls, 'linear fwd', None, f32, (M, N), f32, None,
              lambda out: hip._ck(hip.lib.eve_linear_fwd(M, K, N, hip._p(xd), hip._p(wtd), hip._p(bd), 0, hip._p(out), hip._stream())))
    ec.check_exact(y, y64, 'linear fwd', ('m', 'n'))
    ld = N + 4
    wide = twice(calls, 'linear fwd_ex', None, f32, (M, ld), f32, None, lambda out: hip.linear_fwd_ex(xd, K, wtd, bd, 0, out))
    ec.check_exact(wide[:, :N], y64, 'linear fwd_ex', ('m', 'n'))
    assert bool((wide[:, N:] == ec.GUARD_VALUE).all())
    dx64 = dy.double() @ w.double()
    dx = twice(calls, 'linear dgrad', None, f32, (M, K), f32, None,
               lambda out: hip._ck(hip.lib.eve_linear_dgrad(M, K, N, hip._p(dyd), None, 0, hip._p(wd), hip._p(out), hip._stream())))
    ec.check_exact(dx, dx64, 'linear dgrad', ('m', 'k'))
    base = ec.big_ints((M, K), 300, 900, 45)
    dyw = torch.full((M, ld), 7.0)
    dyw[:, :N] = dy
    dywd = dyw.cuda()
    dx = twice(calls, 'linear dgrad_ex', None, f32, (M, K), f32, base, lambda out: hip.linear_dgrad_ex(dywd, N, None, 0, wd, out, accumulate=True))
    ec.check_exact(dx, dx64 + base.double(), 'linear dgrad_ex +=', ('m', 'k'))
    dw0, db0 = ec.big_ints((N, K), 300, 900, 46), ec.big_ints((N,), 300, 900, 47)
    dw64, db64 = dy.double().t() @ x.double() + dw0.double(), dy.double().sum(0) + db0.double()
    both = torch.cat([dw0.reshape(-1), db0])               # one buffer: the guard plane sits behind db

    def split(out):
        return out[:N * K].view(N, K), out[N * K:]
    for what, name, fn in (('linear wgrad', None, lambda out: hip.linear_wgrad(dyd, None, 0, xd, *split(out))),
                           ('linear wgrad_batch', 'linear_wgrad_batch_kernel',
                            lambda out: hip.linear_wgrad_batch([{'dY': dyd, 'X': xd, 'dW': split(out)[0], 'db': split(out)[1]}]))):
        got = twice(calls, what, name, f32, (both.numel(),), f32, both, fn)
        ec.check_exact(split(got)[0], dw64, what + ' dw', ('n', 'k'))
        ec.check_exact(split(got)[1], db64, what + ' db', ('n',))
