"""GPU: the eight-wave 128 x 384 weight-gradient tile (csrc/wgrad_wg8_t128.h), bit for bit on integer-valued operands the way
tests/test_gpu_conv_exact.py does it (tests/exact_conv.py: both regimes, both 16-bit formats, guard plane, every output twice, the
reported kernel asserted), its dispatch floor, and its rounding against wgrad_tr_kernel on random operands.

Every table row sets wgrad_wg8 = 2 (the tile at any pixel count); each shape is the smallest at which what it exercises can go wrong.
"""
import pytest
import torch

import exact_conv as ec

pytestmark = pytest.mark.gpu

REGIMES = pytest.mark.parametrize('regime', ['exact', 'rounding'])
SLAB, DIRECT = 'wgrad_wg8_t128_kernel<{T}, true>', 'wgrad_wg8_t128_kernel<{T}, false>'
TR = 'wgrad_tr_kernel<{T}, 2, 2, 1, mt4>'


@pytest.fixture(scope='module')
def calls():
    from eve_amd.kernels import HipKernels
    assert torch.cuda.is_available(), 'GPU suite needs a GPU'
    return ec.HipCalls(HipKernels())


def row(id, shape, ops, **override):
    return {'id': id, 'shape': shape, 'ops': ops, 'override': dict(override, wgrad_wg8=2), 'dtypes': ec.HALVES}


# shape = (N, H, W, Cin, Cout, ks, stride, pad)
ROWS = [
    # the sibling of wgrad_tr_2_2_1: M = 304 = three pixel ranges of 128 / 128 / 48, the last one a step and a half (zero fill inside a
    # step); 4 x 4 planes, so every tap leaves the image and a 32-pixel step spans two images
    row('t128_ragged_ranges', (19, 4, 4, 128, 128, 3, 1, 1), {'wgrad': SLAB}, wgrad_min_rows=128),
    # a 32-pixel step spans two image rows; five ranges as slabs + wgrad_slab_reduce_kernel, and by float atomics (no scratch)
    row('t128_slab_and_atomic', (5, 16, 16, 128, 128, 3, 1, 1), {'wgrad': SLAB, 'wgrad_nows': DIRECT}, wgrad_min_rows=256),
    # ONE range (wgrad_min_rows >= M: wgrad_split cannot give more), written straight into dw, no reduce launch
    row('t128_one_range', (5, 8, 8, 128, 128, 3, 1, 1), {'wgrad': DIRECT}, wgrad_min_rows=1 << 20),
    # layer 3's stride-2 convolution: two channel tiles (six workgroups per range: the XCD remap), M = 320
    row('t128_stride2_two_channel_tiles', (5, 16, 16, 128, 256, 3, 2, 1), {'wgrad': DIRECT}),
    # 32 x 32 planes (the fp16 workload's layer 2): a step inside one image row; M = 3 072 = two ranges
    row('t128_32x32_planes', (3, 32, 32, 128, 128, 3, 1, 1), {'wgrad': SLAB}),
    # M = 1 040 = 17 ranges of 64 (the last one 16 pixels, half a step): wgrad_slab_reduce_wide_kernel's eight slab groups take
    # three, two, ... slabs each
    row('t128_many_slabs', (65, 4, 4, 128, 128, 3, 1, 1), {'wgrad': SLAB}, wgrad_min_rows=64),
]


@REGIMES
@pytest.mark.parametrize('r,dtype', [pytest.param(r, dt, id='%s-%s' % (r['id'], ec.DT_ID[dt])) for r in ROWS for dt in r['dtypes']])
def test_tile128_weight_gradient_exact(calls, r, dtype, regime):
    ec.run_wgrad_row(calls, r, dtype, regime)


def _wgrad(calls, x, dy, stride=1):
    dw = torch.zeros((dy.shape[3], 3, 3, x.shape[3]), dtype=torch.float32, device='cuda')
    calls.wgrad(x, dy, 3, 3, stride, 1, dw)
    return dw, calls.last()


@pytest.mark.parametrize('dtype', ec.HALVES, ids=['bf16', 'f16'])
def test_tile128_dispatch_floor_and_switch(calls, dtype):
    """Default configuration: below the pixel floor (M = 304, and M = 65 520, one image short of it) the layer-2 shape stays on
    wgrad_tr_kernel, at the floor (M = 65 536) it is the new tile; wgrad_wg8 = 3 (256 x 256 only) and 0 send the shape at the floor
    to wgrad_tr_kernel as well."""
    g = torch.Generator().manual_seed(3)
    for N, want, override in ((19, TR, {}), (4095, TR, {}), (4096, SLAB, {}), (4096, TR, {'wgrad_wg8': 3}), (4096, TR, {'wgrad_wg8': 0})):
        x = torch.randn((N, 4, 4, 128), generator=g).to(dtype).cuda()
        dy = torch.randn((N, 4, 4, 128), generator=g).to(dtype).cuda()
        with calls.override(**override):
            _, used = _wgrad(calls, x, dy)
        assert used == ec.kname(want, dtype), (N, override, used)


@pytest.mark.parametrize('dtype', ec.HALVES, ids=['bf16', 'f16'])
def test_tile128_random_operands_against_float64(calls, dtype):
    """Random operands, shape (40, 16, 16, 128, 128): the new tile and wgrad_tr_kernel (wgrad_wg8 = 3) each against a float64 CPU
    reference on the same 16-bit inputs.  Both add the same float32 products in a different order, so the new tile's relative L2
    error may be at most twice wgrad_tr_kernel's.
    Measured (MI355X): bf16 2.228e-07 (new) against 2.221e-07 (wgrad_tr_kernel), f16 2.443e-07 against 2.444e-07."""
    g = torch.Generator().manual_seed(41)
    x = torch.randn((40, 16, 16, 128), generator=g).to(dtype)
    dy = (0.05 * torch.randn((40, 16, 16, 128), generator=g)).to(dtype)
    with ec.reference_threads():
        ref = torch.nn.grad.conv2d_weight(ec.nchw(x, torch.float64), (128, 128, 3, 3), ec.nchw(dy, torch.float64), 1, 1).permute(0, 2, 3, 1)
    xd, dyd = x.cuda(), dy.cuda()
    err = {}
    for name, want, override in (('new', SLAB, {'wgrad_wg8': 2}), ('tr', TR, {'wgrad_wg8': 3})):
        with calls.override(**override):
            dw, used = _wgrad(calls, xd, dyd)
        assert used == ec.kname(want, dtype), used
        err[name] = float((dw.cpu().double() - ref).norm() / ref.norm())
    print('relative L2 error against float64, %s: new tile %.3e  wgrad_tr_kernel %.3e' % (ec.DT_ID[dtype], err['new'], err['tr']))
    assert err['new'] <= 2 * err['tr'], err
