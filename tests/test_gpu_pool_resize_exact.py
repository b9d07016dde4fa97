"""GPU: the pooling, resize, layout and cast kernels of eve_amd/csrc/pool_resize.hip against the float64 reference of
tests/pool_resize_ref.py (pinned against ATen by tests/test_pool_resize_host.py), at odd shapes, single channel vectors, 1-pixel
axes, rows longer than one 256-thread pass and launches beyond the grid caps.

Selection, copy and cast kernels are held to equality, indices included; sums and interpolation to bounds derived in
pool_resize_ref.py from the float32 operations the kernels perform (printed as max err / bound, which must stay <= 1).
test_gpu_kernels.py::test_pooling_and_resize / test_layout_and_pack remain the workload-shape checks."""
import pytest
import torch

import pool_resize_ref as R
from fake_kernels import FakeKernels
from test_gpu_kernels import DTYPES, DT_IDS, close, dev, hip, rnd  # noqa: F401  (hip: the module-scoped fixture)

pytestmark = pytest.mark.gpu

F64 = torch.float64
BY_DTYPE = pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
KINDS = pytest.mark.parametrize('kind', R.INPUT_KINDS)
SENTINEL = 0x5A


def ident(s):
    return 'x'.join(map(str, s))


def dt_code(dtype):
    from eve_amd.kernels import dt_code as code
    return code(dtype)


def bits(t):
    """The tensor's bit patterns as integers (equality that tells -0 from +0)."""
    return t.contiguous().cpu().view(torch.int32 if t.element_size() == 4 else torch.int16)


def within(what, got, want64, bound):
    err = (got.detach().cpu().to(F64) - want64).abs()
    r = R.ratio(err, bound)
    print('%-58s max|err| %.3e  max err/bound %.4f' % (what, float(err.max()) if err.numel() else 0.0, r))
    assert r <= 1.0, '%s: an entry is %.3f x its bound away from float64' % (what, r)


# ------------------------------------------------------------------------------------------------ max-pool 3x3 / s2
def check_maxpool(hip, shape, kind, dtype, seed):
    N, IH, IW, C = shape
    x = R.make_input(kind, shape, dtype, seed)
    y_w, idx_w = R.maxpool3x3s2(x)
    y_g, code_g = hip.maxpool3x3s2_fwd(dev(x))
    assert torch.equal(y_g.cpu(), y_w.to(dtype)), 'values'
    assert torch.equal(R.window_code_to_flat(code_g, (IH, IW)), idx_w), 'window code vs the first maximum in row-major order'
    dy = R.integer_grad(tuple(y_w.shape), dtype, seed + 1)
    assert torch.equal(hip.maxpool3x3s2_bwd(dev(dy), code_g, (IH, IW)).cpu(), R.route(dy, idx_w, (IH, IW)).to(dtype)), 'routing'
    dy = rnd(tuple(y_w.shape), dtype, seed + 2)
    within('maxpool bwd %s %s %s' % (ident(shape), kind, dtype), hip.maxpool3x3s2_bwd(dev(dy), code_g, (IH, IW)),
           R.route(dy, idx_w, (IH, IW)), R.pool_bwd_bound(dy, idx_w, (IH, IW), dtype))


@BY_DTYPE
@KINDS
def test_maxpool_values_window_codes_and_routing(hip, dtype, kind):
    for i, shape in enumerate(R.maxpool_shapes(R.vec_of(dtype))):
        check_maxpool(hip, shape, kind, dtype, 1000 + 10 * i)


@BY_DTYPE
def test_maxpool_beyond_the_grid_cap(hip, dtype):
    shape = R.maxpool_cap_shape(R.vec_of(dtype))
    N, IH, IW, C = shape
    assert N * ((IH - 1) // 2 + 1) * ((IW - 1) // 2 + 1) * C // R.vec_of(dtype) > 2048 * 256
    check_maxpool(hip, shape, 'levels', dtype, 1100)


@BY_DTYPE
def test_maxpool_nan_wins_its_window(hip, dtype):
    shape = (2, 7, 9, R.vec_of(dtype))
    g = torch.Generator().manual_seed(1200)
    x = R.make_input('random', shape, dtype, 1201)
    x[torch.rand(shape, generator=g) < 0.08] = float('nan')
    y_w, idx_w = R.maxpool3x3s2(x)
    holds_nan = R.maxpool3x3s2(torch.isnan(x).to(F64))[0] > 0
    assert torch.equal(torch.isnan(y_w), holds_nan) and bool(holds_nan.any()) and not bool(holds_nan.all())
    y_g, code_g = hip.maxpool3x3s2_fwd(dev(x))
    assert torch.equal(torch.isnan(y_g.cpu()), holds_nan), 'NaN exactly where the window holds one'
    assert torch.equal(y_g.cpu()[~holds_nan], y_w.to(dtype)[~holds_nan])
    flat_g = R.window_code_to_flat(code_g, shape[1:3])
    assert torch.equal(flat_g[~holds_nan], idx_w[~holds_nan])
    picked = torch.gather(x.reshape(shape[0], -1, shape[3]), 1, flat_g.reshape(shape[0], -1, shape[3])).reshape(flat_g.shape)
    assert bool(torch.isnan(picked[holds_nan]).all()), 'a NaN window points at one of its NaNs'
    dy = R.integer_grad(tuple(y_w.shape), dtype, 1202)
    assert torch.equal(hip.maxpool3x3s2_bwd(dev(dy), code_g, shape[1:3]).cpu(), R.route(dy, flat_g, shape[1:3]).to(dtype))


# ------------------------------------------------------------------------------------------------ adaptive max-pool
def check_adaptive(hip, shape, kind, dtype, seed):
    N, IH, IW, OH, OW, C = shape
    x = R.make_input(kind, (N, IH, IW, C), dtype, seed)
    y_w, idx_w = R.adaptive_maxpool(x, (OH, OW))
    y_g, idx_g = hip.adaptive_maxpool_fwd(dev(x), (OH, OW))
    assert torch.equal(y_g.cpu(), y_w.to(dtype)), 'values'
    assert torch.equal(idx_g.cpu().long(), idx_w), 'arg-max'
    if (OH, OW) == (IH, IW):
        assert torch.equal(y_g.cpu(), x)
        assert torch.equal(idx_g.cpu().long(), torch.arange(IH * IW).view(1, IH, IW, 1).expand(N, IH, IW, C))
    dy = R.integer_grad(tuple(y_w.shape), dtype, seed + 1)
    assert torch.equal(hip.adaptive_maxpool_bwd(dev(dy), idx_g, (IH, IW)).cpu(), R.route(dy, idx_w, (IH, IW)).to(dtype)), 'routing'
    dy = rnd(tuple(y_w.shape), dtype, seed + 2)
    plain = hip.adaptive_maxpool_bwd(dev(dy), idx_g, (IH, IW))
    within('adaptive bwd %s %s %s' % (ident(shape), kind, dtype), plain, R.route(dy, idx_w, (IH, IW)),
           R.pool_bwd_bound(dy, idx_w, (IH, IW), dtype))
    skipg = dev(rnd((N, IH, IW, C), dtype, seed + 3))
    assert torch.equal(hip.adaptive_maxpool_bwd(dev(dy), idx_g, (IH, IW), add=skipg), hip.add(plain, skipg)), 'add= epilogue'


@BY_DTYPE
@KINDS
def test_adaptive_maxpool_values_indices_and_routing(hip, dtype, kind):
    for i, shape in enumerate(R.adaptive_shapes(R.vec_of(dtype))):
        check_adaptive(hip, shape, kind, dtype, 2000 + 10 * i)


def test_adaptive_maxpool_beyond_the_row_cap(hip):
    shape = R.adaptive_cap_shape(8)
    assert shape[0] * shape[3] > 8192
    check_adaptive(hip, shape, 'levels', torch.bfloat16, 2100)


@BY_DTYPE
def test_adaptive_maxpool_nan_wins_its_window(hip, dtype):
    N, IH, IW, OH, OW, C = (2, 9, 16, 5, 8, R.vec_of(dtype))
    g = torch.Generator().manual_seed(2200)
    x = R.make_input('random', (N, IH, IW, C), dtype, 2201)
    x[torch.rand(x.shape, generator=g) < 0.05] = float('nan')
    y_w, idx_w = R.adaptive_maxpool(x, (OH, OW))
    holds_nan = torch.isnan(y_w)
    assert torch.equal(holds_nan, R.adaptive_maxpool(torch.isnan(x).to(F64), (OH, OW))[0] > 0) and bool(holds_nan.any())
    y_g, idx_g = hip.adaptive_maxpool_fwd(dev(x), (OH, OW))
    assert torch.equal(torch.isnan(y_g.cpu()), holds_nan)
    assert torch.equal(y_g.cpu()[~holds_nan], y_w.to(dtype)[~holds_nan])
    flat_g = idx_g.cpu().long()
    assert torch.equal(flat_g[~holds_nan], idx_w[~holds_nan])
    # a NaN window points at a NaN inside that window
    picked = torch.gather(x.reshape(N, -1, C), 1, flat_g.reshape(N, -1, C)).reshape(flat_g.shape)
    assert bool(torch.isnan(picked[holds_nan]).all())
    for oh in range(OH):
        for ow in range(OW):
            (h0, h1), (w0, w1) = R._ad_window(oh, IH, OH), R._ad_window(ow, IW, OW)
            f = flat_g[:, oh, ow]
            assert bool(((f // IW >= h0) & (f // IW < h1) & (f % IW >= w0) & (f % IW < w1)).all())
    dy = R.integer_grad(tuple(y_w.shape), dtype, 2202)
    assert torch.equal(hip.adaptive_maxpool_bwd(dev(dy), idx_g, (IH, IW)).cpu(), R.route(dy, flat_g, (IH, IW)).to(dtype))


# ------------------------------------------------------------------------------------------------ bilinear
def check_bilinear(hip, shape, dtype, seed):
    N, IH, IW, OH, OW, C = shape
    x, dy = rnd((N, IH, IW, C), dtype, seed), rnd((N, OH, OW, C), dtype, seed + 1)
    y_g, dx_g = hip.bilinear_fwd(dev(x), (OH, OW)), hip.bilinear_bwd(dev(dy), (IH, IW))
    within('bilinear fwd %s %s' % (ident(shape), dtype), y_g, R.bilinear_fwd(x, (OH, OW)), R.bilinear_fwd_bound(x, (OH, OW), dtype))
    within('bilinear bwd %s %s' % (ident(shape), dtype), dx_g, R.bilinear_bwd(dy, (IH, IW)), R.bilinear_bwd_bound(dy, (IH, IW), dtype))
    if (OH, OW) == (IH, IW):
        assert torch.equal(y_g.cpu(), x) and torch.equal(dx_g.cpu(), dy), 'identity'
    if dtype == torch.float32:
        # the adjoint identity <fwd(x), dy> = <x, bwd(dy)>, both inner products in float64 from the kernel outputs: each side
        # is off its exact value by at most the sum of |other operand| * bound
        lhs, rhs = float((y_g.cpu().to(F64) * dy.to(F64)).sum()), float((x.to(F64) * dx_g.cpu().to(F64)).sum())
        slack = float((dy.to(F64).abs() * R.bilinear_fwd_bound(x, (OH, OW), dtype)).sum() +
                      (x.to(F64).abs() * R.bilinear_bwd_bound(dy, (IH, IW), dtype)).sum())
        print('%-58s |<fwd x, dy> - <x, bwd dy>| / bound %.4f' % ('bilinear adjoint %s' % ident(shape), abs(lhs - rhs) / slack))
        assert abs(lhs - rhs) <= slack
        # every output pixel's weights sum to 1: bwd(ones) sums to OH * OW per image and channel
        ones = torch.ones((N, OH, OW, C))
        tot = hip.bilinear_bwd(dev(ones), (IH, IW)).cpu().to(F64).sum(dim=(1, 2))
        room = R.bilinear_bwd_bound(ones, (IH, IW), dtype).sum(dim=(1, 2))
        print('%-58s |sum - OH OW| / bound %.4f' % ('bilinear bwd(ones) %s' % ident(shape), R.ratio((tot - OH * OW).abs(), room)))
        assert bool(((tot - OH * OW).abs() <= room).all())


@BY_DTYPE
@pytest.mark.parametrize('case', range(len(R.bilinear_shapes(4))), ids=[ident(s[1:5]) + ('_4vec' if s[5] > 4 else '') for s in R.bilinear_shapes(4)])
def test_bilinear_both_directions_within_the_derived_bound(hip, dtype, case):
    check_bilinear(hip, R.bilinear_shapes(R.vec_of(dtype))[case], dtype, 3000 + 10 * case)


@BY_DTYPE
def test_bilinear_beyond_the_row_cap(hip, dtype):
    shape = R.bilinear_cap_shape(R.vec_of(dtype))
    assert shape[0] * shape[3] > 8192 and shape[0] * shape[1] > 8192
    check_bilinear(hip, shape, dtype, 3200)


@BY_DTYPE
def test_bilinear_exact_2x_upscale_of_multiples_of_16(hip, dtype):
    """Weights are multiples of 1/16 and inputs multiples of 16 with |x| <= 112: every product and sum is an integer below 2^8,
    exact in all three formats."""
    g = torch.Generator().manual_seed(3300)
    x = (torch.randint(-7, 8, (2, 5, 7, R.vec_of(dtype)), generator=g) * 16).to(dtype)
    want = R.bilinear_fwd(x, (10, 14))
    assert torch.equal(want, want.round()) and float(want.abs().max()) <= 112
    assert torch.equal(hip.bilinear_fwd(dev(x), (10, 14)).cpu(), want.to(dtype))


# ------------------------------------------------------------------------------------------------ average pool
@BY_DTYPE
@pytest.mark.parametrize('hw', [(1, 1), (3, 5), (4, 4), (7, 7), (16, 16)], ids=ident)
def test_avgpool_and_its_float32_side_variants(hip, dtype, hw):
    vec = R.vec_of(dtype)
    HW = hw[0] * hw[1]
    for C in (vec, 3 * vec, 512):
        for N in (1, 7):
            x, dy = rnd((N, hw[0], hw[1], C), dtype, 4000 + C + N), rnd((N, C), dtype, 4001 + C + N)
            y_g, dx_g = hip.avgpool_fwd(dev(x)), hip.avgpool_bwd(dev(dy), hw)
            what = 'avgpool %%s N%d %s C%d %s' % (N, ident(hw), C, dtype)
            within(what % 'fwd', y_g, R.avgpool(x), R.avgpool_fwd_bound(x, dtype))
            if HW & (HW - 1) == 0:                    # a power of two: the division is exact
                assert torch.equal(dx_g.cpu(), (dy.float() / HW).to(dtype)[:, None, None, :].expand(N, hw[0], hw[1], C))
            else:
                within(what % 'bwd', dx_g, R.avgpool_adjoint(dy, hw), R.avgpool_bwd_bound(dy, hw, dtype))
            # the float32-side variants: pool in the format, then cast -- bit for bit
            y32 = hip.avgpool_fwd_f32(dev(x))
            assert y32.dtype == torch.float32 and torch.equal(y32, y_g.float())
            dy32 = dev(rnd((N, C), torch.float32, 4002 + C + N))
            dx = hip.avgpool_bwd_f32(dy32, hw, dtype)
            assert dx.dtype == dtype and torch.equal(dx, hip.avgpool_bwd(dy32.to(dtype), hw))


# ------------------------------------------------------------------------------------------------ layout and cast
def specials():
    """float32 values at the edges of the three formats: signed zeros, infinities, NaN, denormals, the smallest and largest
    normals, float16 overflow, and exact round-to-nearest-even ties."""
    inf, tiny32 = float('inf'), 2.0 ** -126
    v = [0.0, -0.0, inf, -inf, float('nan'),
         2.0 ** -149, -2.0 ** -149, 1e-40, -1e-40, tiny32 * (1 - 2.0 ** -23),         # float32 denormals
         tiny32, -tiny32, 2.0 ** -133, 3 * 2.0 ** -134, 2.0 ** -134,                 # bf16: smallest normal, subnormals, a tie to 0
         float.fromhex('0x1.fep127'), float.fromhex('0x1.fffffep127'), float.fromhex('0x1.ffp127'),   # bf16 max, f32 max -> inf, tie -> inf
         2.0 ** -14, -2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -14 - 2.0 ** -25,    # fp16 normal / subnormal edges
         65504.0, 65519.0, 65519.99, 65520.0, -65520.0, 1e5, -1e5,                   # fp16: max, still finite, the tie, overflow
         1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -23, 1 + 2.0 ** -8 - 2.0 ** -23,   # bf16 ties
         1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 3 * 2.0 ** -11), 1 + 2.0 ** -11 + 2.0 ** -23, 1 + 2.0 ** -11 - 2.0 ** -23]  # fp16 ties
    return torch.tensor(v, dtype=torch.float64).float()


def assert_same_numbers(got, want, what):
    """Bit-equal, NaNs compared with isnan (not by payload)."""
    got, want = got.cpu(), want.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, what
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), '%s: NaN positions' % what
    gb, wb = bits(got), bits(want)
    bad = (gb != wb) & ~nan
    assert not bool(bad.any()), '%s: %d entries differ in bits, first at %s: got %s want %s' % (
        what, int(bad.sum()), bad.nonzero()[0].tolist(), got[bad][0].item(), want[bad][0].item())


def raw_cast(hip, src, dtype):
    """eve_cast itself (HipKernels.cast returns its argument for equal dtypes)."""
    dst = torch.full(src.shape, float('nan'), dtype=dtype, device=src.device)
    hip._ck(hip.lib.eve_cast(dt_code(src.dtype), dt_code(dtype), src.numel(), hip._p(src), hip._p(dst), hip._stream()))
    return dst


CAST_PAIRS = [(torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32), (torch.float32, torch.float16),
              (torch.float16, torch.float32), (torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16),
              (torch.float16, torch.float16)]


@pytest.mark.parametrize('pair', CAST_PAIRS, ids=lambda p: '%s-%s' % (str(p[0])[6:], str(p[1])[6:]))
def test_cast_is_bit_equal_to_tensor_to(hip, pair):
    s, d = pair
    for n in (1, 7, 8 * 1000 + 3, 2048 * 256 + 37):
        src = rnd((n,), torch.float32, 5000 + n, scale=30.0).to(s)
        assert_same_numbers(raw_cast(hip, dev(src), d), src.to(d), 'cast n=%d' % n)
    src = specials().to(s)                             # (for a 16-bit source: that format's own roundings of the list)
    assert_same_numbers(raw_cast(hip, dev(src), d), src.to(d), 'cast specials')
    assert_same_numbers(hip.cast(dev(src), d), src.to(d), 'HipKernels.cast specials')


def test_cast_special_values_land_where_the_formats_say(hip):
    f = lambda v, d: raw_cast(hip, dev(torch.tensor(v, dtype=torch.float32)), d).cpu().float().tolist()   # noqa: E731
    inf = float('inf')
    assert f([65504.0, 65519.0, 65520.0, 1e5, -65520.0], torch.float16) == [65504.0, 65504.0, inf, inf, -inf]
    assert f([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11], torch.float16) == [1.0, 1 + 2.0 ** -9]          # ties to even
    assert f([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8], torch.bfloat16) == [1.0, 1 + 2.0 ** -6]
    assert f([2.0 ** -126, 2.0 ** -133, 1e-40], torch.bfloat16) == [2.0 ** -126, 2.0 ** -133, float(torch.tensor(1e-40).bfloat16())]
    z = raw_cast(hip, dev(torch.tensor([0.0, -0.0])), torch.bfloat16)
    assert bits(z).tolist() == [0, -32768]


def nhwc_from_nchw(src, dtype, cpad):
    N, C, H, W = src.shape
    want = torch.zeros((N, H, W, cpad), dtype=dtype)
    want[..., :C] = src.permute(0, 2, 3, 1).to(dtype)
    return want


@BY_DTYPE
@pytest.mark.parametrize('C', [1, 3, 5, 8, 13])
def test_layout_kernels_are_copies(hip, dtype, C):
    vec = R.vec_of(dtype)
    least = (C + vec - 1) // vec * vec
    for cpad in (least, least + 2 * vec):
        for (H, W) in ((1, 1), (15, 17), (1, 257)):
            src = rnd((2, C, H, W), torch.float32, 6000 + C + H, scale=4.0)
            out = torch.full((2, H, W, cpad), float('nan'), dtype=dtype, device='cuda')
            got = hip.nchw_to_nhwc(dev(src), dtype, cpad, out=out)
            assert torch.equal(bits(got), bits(nhwc_from_nchw(src, dtype, cpad))), 'nchw->nhwc C%d Cpad%d %dx%d' % (C, cpad, H, W)
            assert not bool(bits(got)[..., C:].any()), 'padding channels are +0'
            if cpad > C:
                back = rnd((2, H, W, cpad), dtype, 6100 + C + H)
                got = hip.nhwc_to_nchw(dev(back), C)
                assert torch.equal(bits(got), bits(back[..., :C].permute(0, 3, 1, 2).float())), 'nhwc->nchw'


@BY_DTYPE
def test_layout_kernels_beyond_the_grid_cap(hip, dtype):
    vec = R.vec_of(dtype)
    N, C, H, W = 3, 3, 420, 420
    assert N * H * W * vec // vec > 2048 * 256 and N * C * H * W > 2048 * 256
    src = rnd((N, C, H, W), torch.float32, 6200)
    got = hip.nchw_to_nhwc(dev(src), dtype, vec, out=torch.full((N, H, W, vec), float('nan'), dtype=dtype, device='cuda'))
    want = nhwc_from_nchw(src, dtype, vec)
    assert torch.equal(bits(got), bits(want))
    assert torch.equal(bits(hip.nhwc_to_nchw(got, C)), bits(want[..., :C].permute(0, 3, 1, 2).float()))


@BY_DTYPE
def test_nchw_to_nhwc_rounds_special_values_as_tensor_to(hip, dtype):
    v = specials()
    src = v.view(1, 1, 1, -1)
    got = hip.nchw_to_nhwc(dev(src), dtype, R.vec_of(dtype))
    assert_same_numbers(got[..., 0].reshape(-1), v.to(dtype), 'nchw->nhwc specials')
    assert not bool(bits(got)[..., 1:].any())
    # and back: widening is exact
    assert_same_numbers(hip.nhwc_to_nchw(got, 1).reshape(-1), v.to(dtype).float(), 'nhwc->nchw specials')


# ------------------------------------------------------------------------------------------------ argument checks
def rejected(hip, message, out, call):
    """The C entry point returns an error that _ck raises with the entry point's own message, and writes nothing."""
    out.fill_(0)
    out.view(torch.uint8).fill_(SENTINEL)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError) as e:
        hip._ck(call())
    assert message in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert bool((out.view(torch.uint8) == SENTINEL).all()), '%s: the output was written' % message


@BY_DTYPE
def test_entry_points_reject_bad_arguments_before_any_launch(hip, dtype):
    L, p, st, dt = hip.lib, hip._p, hip._stream(), dt_code(dtype)
    vec = R.vec_of(dtype)
    bad_c = vec + 1
    a = torch.zeros(4096, dtype=torch.float32, device='cuda')          # valid, generously sized device buffers
    out = torch.zeros(4096, dtype=torch.float32, device='cuda')
    i8 = torch.zeros(4096, dtype=torch.uint8, device='cuda')
    i32 = torch.zeros(4096, dtype=torch.int32, device='cuda')
    # C = vec + 1 in every group
    rejected(hip, 'maxpool_fwd: bad dtype / C', out, lambda: L.eve_maxpool3x3s2_fwd(dt, 1, 4, 4, bad_c, p(a), p(out), p(i8), st))
    rejected(hip, 'maxpool_bwd: bad dtype / C', out, lambda: L.eve_maxpool3x3s2_bwd(dt, 1, 4, 4, bad_c, p(a), p(i8), p(out), st))
    rejected(hip, 'avgpool_fwd: bad dtype / C', out, lambda: L.eve_avgpool_fwd(dt, 1, 4, bad_c, p(a), p(out), st))
    rejected(hip, 'avgpool_bwd: bad dtype / C', out, lambda: L.eve_avgpool_bwd(dt, 1, 4, bad_c, p(a), p(out), st))
    rejected(hip, 'avgpool_fwd_f32: bad dtype / C', out, lambda: L.eve_avgpool_fwd_f32(dt, 1, 4, bad_c, p(a), p(out), st))
    rejected(hip, 'avgpool_bwd_f32: bad dtype / C', out, lambda: L.eve_avgpool_bwd_f32(dt, 1, 4, bad_c, p(a), p(out), st))
    rejected(hip, 'adaptive_maxpool_fwd: bad dtype / C', out,
             lambda: L.eve_adaptive_maxpool_fwd(dt, 1, 4, 4, 2, 2, bad_c, p(a), p(out), p(i32), st))
    rejected(hip, 'adaptive_maxpool_bwd: bad dtype / C', out,
             lambda: L.eve_adaptive_maxpool_bwd(dt, 1, 4, 4, 2, 2, bad_c, p(a), p(i32), None, p(out), st))
    rejected(hip, 'bilinear_fwd: bad dtype / C', out, lambda: L.eve_bilinear_fwd(dt, 1, 4, 4, 2, 2, bad_c, p(a), p(out), st))
    rejected(hip, 'bilinear_bwd: bad dtype / C', out, lambda: L.eve_bilinear_bwd(dt, 1, 4, 4, 2, 2, bad_c, p(a), p(out), st))
    rejected(hip, 'nchw_to_nhwc: bad dtype / Cpad', out, lambda: L.eve_nchw_to_nhwc(dt, 1, 3, 4, 4, bad_c, p(a), p(out), st))
    # a bad dtype code
    rejected(hip, 'maxpool_fwd: bad dtype / C', out, lambda: L.eve_maxpool3x3s2_fwd(7, 1, 4, 4, vec, p(a), p(out), p(i8), st))
    rejected(hip, 'nhwc_to_nchw: bad dtype', out, lambda: L.eve_nhwc_to_nchw(7, 1, 3, 4, 4, vec, p(a), p(out), st))
    # adaptive pooling never upsamples
    for oh, ow in ((5, 2), (2, 5)):
        rejected(hip, 'adaptive_maxpool_fwd: bad arguments', out,
                 lambda: L.eve_adaptive_maxpool_fwd(dt, 1, 4, 4, oh, ow, vec, p(a), p(out), p(i32), st))
        rejected(hip, 'adaptive_maxpool_fwd: bad arguments', i32,
                 lambda: L.eve_adaptive_maxpool_fwd(dt, 1, 4, 4, oh, ow, vec, p(a), p(out), p(i32), st))
        rejected(hip, 'adaptive_maxpool_bwd: bad arguments', out,
                 lambda: L.eve_adaptive_maxpool_bwd(dt, 1, 4, 4, oh, ow, vec, p(a), p(i32), None, p(out), st))
    # more channels than the padded layout holds
    rejected(hip, 'nchw_to_nhwc: bad arguments', out, lambda: L.eve_nchw_to_nhwc(dt, 1, vec + 1, 4, 4, vec, p(a), p(out), st))
    rejected(hip, 'nhwc_to_nchw: bad arguments', out, lambda: L.eve_nhwc_to_nchw(dt, 1, vec + 1, 4, 4, vec, p(a), p(out), st))
    # no direct conversion between the two 16-bit formats; empty and null
    rejected(hip, 'cast: bad dtype', out, lambda: L.eve_cast(dt_code(torch.bfloat16), dt_code(torch.float16), 64, p(a), p(out), st))
    rejected(hip, 'cast: bad dtype', out, lambda: L.eve_cast(dt_code(torch.float16), dt_code(torch.bfloat16), 64, p(a), p(out), st))
    rejected(hip, 'cast: bad arguments', out, lambda: L.eve_cast(dt, dt, 0, p(a), p(out), st))
    rejected(hip, 'bilinear_fwd: bad arguments', out, lambda: L.eve_bilinear_fwd(dt, 1, 4, 4, 0, 2, vec, p(a), p(out), st))
    rejected(hip, 'maxpool_fwd: bad arguments', out, lambda: L.eve_maxpool3x3s2_fwd(dt, 1, 4, 4, vec, None, p(out), p(i8), st))


# ------------------------------------------------------------------------------------------------ fused stem tail
def test_fused_stem_tail_at_an_odd_plane(hip):
    """in_relu_maxpool at 33 x 31 (the per-pixel path of the backward: odd sizes), float32, against the three separate reference
    steps exactly as test_pooling_and_resize compares the 64 x 64 stem (whose comment says why the 16-bit formats are not
    compared: rounding the normalised tensor first creates window ties with an arbitrary arg-max)."""
    ref = FakeKernels()
    dtype = torch.float32
    xs = rnd((2, 33, 31, 64), dtype, 7000) * 1.3 + 0.2
    mr = ref.instnorm_stats(xs)
    yp_w, idx_w = ref.in_relu_maxpool_fwd(xs, mr)
    yp_g, idx_g = hip.in_relu_maxpool_fwd(dev(xs), dev(mr))
    close(yp_g, yp_w, dtype, 'in_relu_maxpool fwd')
    dyp = rnd(tuple(yp_w.shape), dtype, 7001)
    close(hip.in_relu_maxpool_bwd(dev(dyp), yp_g, idx_g, dev(xs), dev(mr)),
          ref.in_relu_maxpool_bwd(dyp, yp_w, idx_w, xs, mr), dtype, 'in_relu_maxpool bwd')
    # the window codes are the plain max-pool's: both take the arg-max on raw values (relu(IN(.)) is monotone)
    assert torch.equal(R.window_code_to_flat(idx_g, (33, 31)), R.maxpool3x3s2(xs)[1])
