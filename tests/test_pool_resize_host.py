"""CPU: pins tests/pool_resize_ref.py -- the float64 reference and the error bounds that tests/test_gpu_pool_resize_exact.py holds
the pooling / resize kernels to -- against ATen in float64, at every shape the GPU tests use.  A wrong helper could otherwise
not be told from a wrong kernel."""
import pytest
import torch
import torch.nn.functional as F

import pool_resize_ref as R

F64 = torch.float64
VECS = pytest.mark.parametrize('vec', [4, 8], ids=['vec4', 'vec8'])


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def ident(s):
    return 'x'.join(map(str, s))


# ------------------------------------------------------------------------------------------------ pools against ATen
def check_maxpool(shape, kind, seed):
    x = R.make_input(kind, shape, F64, seed)
    y, idx = R.maxpool3x3s2(x)
    y_w, idx_w = F.max_pool2d(nchw(x), 3, 2, 1, return_indices=True)
    assert torch.equal(y, nhwc(y_w)), 'values'
    assert torch.equal(idx, nhwc(idx_w)), 'arg-max (first maximum in row-major window order)'
    # the kernel's window code names the same pixel
    oh = torch.arange(y.shape[1])[None, :, None, None]
    ow = torch.arange(y.shape[2])[None, None, :, None]
    code = (idx // shape[2] - (2 * oh - 1)) * 3 + (idx % shape[2] - (2 * ow - 1))
    assert bool(((code >= 0) & (code < 9)).all())
    assert torch.equal(R.window_code_to_flat(code.to(torch.uint8), shape[1:3]), idx)
    # the adjoint against autograd
    xa = nchw(x).requires_grad_(True)
    dy = R.integer_grad(tuple(y.shape), F64, seed + 1)
    dx_w, = torch.autograd.grad(F.max_pool2d(xa, 3, 2, 1), xa, nchw(dy))
    assert torch.equal(R.route(dy, idx, shape[1:3]), nhwc(dx_w)), 'route'


@VECS
@pytest.mark.parametrize('kind', R.INPUT_KINDS)
def test_maxpool_reference_is_aten_in_float64(vec, kind):
    for i, shape in enumerate(R.maxpool_shapes(vec)):
        check_maxpool(shape, kind, 100 + i)


@VECS
def test_maxpool_reference_is_aten_at_the_grid_cap_shape(vec):
    check_maxpool(R.maxpool_cap_shape(vec), 'levels', 110)


def check_adaptive(shape, kind, seed):
    N, IH, IW, OH, OW, C = shape
    x = R.make_input(kind, (N, IH, IW, C), F64, seed)
    y, idx = R.adaptive_maxpool(x, (OH, OW))
    y_w, idx_w = F.adaptive_max_pool2d(nchw(x), (OH, OW), return_indices=True)
    assert torch.equal(y, nhwc(y_w)), 'values'
    assert torch.equal(idx, nhwc(idx_w)), 'arg-max'
    xa = nchw(x).requires_grad_(True)
    dy = R.integer_grad(tuple(y.shape), F64, seed + 1)
    dx_w, = torch.autograd.grad(F.adaptive_max_pool2d(xa, (OH, OW)), xa, nchw(dy))
    assert torch.equal(R.route(dy, idx, (IH, IW)), nhwc(dx_w)), 'route'


@VECS
@pytest.mark.parametrize('kind', R.INPUT_KINDS)
def test_adaptive_maxpool_reference_is_aten_in_float64(vec, kind):
    for i, shape in enumerate(R.adaptive_shapes(vec)):
        check_adaptive(shape, kind, 200 + i)


def test_adaptive_maxpool_reference_is_aten_at_the_row_cap_shape():
    check_adaptive(R.adaptive_cap_shape(8), 'levels', 210)


def test_a_nan_in_the_window_wins_and_absent_taps_are_not_zero():
    x = torch.full((1, 3, 3, 1), -5.0, dtype=F64)
    y, idx = R.maxpool3x3s2(x)
    assert torch.equal(y, torch.full((1, 2, 2, 1), -5.0, dtype=F64)) and idx.flatten().tolist() == [0, 1, 3, 4]
    x[0, 1, 1, 0] = float('nan')
    x[0, 2, 2, 0] = 7.0
    y, idx = R.maxpool3x3s2(x)
    assert bool(torch.isnan(y).all()) and idx.flatten().tolist() == [4, 4, 4, 4]
    ya, ia = R.adaptive_maxpool(x, (2, 2))            # windows [0, 2) and [1, 3) per axis: all four hold the centre
    assert bool(torch.isnan(ya).all()) and ia.flatten().tolist() == [4, 4, 4, 4]
    x = torch.full((1, 2, 2, 1), float('-inf'), dtype=F64)
    assert R.maxpool3x3s2(x)[1].flatten().tolist() == [0] and R.adaptive_maxpool(x, (1, 1))[1].flatten().tolist() == [0]


# ------------------------------------------------------------------------------------------------ bilinear against ATen
def bilinear_cases():
    return R.bilinear_shapes(4) + R.bilinear_shapes(8)[-1:] + [(3,) + R.bilinear_cap_shape(4)[1:]]


@pytest.mark.parametrize('shape', bilinear_cases(), ids=ident)
def test_bilinear_reference_is_aten_in_float64(shape):
    N, IH, IW, OH, OW, C = shape
    g = torch.Generator().manual_seed(300)
    x = torch.randn((N, IH, IW, C), generator=g, dtype=F64)
    dy = torch.randn((N, OH, OW, C), generator=g, dtype=F64)
    xa = nchw(x).requires_grad_(True)
    y_w = F.interpolate(xa, size=(OH, OW), mode='bilinear', align_corners=False)
    dx_w, = torch.autograd.grad(y_w, xa, nchw(dy))
    y, dx = R.bilinear_fwd(x, (OH, OW)), R.bilinear_bwd(dy, (IH, IW))
    # both sides are float64 evaluations of the same four-tap sums: a few float64 roundings of the magnitude sums apart
    # (ATen forms its coordinates in floating point; where one lands beside an integer the continuity argument of
    # bilinear_support applies with a float64 slack)
    tol_y = 64 * 2.0 ** -53 * max(IH, IW) * float(x.abs().max())
    assert float((y - nhwc(y_w.detach())).abs().max()) <= tol_y
    tol_dx = 64 * 2.0 ** -53 * max(IH, IW) * float(R.bilinear_bwd(dy.abs(), (IH, IW)).max())
    assert float((dx - nhwc(dx_w)).abs().max()) <= tol_dx
    for I, O in ((IH, OH), (IW, OW)):
        W = R.bilinear_matrices(I, O)
        assert float((W.sum(dim=1) - 1).abs().max()) <= 2.0 ** -52 and bool((W >= 0).all())
        assert int((W > 0).sum(dim=1).max()) <= 2


def test_bilinear_matrix_by_hand():
    W = R.bilinear_matrices(2, 4)                      # s = max(0, o / 2 - 1 / 4): 0, 1/4, 3/4, 5/4 -> clamps at both ends
    assert torch.equal(W, torch.tensor([[1, 0], [0.75, 0.25], [0.25, 0.75], [0, 1]], dtype=F64))
    assert torch.equal(R.bilinear_matrices(1, 3), torch.ones((3, 1), dtype=F64))
    assert torch.equal(R.bilinear_matrices(5, 5), torch.eye(5, dtype=F64))
    # 5 -> 9: output 4 sits exactly on pixel 2; a coordinate a hair below it draws on pixel 1 as well: three taps, else two
    S = R.bilinear_support(5, 9)
    assert S[4].tolist() == [False, True, True, True, False] and S[3].tolist() == [False, True, True, False, False]
    assert S[0].tolist() == [True, True, False, False, False]          # s = 0 exactly (clamped): pixel 1 at distance 1 + slack
    assert bool((S.to(F64) >= (R.bilinear_matrices(5, 9) > 0).to(F64)).all())


def test_avgpool_reference():
    g = torch.Generator().manual_seed(5)
    x = torch.randn((3, 3, 5, 8), generator=g, dtype=F64)
    assert float((R.avgpool(x) - x.mean(dim=(1, 2))).abs().max()) <= 2.0 ** -50
    dy = torch.randn((3, 8), generator=g, dtype=F64)
    xa = x.clone().requires_grad_(True)
    dx_w, = torch.autograd.grad(xa.mean(dim=(1, 2)), xa, dy)
    assert float((R.avgpool_adjoint(dy, (3, 5)) - dx_w).abs().max()) <= 2.0 ** -50


# ------------------------------------------------------------------------------------------------ the bounds
@pytest.mark.parametrize('shape', bilinear_cases(), ids=ident)
def test_a_float32_evaluation_of_the_matrices_stays_inside_the_bilinear_bounds(shape):
    """The derivation's own check: the reference's matrices cast to float32 and applied in float32 make fewer roundings than the
    bound allows for (no coordinate error at all), so they must sit inside it -- for float32 outputs and, rounded once more,
    for the 16-bit formats."""
    N, IH, IW, OH, OW, C = shape
    g = torch.Generator().manual_seed(400)
    x = torch.randn((N, IH, IW, C), generator=g)
    dy = torch.randn((N, OH, OW, C), generator=g)
    Wy, Wx = R.bilinear_matrices(IH, OH).float(), R.bilinear_matrices(IW, OW).float()
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        xd, dyd = x.to(dtype), dy.to(dtype)
        y32 = torch.einsum('oi,nipc->nopc', Wy, torch.einsum('nijc,pj->nipc', xd.float(), Wx))
        dx32 = torch.einsum('oi,nojc->nijc', Wy, torch.einsum('nopc,pj->nojc', dyd.float(), Wx))
        r_f = R.ratio((y32.to(dtype).to(F64) - R.bilinear_fwd(xd, (OH, OW))).abs(), R.bilinear_fwd_bound(xd, (OH, OW), dtype))
        r_b = R.ratio((dx32.to(dtype).to(F64) - R.bilinear_bwd(dyd, (IH, IW))).abs(), R.bilinear_bwd_bound(dyd, (IH, IW), dtype))
        print('float32 matrices %s %-14s fwd err/bound %.4f  bwd err/bound %.4f' % (ident(shape), dtype, r_f, r_b))
        assert r_f <= 1.0 and r_b <= 1.0


def test_bilinear_bound_covers_a_coordinate_that_lands_beside_an_integer():
    """5 -> 9, output 4: s = 2 exactly.  Computed a float32 hair below, it reads pixel 1 with weight ~1e-7 instead of pixel 3
    with weight 0: the bound must hold with a large value on pixel 1 and nothing on pixels 2 and 3."""
    x = torch.zeros((1, 5, 1, 4), dtype=F64)
    x[0, 1] = 1000.0
    d = R.coord_slack(5)
    W = R.bilinear_matrices(5, 9).clone()
    W[4] = torch.tensor([0, d, 1 - d, 0, 0], dtype=F64)                # the weights at s = 2 - d
    err = (torch.einsum('oi,nijc->nojc', W, x) - R.bilinear_fwd(x, (9, 1))).abs()
    bound = R.bilinear_fwd_bound(x, (9, 1), torch.float32)
    assert float(err[0, 4].max()) > 0 and bool((err <= bound).all())
    dy = torch.zeros((1, 9, 1, 4), dtype=F64)
    dy[0, 4] = 1000.0
    errb = (torch.einsum('oi,nojc->nijc', W, dy) - R.bilinear_bwd(dy, (5, 1))).abs()
    assert float(errb[0, 1].max()) > 0 and bool((errb <= R.bilinear_bwd_bound(dy, (5, 1), torch.float32)).all())


@pytest.mark.parametrize('k', [1, 2, 4, 15, 49, 256])
def test_sum_bound_holds_for_float32_sums_in_either_order(k):
    g = torch.Generator().manual_seed(500 + k)
    t = torch.randn((4096, k), generator=g) * torch.rand((4096, 1), generator=g) * 50
    exact, mag = t.to(F64).sum(dim=1), t.to(F64).abs().sum(dim=1)
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        for order in (t, t.flip(1)):
            acc = torch.zeros(4096)
            for j in range(k):
                acc = acc + order[:, j]
            r = R.ratio((acc.to(dtype).to(F64) - exact).abs(), R.sum_bound(k, mag, exact, dtype))
            assert r <= 1.0, (k, dtype, r)
    if k == 1:                                           # one float32 term into float32: nothing may differ
        assert float(R.sum_bound(1, mag, exact, torch.float32).max()) == 0.0


def test_store_bound_is_half_the_spacing_of_the_format():
    g = torch.Generator().manual_seed(6)
    v = torch.cat([torch.randn(20000, generator=g) * 10, torch.randn(20000, generator=g) * 1e-5, torch.randn(2000, generator=g) * 1e-8])
    for dtype in (torch.bfloat16, torch.float16):
        err = (v.to(dtype).to(F64) - v.to(F64)).abs()
        assert R.ratio(err, R.store_bound(v.to(F64), 0.0, dtype)) <= 1.0
        # ... and is reached: a tie just above 1 is off by u, against a bound of u (1 + u)
        tie = torch.tensor([1.0 + R.U[dtype]], dtype=F64)
        assert float((tie.float().to(dtype).to(F64) - tie).abs()) == R.U[dtype]
        assert float(R.store_bound(tie, 0.0, dtype)) == R.U[dtype] * (1.0 + R.U[dtype])
    assert float(torch.as_tensor(R.store_bound(v.to(F64), 0.0, torch.float32)).abs().max()) == 0.0
    # float16 subnormals: the relative term alone would not cover them
    small = torch.tensor([3.0 * 2.0 ** -25], dtype=F64)
    assert float((small.float().to(torch.float16).to(F64) - small).abs()) > R.U[torch.float16] * float(small)


def test_pool_and_avgpool_bounds():
    dtype = torch.bfloat16
    x = R.make_input('levels', (2, 7, 9, 8), dtype, 7)
    _, idx = R.maxpool3x3s2(x)
    dy = R.make_input('random', tuple(idx.shape), dtype, 8)
    b = R.pool_bwd_bound(dy, idx, (7, 9), dtype)
    k = R.route(torch.ones(idx.shape, dtype=F64), idx, (7, 9))
    assert int(k.max()) <= 4 and int(k.sum()) == idx.numel()
    assert bool((b[k == 0] == R.TINY[dtype]).all())                    # nothing routed: the store of 0 only
    one = k == 1                                                       # one term: its own store
    assert torch.equal(b[one], torch.clamp(R.U[dtype] * R.route(dy, idx, (7, 9))[one].abs(), min=R.TINY[dtype]))
    # average pool: a float32 evaluation in the kernel's order stays inside
    xa = R.make_input('random', (3, 7, 7, 8), torch.float32, 9)
    acc = torch.zeros((3, 8))
    for p in range(49):
        acc = acc + xa.reshape(3, 49, 8)[:, p]
    y32 = acc / 49.0
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        assert R.ratio((y32.to(dt).to(F64) - R.avgpool(xa)).abs(), R.avgpool_fwd_bound(xa, dt)) <= 1.0
        g = (xa[:, 0, 0].to(dt).float() / 49.0).to(dt).to(F64)
        want = R.avgpool_adjoint(xa[:, 0, 0].to(dt), (7, 7))
        assert R.ratio((g[:, None, None, :] - want).abs(), R.avgpool_bwd_bound(xa[:, 0, 0].to(dt), (7, 7), dt)) <= 1.0
