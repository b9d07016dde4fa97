"""Float64 restatement of the pooling, resize and average-pool kernels (eve_amd/csrc/pool_resize.hip), written from the
definition of each operation -- no F.max_pool2d / F.adaptive_max_pool2d / F.interpolate: tests/fake_kernels.py states the
contracts through those, this file states them a second time -- plus the error bounds the GPU tests hold the kernels to and
the shape / input lists the host and GPU tests share.  tests/test_pool_resize_host.py pins this file against ATen.

All tensors are NHWC, on the CPU.  Values come back in float64, indices in int64.
"""
import functools
from fractions import Fraction

import numpy as np
import torch

F64 = torch.float64


def vec_of(dtype):
    """Elements of one 16-byte channel vector."""
    return 4 if dtype == torch.float32 else 8


# ------------------------------------------------------------------------------------------------ max-pools
def maxpool3x3s2(x):
    """3x3 / stride 2 / pad 1.  -> (y [N, OH, OW, C] float64, idx int64: flat ih * IW + iw of the FIRST maximum in row-major
    window order).  Taps outside the image are absent (not zero, not -inf: a window of -inf picks its first real tap); a NaN
    in the window wins (the first one)."""
    x = x.to(F64)
    N, IH, IW, C = x.shape
    OH, OW = (IH - 1) // 2 + 1, (IW - 1) // 2 + 1
    best = torch.zeros((N, OH, OW, C), dtype=F64)
    bidx = torch.full((N, OH, OW, C), -1, dtype=torch.int64)
    have = torch.zeros((1, OH, OW, 1), dtype=torch.bool)
    for kh in range(3):
        ih = torch.arange(OH) * 2 - 1 + kh
        for kw in range(3):
            iw = torch.arange(OW) * 2 - 1 + kw
            valid = ((ih >= 0) & (ih < IH))[:, None] & ((iw >= 0) & (iw < IW))[None, :]
            v = x[:, ih.clamp(0, IH - 1)][:, :, iw.clamp(0, IW - 1)]
            flat = (ih[:, None] * IW + iw[None, :])[None, :, :, None]
            valid = valid[None, :, :, None]
            take = valid & (~have | (v > best) | (torch.isnan(v) & ~torch.isnan(best)))
            best = torch.where(take, v, best)
            bidx = torch.where(take, flat.expand_as(bidx), bidx)
            have = have | valid
    assert bool(have.all()) and bool((bidx >= 0).all())
    return best, bidx


def _ad_window(o, I, O):
    return (o * I) // O, -((-(o + 1) * I) // O)          # [floor(o I / O), ceil((o + 1) I / O))


def adaptive_maxpool(x, out_hw):
    """Windows [floor(o I / O), ceil((o + 1) I / O)) per axis; the same arg-max rule as maxpool3x3s2."""
    x = x.to(F64).numpy()
    N, IH, IW, C = x.shape
    OH, OW = out_hw
    y = np.empty((N, OH, OW, C), dtype=np.float64)
    idx = np.empty((N, OH, OW, C), dtype=np.int64)
    for oh in range(OH):
        h0, h1 = _ad_window(oh, IH, OH)
        for ow in range(OW):
            w0, w1 = _ad_window(ow, IW, OW)
            win = x[:, h0:h1, w0:w1, :].reshape(N, (h1 - h0) * (w1 - w0), C)
            nan = np.isnan(win)
            k = np.where(nan.any(axis=1), nan.argmax(axis=1), np.where(nan, -np.inf, win).argmax(axis=1))   # first of each
            y[:, oh, ow, :] = np.take_along_axis(win, k[:, None, :], axis=1)[:, 0, :]
            idx[:, oh, ow, :] = (h0 + k // (w1 - w0)) * IW + w0 + k % (w1 - w0)
    return torch.from_numpy(y), torch.from_numpy(idx)


def route(dy, idx, in_hw):
    """The pools' adjoint: dx[n, idx[n, o, c], c] += dy[n, o, c], in float64."""
    N, C = dy.shape[0], dy.shape[-1]
    dx = torch.zeros((N, in_hw[0] * in_hw[1], C), dtype=F64)
    dx.scatter_add_(1, idx.reshape(N, -1, C), dy.to(F64).reshape(N, -1, C))
    return dx.view(N, in_hw[0], in_hw[1], C)


def window_code_to_flat(idx_u8, in_hw):
    """The 3x3/s2 kernel's window code kh * 3 + kw -> flat input index (2 oh - 1 + kh) * IW + (2 ow - 1 + kw)."""
    code = idx_u8.cpu().to(torch.int64)
    N, OH, OW, C = code.shape
    assert bool((code < 9).all()), 'window code outside 0..8'
    ih = (torch.arange(OH) * 2 - 1)[None, :, None, None] + code // 3
    iw = (torch.arange(OW) * 2 - 1)[None, None, :, None] + code % 3
    assert bool(((ih >= 0) & (ih < in_hw[0]) & (iw >= 0) & (iw < in_hw[1])).all()), 'window code points outside the image'
    return ih * in_hw[1] + iw


# ------------------------------------------------------------------------------------------------ bilinear
def _src_coord(o, I, O):
    """max(0, (I / O)(o + 1/2) - 1/2), exactly."""
    return max(Fraction(0), Fraction(I * (2 * o + 1) - O, 2 * O))


@functools.lru_cache(maxsize=None)
def bilinear_matrices(I, O):
    """[O, I] float64 matrix of align_corners=False interpolation along one axis: i0 = floor(s), i1 = min(i0 + 1, I - 1),
    weights 1 - f and f (both on one column where i1 == i0).  Coordinates are formed in rational arithmetic."""
    W = np.zeros((O, I), dtype=np.float64)
    for o in range(O):
        s = _src_coord(o, I, O)
        i0 = min(s.numerator // s.denominator, I - 1)
        i1 = min(i0 + 1, I - 1)
        f = s - i0
        W[o, i0] += float(1 - f)
        W[o, i1] += float(f)
    return torch.from_numpy(W)


def bilinear_fwd(x, out_hw):
    Wy, Wx = bilinear_matrices(x.shape[1], out_hw[0]), bilinear_matrices(x.shape[2], out_hw[1])
    return torch.einsum('oi,nijc,pj->nopc', Wy, x.to(F64), Wx)


def bilinear_bwd(dy, in_hw):
    Wy, Wx = bilinear_matrices(in_hw[0], dy.shape[1]), bilinear_matrices(in_hw[1], dy.shape[2])
    return torch.einsum('oi,nopc,pj->nijc', Wy, dy.to(F64), Wx)


# ------------------------------------------------------------------------------------------------ average pool
def avgpool(x):
    return x.to(F64).sum(dim=(1, 2)) / (x.shape[1] * x.shape[2])


def avgpool_adjoint(dy, hw):
    N, C = dy.shape
    return (dy.to(F64) / (hw[0] * hw[1]))[:, None, None, :].expand(N, hw[0], hw[1], C).contiguous()


# ------------------------------------------------------------------------------------------------ bounds
# u: the store's relative rounding error, the format's unit round-off 2^-p for p significand bits (round to nearest: half the
# spacing 2^(1-p) at the bottom of a binade; bfloat16 has p = 8, float16 p = 11; 0 where a float32 result is stored as it is).
# TINY: half the spacing of the format's subnormals, the store's absolute error where u * |v| is below it (only float16's is
# within reach of float32 data).
EPS32 = 2.0 ** -24
U = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
TINY = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}


def store_bound(exact, e32, dtype):
    """A float32 value v with |v - exact| <= e32, rounded once to `dtype`: |stored - exact| <= e32 + max(u |v|, tiny)
    <= e32 (1 + u) + max(u |exact|, tiny)."""
    u = U[dtype]
    if u == 0.0:
        return e32
    return e32 * (1.0 + u) + torch.clamp(u * exact.abs(), min=TINY[dtype])


def sum_bound(k, mag, exact, dtype, extra=0):
    """k float32 terms summed in any order (k - 1 additions, each off by at most 2^-24 of a partial sum that the sum of
    magnitudes `mag` bounds), `extra` further float32 roundings of a value no larger than `mag`, one store:
    (k - 1 + extra) 2^-24 mag + u |exact|.  k may be a tensor (per entry)."""
    k = torch.as_tensor(k, dtype=F64)
    return store_bound(exact, (torch.clamp(k - 1, min=0) + extra) * EPS32 * mag, dtype)


def pool_bwd_bound(dy, idx, in_hw, dtype):
    """Routing random gradients: an input pixel sums its k routed terms in float32, then one store."""
    k = route(torch.ones_like(dy, dtype=F64), idx, in_hw)
    return sum_bound(k, route(dy.to(F64).abs(), idx, in_hw), route(dy, idx, in_hw), dtype)


def avgpool_fwd_bound(x, dtype):
    """HW terms summed in float32, one float32 division (one more rounding of a quotient no larger than mean |x|)."""
    HW = x.shape[1] * x.shape[2]
    return sum_bound(HW, x.to(F64).abs().sum(dim=(1, 2)) / HW, avgpool(x), dtype, extra=1)


def avgpool_bwd_bound(dy, hw, dtype):
    exact = avgpool_adjoint(dy, hw)
    return sum_bound(1, exact.abs(), exact, dtype, extra=1)


def coord_slack(I):
    """The kernels form a source coordinate with three float32 operations (I / O, times o + 1/2, minus 1/2) on magnitudes up
    to I: |computed s - s| <= 3 * 2^-24 * max(I, 1)."""
    return 3.0 * EPS32 * max(I, 1)


@functools.lru_cache(maxsize=None)
def bilinear_support(I, O):
    """[O, I] bool: the input pixels output o can draw on when its coordinate is off by up to coord_slack(I): |s - i| < 1 +
    slack.  Interpolation is continuous in s (pixel i's weight is the hat function max(0, 1 - |s - i|), clamped at the
    edges, 1-Lipschitz), so a floor that lands on the other side of an integer moves at most `slack` of weight -- but it moves
    it onto the neighbouring pixel, which therefore belongs to the taps: three per axis where s is an integer, else two."""
    d = Fraction(coord_slack(I))
    S = np.zeros((O, I), dtype=bool)
    for o in range(O):
        s = _src_coord(o, I, O)
        for i in range(I):
            S[o, i] = abs(s - i) < 1 + d
    return torch.from_numpy(S)


def _neighbourhood_max(ax, Sy, Sx):
    rows = torch.stack([ax[:, Sy[o]].amax(dim=1) for o in range(Sy.shape[0])], dim=1)           # [N, OH, IW, C]
    return torch.stack([rows[:, :, Sx[p]].amax(dim=2) for p in range(Sx.shape[0])], dim=2)      # [N, OH, OW, C]


def bilinear_fwd_bound(x, out_hw, dtype):
    """|kernel - Wy x Wx^T|.  With w' the weights at the computed coordinates, w' w' - w w = (wy' - wy) wx + wy' (wx' - wx) and
    sum_i |w'_i - w_i| <= 2 |ds| per axis, so the coordinates cost at most 2 (|ds_y| + |ds_x|) max |x| over the taps; the
    float32 evaluation costs 6 * 2^-24 * sum w |x| (a tap passes 1 - f, a product and a sum in its row expression, a product
    and a sum in the outer one, and the other axis' 1 - f); then the store."""
    IH, IW = x.shape[1], x.shape[2]
    ax = x.to(F64).abs()
    Wy, Wx = bilinear_matrices(IH, out_hw[0]), bilinear_matrices(IW, out_hw[1])
    tapmax = _neighbourhood_max(ax, bilinear_support(IH, out_hw[0]), bilinear_support(IW, out_hw[1]))
    mag = torch.einsum('oi,nijc,pj->nopc', Wy, ax, Wx)
    e32 = 2.0 * (coord_slack(IH) + coord_slack(IW)) * tapmax + 6.0 * EPS32 * mag
    return store_bound(bilinear_fwd(x, out_hw), e32, dtype)


def bilinear_bwd_bound(dy, in_hw, dtype):
    """The same over the output pixels that reach an input pixel: |w' w' - w w| <= ds_y S_y w_x + (w_y + ds_y S_y) ds_x S_x per
    (output, input) pair (S: bilinear_support); each of the k = |S_y column| * |S_x column| terms passes 1 - f twice, two
    products and the k - 1 additions: (k + 5) * 2^-24 * |Wy|^T |dy| |Wx|; then the store."""
    IH, IW = in_hw
    OH, OW = dy.shape[1], dy.shape[2]
    ady = dy.to(F64).abs()
    Wy, Wx = bilinear_matrices(IH, OH), bilinear_matrices(IW, OW)
    Sy, Sx = bilinear_support(IH, OH).to(F64), bilinear_support(IW, OW).to(F64)
    dsy, dsx = coord_slack(IH), coord_slack(IW)

    def both(A, B):
        return torch.einsum('oi,nopc,pj->nijc', A, ady, B)
    coord = dsy * both(Sy, Wx) + dsx * both(Wy, Sx) + dsy * dsx * both(Sy, Sx)
    k = Sy.sum(dim=0)[:, None] * Sx.sum(dim=0)[None, :]
    e32 = coord + (k[None, :, :, None] + 5.0) * EPS32 * both(Wy, Wx)
    return store_bound(bilinear_bwd(dy, in_hw), e32, dtype)


def ratio(err, bound):
    """max err / bound over the entries with an error (an entry with bound 0 must be exact: ratio inf otherwise)."""
    err, bound = err.to(F64), torch.as_tensor(bound, dtype=F64).expand_as(err)
    r = torch.where(err > 0, err / bound, torch.zeros_like(err))
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------------------ cases
def maxpool_shapes(vec):
    """(N, IH, IW, C): smallest; one window per axis plus edge; odd non-square; odd width, several vectors; a wide row."""
    return [(1, 1, 1, vec), (2, 2, 2, vec), (2, 7, 9, vec), (3, 64, 33, 2 * vec), (1, 5, 300, vec)]


def maxpool_cap_shape(vec):
    """N OH OW C / vec > 2048 * 256: the grid-stride loop takes a second turn."""
    return (17, 128, 128, 64) if vec == 8 else (9, 128, 128, 64)


def adaptive_shapes(vec):
    """(N, IH, IW, OH, OW, C): non-divisible; overlapping; large windows; identity; global; rows over 256 items."""
    return [(2, 7, 11, 3, 4, vec), (2, 9, 16, 5, 8, 2 * vec), (1, 72, 128, 5, 8, vec), (2, 6, 10, 6, 10, vec),
            (2, 6, 10, 1, 1, vec), (1, 4, 300, 2, 150, vec)]


def adaptive_cap_shape(vec):
    """N OH > 8192 rows (and N IH in the backward): the row loop takes a second turn."""
    return (230, 72, 16, 36, 8, vec)


def bilinear_shapes(vec):
    """(N, IH, IW, OH, OW, C)."""
    pairs = [((5, 8), (9, 16)), ((9, 16), (5, 8)), ((9, 16), (72, 128)), ((72, 128), (9, 16)), ((3, 5), (64, 40)),
             ((64, 40), (3, 5)), ((1, 7), (6, 7)), ((6, 7), (1, 1)), ((6, 10), (6, 10)), ((4, 300), (8, 600))]
    return [(2, i[0], i[1], o[0], o[1], vec) for i, o in pairs] + [(2, 5, 8, 9, 16, 4 * vec)]


def bilinear_cap_shape(vec):
    """N OH > 8192 rows in the forward, N IH > 8192 in the backward."""
    return (2060, 4, 5, 8, 10, vec)


INPUT_KINDS = ['random', 'negative', 'levels', 'constant', 'inf']


def make_input(kind, shape, dtype, seed):
    """random | negative: in [-9, -1], zero padding would win every border window | levels: 4 values, most windows tie |
    constant | inf: +-inf sprinkled in."""
    g = torch.Generator().manual_seed(seed)
    if kind == 'random':
        x = torch.randn(shape, generator=g)
    elif kind == 'negative':
        x = -1.0 - 8.0 * torch.rand(shape, generator=g)
    elif kind == 'levels':
        x = torch.randint(0, 4, shape, generator=g).float() - 1.5
    elif kind == 'constant':
        x = torch.full(shape, -2.5)
    elif kind == 'inf':
        x = torch.randn(shape, generator=g)
        r = torch.rand(shape, generator=g)
        x = torch.where(r < 0.1, torch.full_like(x, float('inf')), x)
        x = torch.where(r > 0.85, torch.full_like(x, float('-inf')), x)
    else:
        raise ValueError(kind)
    return x.to(dtype)


def integer_grad(shape, dtype, seed):
    """Integer-valued, |v| <= 8: sums of up to four are exact in all three formats."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, shape, generator=g).to(dtype)
