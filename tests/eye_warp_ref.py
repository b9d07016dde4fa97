"""The contract of eve_eye_warp_u8_to_nchw / eve_eye_warp_u8_to_stem (include/eve_hip.h) in numpy, vectorised per patch, the warps
the tests share, and stand-ins of the two HipKernels methods for the torch-CPU FakeKernels.

For output pixel (oy, ox) of patch n, with m = warps[n] (patch pixel -> camera pixel), all in float64:
    X = (m00*ox + m01*oy) + m02,  Y = (m10*ox + m11*oy) + m12,  Wd = (m20*ox + m21*oy) + m22,  u = X / Wd,  v = Y / Wd
    inside iff Wd > 0 and u > -1 and u < IW and v > -1 and v < IH            (a NaN fails its comparison)
    fu = floor(u*256 + 0.5), x0 = fu >> 8, ax = fu & 255 (fv, y0, ay likewise); taps outside the frame read 0
    S = (256-ax)(256-ay) p00 + ax(256-ay) p01 + (256-ax)ay p10 + ax ay p11;  S = 0 outside
    value = float32(S) * 2^-16 * float32(2/255) + float32(-1), each step rounded to float32
numpy evaluates every ufunc on its own, so no product and sum are contracted here."""
import math

import numpy as np
import torch

MAX_FRAME, MAX_PATCH = 16384, 4096
EYE_SCALE, EYE_SHIFT = np.float32(2.0 / 255.0), np.float32(-1.0)


def check_shapes(frames_shape, warps_shape, out_hw):
    N, IH, IW, C = frames_shape
    if C not in (3, 4):
        raise ValueError('eye_warp: C must be 3 or 4')
    if N < 1 or not (0 < IH <= MAX_FRAME and 0 < IW <= MAX_FRAME):
        raise ValueError('eye_warp: frame too large or empty')
    if not (0 < out_hw[0] <= MAX_PATCH and 0 < out_hw[1] <= MAX_PATCH):
        raise ValueError('eye_warp: patch too large or empty')
    if tuple(warps_shape) != (N, 3, 3):
        raise ValueError('eye_warp: warps must be [N, 3, 3]')


def warp_sums(frames, warps, out_hw):
    """frames uint8 [N, IH, IW, C], warps float32 [N, 3, 3] -> (S int64 [N, 3, OH, OW], outside bool [N, OH, OW])."""
    frames, warps = np.asarray(frames), np.asarray(warps)
    assert frames.dtype == np.uint8 and warps.dtype == np.float32
    check_shapes(frames.shape, warps.shape, out_hw)
    N, IH, IW, C = frames.shape
    OH, OW = out_hw
    ox = np.arange(OW, dtype=np.float64)[None, :]
    oy = np.arange(OH, dtype=np.float64)[:, None]
    S = np.zeros((N, 3, OH, OW), dtype=np.int64)
    outside = np.zeros((N, OH, OW), dtype=bool)
    for n in range(N):
        m = warps[n].astype(np.float64)
        with np.errstate(all='ignore'):
            X = (m[0, 0] * ox + m[0, 1] * oy) + m[0, 2]
            Y = (m[1, 0] * ox + m[1, 1] * oy) + m[1, 2]
            Wd = (m[2, 0] * ox + m[2, 1] * oy) + m[2, 2]
            u, v = X / Wd, Y / Wd
            inside = (Wd > 0) & (u > -1) & (u < IW) & (v > -1) & (v < IH)
            fu = np.where(inside, np.floor(u * 256.0 + 0.5), 0.0).astype(np.int64)
            fv = np.where(inside, np.floor(v * 256.0 + 0.5), 0.0).astype(np.int64)
        x0, ax, y0, ay = fu >> 8, fu & 255, fv >> 8, fv & 255
        # x0 in [-1, IW], so x0 + 1 reaches IW + 1: one zero row / column before the frame, two behind it
        padded = np.zeros((IH + 3, IW + 3, 3), dtype=np.int64)
        padded[1:IH + 1, 1:IW + 1] = frames[n, :, :, :3]
        p = lambda dy, dx: padded[y0 + 1 + dy, x0 + 1 + dx]                   # [OH, OW, 3]
        w = lambda a: a[..., None]
        s = (w((256 - ax) * (256 - ay)) * p(0, 0) + w(ax * (256 - ay)) * p(0, 1) +
             w((256 - ax) * ay) * p(1, 0) + w(ax * ay) * p(1, 1))
        s = np.where(inside[..., None], s, 0)
        S[n] = s.transpose(2, 0, 1)
        outside[n] = ~inside
    assert S.min() >= 0 and S.max() <= 255 * 65536
    return S, outside


def values_of_sums(S):
    val = S.astype(np.float32) * np.float32(2.0 ** -16)       # exact: S < 2^24
    return val * EYE_SCALE + EYE_SHIFT


def eye_warp(frames, warps, out_hw):
    """-> (float32 [N, 3, OH, OW], outside bool [N, OH, OW])"""
    S, outside = warp_sums(frames, warps, out_hw)
    return values_of_sums(S), outside


def pack_stem(values, dtype):
    """float32 [N, 3, OH, OW] (numpy or torch) -> the stem's packed [N, OH+6, OW+8, 4] of `dtype` (round to nearest even), the pixel
    at (y+3, x+4), ring and fourth channel zero."""
    v = torch.as_tensor(values)
    N, C, OH, OW = v.shape
    out = torch.zeros((N, OH + 6, OW + 8, 4), dtype=dtype)
    out[:, 3:OH + 3, 4:OW + 4, :C] = v.permute(0, 2, 3, 1).to(dtype)
    return out


# ------------------------------------------------------------------------------------------------ the warps the tests share
def shift(tx, ty):
    """patch (x, y) -> camera (x + tx, y + ty)"""
    return np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], dtype=np.float32)


def similarity(scale, degrees, tx, ty, persp=(0.0, 0.0)):
    c, s = scale * math.cos(math.radians(degrees)), scale * math.sin(math.radians(degrees))
    return np.array([[c, -s, tx], [s, c, ty], [persp[0], persp[1], 1]], dtype=np.float32)


# name -> (matrix, the share of a 128 x 128 patch over a 160 x 200 frame that falls outside: 'none', 'some' (strictly between 0.2
# and 0.9), 'few' (a sliver: above 0, below 0.05) or 'all')
WARPS = {
    'integer-shift': (shift(37, 21), 'none'),
    'fractional-shift': (shift(0.5, 0.25), 'none'),
    'rotated-perspective': (similarity(1.1, 10.0, 25.0, 3.0, persp=(1e-4, -2e-4)), 'few'),
    'partly-outside': (similarity(1.5, 0.0, -40.25, -30.5), 'some'),
    'negative-denominator': (np.array([[1, 0, 20], [0, 1, 10], [-0.02, 0, 1]], dtype=np.float32), 'some'),
}
NAN_WARP = np.array([[1, 0, 3], [0, np.nan, 2], [0, 0, 1]], dtype=np.float32)
OFF_FRAME_WARP = shift(5000, -7000)


def outside_share_ok(kind, share):
    return {'none': share == 0.0, 'few': 0.0 < share < 0.05, 'some': 0.2 < share < 0.9, 'all': share == 1.0}[kind]


def random_frames(N, IH, IW, C, seed):
    v = np.random.default_rng(seed).integers(0, 256, size=(N, IH, IW, C), dtype=np.uint8)
    if C == 4:
        v[..., 3] = 255                        # the alpha plane: must leave no trace
    return v


def checkerboard_frames(N, IH, IW, C):
    """Pixels alternate 0 / 255 along both axes (frame n starts at phase n): a tap off by one pixel changes every output."""
    y = np.arange(IH)[None, :, None, None]
    x = np.arange(IW)[None, None, :, None]
    n = np.arange(N)[:, None, None, None]
    v = (((y + x + n) % 2) == 0).astype(np.uint8) * 255
    v = np.broadcast_to(v, (N, IH, IW, C)).copy()
    if C == 4:
        v[..., 3] = 255
    return v


# ------------------------------------------------------------------------------------------------ stand-ins for FakeKernels
def eye_warp_u8_to_nchw(self, frames, warps, out_hw):
    """Stand-in of HipKernels.eye_warp_u8_to_nchw: `class Fakes(FakeKernels): eye_warp_u8_to_nchw = eye_warp_ref.eye_warp_u8_to_nchw`."""
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] not in (3, 4):
        raise TypeError('eye_warp: frames must be uint8 [N, IH, IW, 3 | 4]')
    if warps.dtype != torch.float32 or tuple(warps.shape) != (frames.shape[0], 3, 3):
        raise TypeError('eye_warp: warps must be float32 [N, 3, 3]')
    return torch.from_numpy(eye_warp(frames.numpy(), warps.numpy(), (int(out_hw[0]), int(out_hw[1])))[0])


def eye_warp_u8_to_stem(self, frames, warps, out_hw, out=None, dtype=torch.bfloat16):
    return self.stem_pack_input(eye_warp_u8_to_nchw(self, frames, warps, out_hw), out=out, dtype=dtype)
