"""The contract of eve_eye_warp_lens_u8_to_nchw / eve_eye_warp_lens_u8_to_stem (include/eve_hip.h) in numpy, vectorised per patch,
the lenses the tests share, and stand-ins of the two HipKernels methods for the torch-CPU FakeKernels.  The plain contract, its
value and packing code, its warps and its frames are tests/eye_warp_ref.py's, by import.

A lens row is 12 float32, widened to float64: L = (fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6) -- OpenCV's pinhole + radial /
tangential / rational model.  For output pixel (oy, ox) of patch n: X, Y, Wd, u = X / Wd, v = Y / Wd as in eye_warp_ref; (u, v) is a
pixel of the UNDISTORTED image.  Then, every operation rounded on its own in float64 and in exactly this association:
    x  = (u - cx) / fx            y  = (v - cy) / fy
    xx = x*x   yy = y*y   xy = x*y   r2 = xx + yy
    num = ((k3*r2 + k2)*r2 + k1)*r2 + 1.0
    den = ((k6*r2 + k5)*r2 + k4)*r2 + 1.0
    rad = num / den               a = xy + xy
    xd = (x*rad + p1*a) + p2*(r2 + (xx + xx))
    yd = (y*rad + p1*(r2 + (yy + yy))) + p2*a
    ud = fx*xd + cx               vd = fy*yd + cy
    inside iff Wd > 0 and den > 0 and ud > -1 and ud < IW and vd > -1 and vd < IH      (a NaN fails its comparison)
and from (ud, vd) on the plain contract.  A row whose eight coefficients are all +-0 takes the plain coordinate (u, v) for its
patch, whatever its intrinsics.  numpy evaluates every ufunc on its own, so nothing is contracted here."""
import numpy as np
import torch

import eye_warp_ref as ref

# name -> float32 [12]
LENSES = {
    'barrel5': np.array([180, 180, 100, 80, -0.25, 0.08, 1e-3, -5e-4, -0.01, 0, 0, 0], dtype=np.float32),
    'rational8': np.array([180, 182, 101, 79, 0.9, 0.1, 2e-3, 1e-3, 0.01, 1.1, 0.15, 0.02], dtype=np.float32),
    'tangential': np.array([180, 180, 100, 80, 0, 0, 5e-3, -4e-3, 0, 0, 0, 0], dtype=np.float32),
    'pole': np.array([120, 120, 100, 80, 0, 0, 0, 0, 0, -3, 0, 0], dtype=np.float32),
}
# (lens, warp of eye_warp_ref.WARPS) -> the share class of a 128 x 128 patch over a 160 x 200 frame that falls outside; a pair not
# listed has the plain warp's class
OUTSIDE = {('pole', 'integer-shift'): 'some', ('pole', 'fractional-shift'): 'some'}


def outside_kind(lens_name, warp_name):
    return OUTSIDE.get((lens_name, warp_name), ref.WARPS[warp_name][1])


def lens_row(fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0, k4=0.0, k5=0.0, k6=0.0):
    return np.array([fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6], dtype=np.float32)


def takes_the_plain_path(row):
    """All eight coefficients +-0 (a NaN is not zero)."""
    return not np.any(np.asarray(row)[4:] != 0)


def distort(u, v, row):
    """(u, v) float64 arrays, pixels of the undistorted image; row: 12 values -> (ud, vd, den), the contract's expressions."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6 = (np.float64(t) for t in row)
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    with np.errstate(all='ignore'):
        x, y = (u - cx) / fx, (v - cy) / fy
        xx, yy, xy = x * x, y * y, x * y
        r2 = xx + yy
        num = ((k3 * r2 + k2) * r2 + k1) * r2 + 1.0
        den = ((k6 * r2 + k5) * r2 + k4) * r2 + 1.0
        rad, a = num / den, xy + xy
        xd = (x * rad + p1 * a) + p2 * (r2 + (xx + xx))
        yd = (y * rad + p1 * (r2 + (yy + yy))) + p2 * a
        return fx * xd + cx, fy * yd + cy, den


def coordinates(m, row, frame_hw, out_hw):
    """m float32 [3, 3], row float32 [12] -> (fu, fv int64 [OH, OW] fixed-point coordinates with 8 fractional bits, zero where
    outside; inside bool [OH, OW]; pole bool [OH, OW]: den <= 0 although every other comparison holds)."""
    (IH, IW), (OH, OW) = frame_hw, out_hw
    ox = np.arange(OW, dtype=np.float64)[None, :]
    oy = np.arange(OH, dtype=np.float64)[:, None]
    m = np.asarray(m).astype(np.float64)
    with np.errstate(all='ignore'):
        X = (m[0, 0] * ox + m[0, 1] * oy) + m[0, 2]
        Y = (m[1, 0] * ox + m[1, 1] * oy) + m[1, 2]
        Wd = (m[2, 0] * ox + m[2, 1] * oy) + m[2, 2]
        u, v = X / Wd, Y / Wd
        front = Wd > 0
        pole = np.zeros((OH, OW), dtype=bool)
        if not takes_the_plain_path(row):
            u, v, den = distort(u, v, row)
            pole = ~(den > 0)
        framed = front & (u > -1) & (u < IW) & (v > -1) & (v < IH)
        inside = framed & ~pole
        fu = np.where(inside, np.floor(u * 256.0 + 0.5), 0.0).astype(np.int64)
        fv = np.where(inside, np.floor(v * 256.0 + 0.5), 0.0).astype(np.int64)
    return fu, fv, inside, framed & pole


def tap_sums(frame, fu, fv, inside):
    """eye_warp_ref.warp_sums' taps and weights on given fixed-point coordinates: frame uint8 [IH, IW, C] -> S int64 [3, OH, OW]."""
    IH, IW = frame.shape[:2]
    x0, ax, y0, ay = fu >> 8, fu & 255, fv >> 8, fv & 255
    padded = np.zeros((IH + 3, IW + 3, 3), dtype=np.int64)          # x0 in [-1, IW]: one zero line before the frame, two behind
    padded[1:IH + 1, 1:IW + 1] = frame[:, :, :3]
    p = lambda dy, dx: padded[y0 + 1 + dy, x0 + 1 + dx]
    w = lambda t: t[..., None]
    s = (w((256 - ax) * (256 - ay)) * p(0, 0) + w(ax * (256 - ay)) * p(0, 1) + w((256 - ax) * ay) * p(1, 0) + w(ax * ay) * p(1, 1))
    return np.where(inside[..., None], s, 0).transpose(2, 0, 1)


def check_lens(lens_shape, N):
    if tuple(lens_shape) != (N, 12):
        raise ValueError('eye_warp: lens must be [N, 12]')


def warp_sums(frames, warps, lens, out_hw):
    """frames uint8 [N, IH, IW, C], warps float32 [N, 3, 3], lens float32 [N, 12] -> (S int64 [N, 3, OH, OW], outside bool [N, OH, OW])."""
    frames, warps, lens = np.asarray(frames), np.asarray(warps), np.asarray(lens)
    assert frames.dtype == np.uint8 and warps.dtype == np.float32 and lens.dtype == np.float32
    ref.check_shapes(frames.shape, warps.shape, out_hw)
    check_lens(lens.shape, frames.shape[0])
    N, IH, IW, C = frames.shape
    S = np.zeros((N, 3) + tuple(out_hw), dtype=np.int64)
    outside = np.zeros((N,) + tuple(out_hw), dtype=bool)
    for n in range(N):
        fu, fv, inside, _ = coordinates(warps[n], lens[n], (IH, IW), out_hw)
        S[n] = tap_sums(frames[n], fu, fv, inside)
        outside[n] = ~inside
    assert S.min() >= 0 and S.max() <= 255 * 65536
    return S, outside


def eye_warp(frames, warps, lens, out_hw):
    """-> (float32 [N, 3, OH, OW], outside bool [N, OH, OW])"""
    S, outside = warp_sums(frames, warps, lens, out_hw)
    return ref.values_of_sums(S), outside


# ------------------------------------------------------------------------------------------------ stand-ins for FakeKernels
def eye_warp_lens_u8_to_nchw(self, frames, warps, lens, out_hw):
    """Stand-in of HipKernels.eye_warp_lens_u8_to_nchw: `class Fakes(FakeKernels): eye_warp_lens_u8_to_nchw = ...`."""
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] not in (3, 4):
        raise TypeError('eye_warp: frames must be uint8 [N, IH, IW, 3 | 4]')
    if warps.dtype != torch.float32 or tuple(warps.shape) != (frames.shape[0], 3, 3):
        raise TypeError('eye_warp: warps must be float32 [N, 3, 3]')
    if not torch.is_tensor(lens) or lens.dtype != torch.float32 or tuple(lens.shape) != (frames.shape[0], 12):
        raise TypeError('eye_warp: lens must be float32 [N, 12]')
    return torch.from_numpy(eye_warp(frames.numpy(), warps.numpy(), lens.numpy(), (int(out_hw[0]), int(out_hw[1])))[0])


def eye_warp_lens_u8_to_stem(self, frames, warps, lens, out_hw, out=None, dtype=torch.bfloat16):
    return self.stem_pack_input(eye_warp_lens_u8_to_nchw(self, frames, warps, lens, out_hw), out=out, dtype=dtype)
