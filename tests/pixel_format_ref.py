"""The pixel formats of eve_eye_warp_fmt_to_nchw / eve_eye_warp_fmt_to_stem (include/eve_hip.h) in numpy: the whole-frame
conversion to RGB the contract is stated through, frames to test it with, and stand-ins of the two HipKernels methods (and of
screen_u8_area_bgr_to_nchw) for the torch-CPU FakeKernels.

The contract in one line: for every format F and matrix M, warp_F(buf) == warp_rgb(to_rgb(buf, F, M)) bit for bit, where to_rgb
converts every pixel as the kernel converts a tap -- int32 arithmetic, arithmetic shifts, chroma the nearest sample:
    yy = max(0, Y - y0) * CY;   u = U - 128;   v = V - 128
    R = clamp((yy + 2^19 + CVR*v)         >> 20, 0, 255)
    G = clamp((yy + 2^19 - CVG*v - CUG*u) >> 20, 0, 255)
    B = clamp((yy + 2^19 + CUB*u)         >> 20, 0, 255)
Layouts, per frame and byte-linear: bgr [IH, IW, 3 | 4]; nv12 [IH*3/2, IW] (luma rows, then IH/2 rows of interleaved U, V); i420
[IH*3/2, IW] (luma, the U plane of (IH/2)*(IW/2) bytes, the V plane); yuyv [IH, IW, 2] (Y U Y V per pixel pair)."""
import numpy as np
import torch

import eye_warp_lens_ref as lref
import eye_warp_ref as ref
import screen_resize_ref as sref

FORMATS = ('bgr', 'nv12', 'i420', 'yuyv')
# matrix -> (the coefficients behind the constants: y scale, V->R, U->G, V->G, U->B; y0)
COEFFICIENTS = {'bt601': ((1.164, 1.596, 0.391, 0.813, 2.018), 16), 'bt709': ((1.164, 1.793, 0.213, 0.533, 2.112), 16),
                'jfif': ((1.0, 1.402, 0.344136, 0.714136, 1.772), 0)}


def constants(matrix):
    """-> (y0, CY, CVR, CUG, CVG, CUB): each constant floor(c * 2^20 + 0.5)."""
    if matrix not in COEFFICIENTS:
        raise ValueError('unknown matrix %r' % (matrix,))
    c, y0 = COEFFICIENTS[matrix]
    return (y0,) + tuple(int(np.floor(x * 2.0 ** 20 + 0.5)) for x in c)


def yuv_to_rgb(Y, U, V, matrix):
    """uint8 arrays of one shape -> uint8 [..., 3] by the integer formulas; the intermediates are checked to stay below 2^30."""
    y0, CY, CVR, CUG, CVG, CUB = constants(matrix)
    Y, U, V = (np.asarray(a).astype(np.int64) for a in (Y, U, V))
    yy = np.maximum(0, Y - y0) * CY + (1 << 19)
    u, v = U - 128, V - 128
    sums = (yy + CVR * v, yy - CVG * v - CUG * u, yy + CUB * u)
    assert all(np.abs(s_).max(initial=0) < 2 ** 30 for s_ in sums)
    return np.stack([np.clip(s_ >> 20, 0, 255) for s_ in sums], axis=-1).astype(np.uint8)


def frame_hw(shape, fmt):
    """The trailing dimensions of a buffer of format fmt -> (IH, IW); ValueError for sizes the format cannot have."""
    if fmt in ('nv12', 'i420'):
        rows, IW = shape[-2:]
        if rows % 3 or IW % 2:
            raise ValueError('%s: [IH*3/2, IW] with IH and IW even, got %s' % (fmt, tuple(shape[-2:])))
        return rows // 3 * 2, IW
    IH, IW, C = shape[-3:]
    if fmt == 'yuyv' and (C != 2 or IW % 2):
        raise ValueError('yuyv: [IH, IW, 2] with IW even, got %s' % (tuple(shape[-3:]),))
    if fmt == 'bgr' and C not in (3, 4):
        raise ValueError('bgr: [IH, IW, 3 | 4], got %s' % (tuple(shape[-3:]),))
    return IH, IW


def planes(buf, fmt):
    """A YUV buffer [N, ...] -> (Y, U, V) uint8 [N, IH, IW], chroma replicated over its 2 x 2 block (yuyv: its pair)."""
    buf = np.asarray(buf)
    N = buf.shape[0]
    IH, IW = frame_hw(buf.shape, fmt)
    if fmt == 'yuyv':
        return buf[..., 0], np.repeat(buf[:, :, 0::2, 1], 2, axis=2), np.repeat(buf[:, :, 1::2, 1], 2, axis=2)
    flat = buf.reshape(N, -1)
    Y = flat[:, :IH * IW].reshape(N, IH, IW)
    if fmt == 'nv12':
        uv = flat[:, IH * IW:].reshape(N, IH // 2, IW // 2, 2)
        U, V = uv[..., 0], uv[..., 1]
    else:
        q = (IH // 2) * (IW // 2)
        U = flat[:, IH * IW:IH * IW + q].reshape(N, IH // 2, IW // 2)
        V = flat[:, IH * IW + q:].reshape(N, IH // 2, IW // 2)
    up = lambda c: np.repeat(np.repeat(c, 2, axis=1), 2, axis=2)
    return Y, up(U), up(V)


def to_rgb(buf, fmt, matrix='bt601'):
    """A buffer uint8 [N, ...] of format fmt -> the RGB frames uint8 [N, IH, IW, 3] the contract is stated through."""
    buf = np.asarray(buf)
    assert buf.dtype == np.uint8
    if fmt == 'bgr':
        frame_hw(buf.shape, fmt)
        return np.ascontiguousarray(buf[..., 2::-1])
    if fmt not in FORMATS:
        raise ValueError('unknown format %r' % (fmt,))
    constants(matrix)
    return yuv_to_rgb(*planes(buf, fmt), matrix)


def pack(Y, U, V, fmt):
    """Planes Y uint8 [N, IH, IW] and U, V uint8 [N, IH/2, IW/2] -> the buffer of fmt.  yuyv has a chroma sample per row and pixel
    pair: it takes U, V as [N, IH, IW/2] too, and repeats 4:2:0 chroma over the two rows of its block."""
    N, IH, IW = Y.shape
    if fmt == 'nv12':
        return np.concatenate([Y.reshape(N, -1), np.stack([U, V], axis=-1).reshape(N, -1)], axis=1).reshape(N, IH * 3 // 2, IW)
    if fmt == 'i420':
        return np.concatenate([Y.reshape(N, -1), U.reshape(N, -1), V.reshape(N, -1)], axis=1).reshape(N, IH * 3 // 2, IW)
    if fmt == 'yuyv':
        if U.shape[1] != IH:                                  # 4:2:0 chroma: each sample serves both rows of its block
            U, V = np.repeat(U, 2, axis=1), np.repeat(V, 2, axis=1)
        out = np.empty((N, IH, IW, 2), dtype=np.uint8)
        out[..., 0] = Y
        out[:, :, 0::2, 1] = U
        out[:, :, 1::2, 1] = V
        return out
    raise ValueError('unknown format %r' % (fmt,))


def buffer_shape(fmt, N, IH, IW, C=3):
    return {'bgr': (N, IH, IW, C), 'nv12': (N, IH * 3 // 2, IW), 'i420': (N, IH * 3 // 2, IW), 'yuyv': (N, IH, IW, 2)}[fmt]


def random_yuv_frames(fmt, N, IH, IW, seed, C=3):
    """Uniform bytes in the layout of fmt (any bytes are valid); bgr with C = 4 carries a constant alpha plane that must leave no trace."""
    v = np.random.default_rng(seed).integers(0, 256, size=buffer_shape(fmt, N, IH, IW, C), dtype=np.uint8)
    if fmt == 'bgr' and C == 4:
        v[..., 3] = 255
    return v


def chroma_checkerboard(fmt, N, IH, IW):
    """Y = 128 everywhere, U and V alternating 16 / 240 from one chroma sample to the next along both chroma axes (V opposite to U),
    the phase shifted per frame: a chroma index off by one block changes every output.  bgr: the pixel checkerboard of eye_warp_ref."""
    if fmt == 'bgr':
        return ref.checkerboard_frames(N, IH, IW, 3)
    rows = IH if fmt == 'yuyv' else IH // 2                   # yuyv has a chroma sample per row and pixel pair
    cy, cx, n = np.arange(rows)[None, :, None], np.arange(IW // 2)[None, None, :], np.arange(N)[:, None, None]
    even = ((cy + cx + n) % 2) == 0
    U = np.where(even, 16, 240).astype(np.uint8)
    V = np.where(even, 240, 16).astype(np.uint8)
    return pack(np.full((N, IH, IW), 128, dtype=np.uint8), U, V, fmt)


def constant_frames(fmt, N, IH, IW, Y, U, V):
    q = (N, IH // 2, IW // 2)
    return pack(np.full((N, IH, IW), Y, dtype=np.uint8), np.full(q, U, dtype=np.uint8), np.full(q, V, dtype=np.uint8), fmt)


def eye_warp(buf, warps, out_hw, fmt, matrix='bt601', lens=None):
    """-> (float32 [N, 3, OH, OW], outside bool [N, OH, OW]): the existing reference on the converted frames."""
    rgb = to_rgb(buf, fmt, matrix)
    return ref.eye_warp(rgb, warps, out_hw) if lens is None else lref.eye_warp(rgb, warps, lens, out_hw)


# ------------------------------------------------------------------------------------------------ stand-ins for FakeKernels
def _checked(frames, fmt, matrix):
    from eve_amd.kernels import YUV_MATRICES, pixel_format_shape
    pixel_format_shape(frames, fmt, lead=1)                   # the wrapper's own TypeError / ValueError
    if fmt == 'rgb':
        raise ValueError('eye_warp: the format calls take bgr, nv12, i420 or yuyv')
    if matrix not in YUV_MATRICES:
        raise ValueError('eye_warp: unknown matrix %r' % (matrix,))
    return torch.from_numpy(to_rgb(frames.numpy(), fmt, matrix))


def eye_warp_fmt_to_nchw(self, frames, warps, out_hw, format, matrix='bt601', lens=None):
    """Stand-in of HipKernels.eye_warp_fmt_to_nchw: to_rgb, then the existing stand-in."""
    rgb = _checked(frames, format, matrix)
    if lens is None:
        return ref.eye_warp_u8_to_nchw(self, rgb, warps, out_hw)
    return lref.eye_warp_lens_u8_to_nchw(self, rgb, warps, lens, out_hw)


def eye_warp_fmt_to_stem(self, frames, warps, out_hw, format, matrix='bt601', lens=None, out=None, dtype=torch.bfloat16):
    return self.stem_pack_input(eye_warp_fmt_to_nchw(self, frames, warps, out_hw, format, matrix, lens), out=out, dtype=dtype)


def screen_u8_area_bgr_to_nchw(self, frames, out_hw):
    """Stand-in of HipKernels.screen_u8_area_bgr_to_nchw: the existing stand-in on the channel-reversed capture."""
    return sref.screen_u8_area_to_nchw(self, torch.from_numpy(np.ascontiguousarray(frames.numpy()[..., 2::-1])), out_hw)
