"""The contract of eve_screen_area_fmt_to_nchw (include/eve_hip.h) in numpy: the area average of screen_resize_ref on the frame
pixel_format_ref.to_rgb converts -- CONVERT, THEN AVERAGE -- plus an independent brute-force evaluation of it, the tempting
shortcut that is NOT the contract (average Y, U and V, convert once), test frames, and a stand-in of
HipKernels.screen_area_fmt_to_nchw for the torch-CPU FakeKernels.

    screen_area_F(buf) == eve_screen_u8_area_to_nchw(to_rgb(buf, F, M))        bit for bit, F in nv12, i420, yuyv"""
import numpy as np
import torch

import pixel_format_ref as pref
import screen_resize_ref as sref

FORMATS = ('nv12', 'i420', 'yuyv')
# (y0, CY, CVR, CUG, CVG, CUB) as include/eve_hip.h lists them: brute_force reads these, not pixel_format_ref.constants
HEADER_CONSTANTS = {'bt601': (16, 1220542, 1673527, 409993, 852492, 2116026), 'bt709': (16, 1220542, 1880097, 223347, 558891, 2214593),
                    'jfif': (0, 1048576, 1470104, 360853, 748826, 1858077)}


def screen_area(buf, out_hw, fmt, matrix='bt601'):
    """THE CONTRACT: a buffer uint8 [N, ...] of format fmt -> float32 [N, 3, OH, OW]."""
    if fmt not in FORMATS:
        raise ValueError('unknown format %r' % (fmt,))
    return sref.area_resize(pref.to_rgb(buf, fmt, matrix), out_hw)


def yuv_at(flat, fmt, IH, IW, y, x):
    """(Y, U, V) of pixel (y, x) as Python ints, by the byte offsets include/eve_hip.h states for one frame's flat bytes."""
    if fmt == 'nv12':
        c = IH * IW + (y >> 1) * IW + (x & ~1)
        return int(flat[y * IW + x]), int(flat[c]), int(flat[c + 1])
    if fmt == 'i420':
        c = IH * IW + (y >> 1) * (IW // 2) + (x >> 1)
        return int(flat[y * IW + x]), int(flat[c]), int(flat[c + (IH // 2) * (IW // 2)])
    if fmt == 'yuyv':
        return int(flat[(y * IW + x) * 2]), int(flat[(y * IW + (x & ~1)) * 2 + 1]), int(flat[(y * IW + (x | 1)) * 2 + 1])
    raise ValueError('unknown format %r' % (fmt,))


def brute_force(buf, out_hw, fmt, matrix='bt601'):
    """The contract again with nothing shared: for every output pixel a plain loop over ALL source pixels, Python integers for the
    conversion, the weights and the sum, one float64 division, one float32 multiply."""
    buf = np.asarray(buf)
    N = buf.shape[0]
    IH, IW = pref.frame_hw(buf.shape, fmt)
    OH, OW = out_hw
    y0, CY, CVR, CUG, CVG, CUB = HEADER_CONSTANTS[matrix]
    clamp = lambda s_: min(255, max(0, s_ >> 20))            # (Python's >> on a negative int is arithmetic)
    out = np.zeros((N, 3, OH, OW), dtype=np.float32)
    for n in range(N):
        flat = buf[n].reshape(-1)
        rgb = [[None] * IW for _ in range(IH)]
        for y in range(IH):
            for x in range(IW):
                Y, U, V = yuv_at(flat, fmt, IH, IW, y, x)
                yy, u, v = max(0, Y - y0) * CY + (1 << 19), U - 128, V - 128
                rgb[y][x] = (clamp(yy + CVR * v), clamp(yy - CVG * v - CUG * u), clamp(yy + CUB * u))
        for oy in range(OH):
            for ox in range(OW):
                S = [0, 0, 0]
                for y in range(IH):
                    wy = max(0, min((y + 1) * OH, (oy + 1) * IH) - max(y * OH, oy * IH))
                    for x in range(IW):
                        w = wy * max(0, min((x + 1) * OW, (ox + 1) * IW) - max(x * OW, ox * IW))
                        for c in range(3):
                            S[c] += w * rgb[y][x][c]
                for c in range(3):
                    assert S[c] < 2 ** 32
                    out[n, c, oy, ox] = np.float32(np.float64(S[c]) / np.float64(IH * IW)) * np.float32(1.0 / 255.0)
    return out


def average_then_convert(buf, out_hw, fmt, matrix='bt601'):
    """NOT the contract: the area average of the Y, U and V planes (rounded to bytes), converted once per output pixel.  The
    clamps make the conversion non-linear, so this differs wherever a clamp acts; the tests show that their frames see it."""
    Y, U, V = pref.planes(buf, fmt)
    IH, IW = Y.shape[1:]
    mean = lambda p: np.floor(sref.area_sums(np.repeat(p[..., None], 3, axis=-1), out_hw)[:, 0].astype(np.float64) / (IH * IW) + 0.5).astype(np.uint8)
    rgb = pref.yuv_to_rgb(mean(Y), mean(U), mean(V), matrix)                  # [N, OH, OW, 3]
    return rgb.transpose(0, 3, 1, 2).astype(np.float32) * np.float32(1.0 / 255.0)


def both_clamps(buf, fmt, matrix='bt601'):
    """True when the converted frames hold both 0 and 255 in every channel: both clamps of the conversion act."""
    rgb = pref.to_rgb(buf, fmt, matrix)
    return all((rgb[..., c] == 0).any() and (rgb[..., c] == 255).any() for c in range(3))


# ------------------------------------------------------------------------------------------------ stand-in for FakeKernels
def screen_area_fmt_to_nchw(self, frames, out_hw, format, matrix='bt601'):
    """Stand-in of HipKernels.screen_area_fmt_to_nchw: attach it to a FakeKernels subclass.  to_rgb, then the existing stand-in."""
    from eve_amd.kernels import YUV_MATRICES, pixel_format_shape
    pixel_format_shape(frames, format, lead=1)                # the wrapper's own TypeError / ValueError
    if format == 'rgb':
        raise ValueError('screen_area_fmt_to_nchw takes bgr, nv12, i420 or yuyv')
    if matrix not in YUV_MATRICES:
        raise ValueError('screen_area_fmt_to_nchw: unknown matrix %r' % (matrix,))
    if not frames.is_contiguous():
        raise RuntimeError('eve_amd: non-contiguous tensor handed to a kernel')
    return sref.screen_u8_area_to_nchw(self, torch.from_numpy(pref.to_rgb(frames.numpy(), format, matrix)), out_hw)
