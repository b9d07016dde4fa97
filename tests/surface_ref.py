"""Surfaces (include/eve_hip.h eve_surface, eve_amd.data.SurfaceLayout) in numpy: frames as a decoder or a capture API leaves them
in memory -- pitched rows, coded rows below the picture, aligned planes, a crop -- and their relation to the byte-linear formats the
existing entry points take.

    linear(buf, layout)          gathers the visible region into a byte-linear frame of the nearest existing format (LINEAR_FORMAT):
                                 nv21 -> nv12 by swapping U and V, yv12 -> i420, uyvy -> yuyv, p010 -> nv12 by taking the high byte of
                                 every 16-bit word, pitched or cropped rgb(a) / bgr(a) -> tight three-channel rgb / bgr
    embed(frame, layout, fill)   the inverse: the frame written into a padded buffer whose other bytes are `fill`
    components(buf, layout)      the address rule itself, stated once: component c of pixel (x, y) is byte
                                 offset[c] + (y >> ys) * pitch[c] + (x >> xs) * step[c] of the frame

linear and embed slice planes by the layout's own parameters (format, pitch, coded_height, x0, y0, plane_offsets) and never look at
the descriptor; components reads ONLY the descriptor.  tests/test_surface_host.py holds the two against each other, so a wrong
offset, pitch or step in SurfaceLayout cannot hide behind the stand-in kernels.  The contract of the surface entry points is then
    surface_call(buf, layout) == format_call(linear(buf, layout))          bit for bit."""
import numpy as np

import pixel_format_ref as pref

FORMATS = ('rgb', 'rgba', 'bgr', 'bgra', 'nv12', 'nv21', 'i420', 'yv12', 'yuyv', 'uyvy', 'p010')
# the byte-linear format linear() produces, in the names of kernels.pixel_format_shape
LINEAR_FORMAT = {'rgb': 'rgb', 'rgba': 'rgb', 'bgr': 'bgr', 'bgra': 'bgr', 'nv12': 'nv12', 'nv21': 'nv12', 'i420': 'i420', 'yv12': 'i420',
                 'yuyv': 'yuyv', 'uyvy': 'yuyv', 'p010': 'nv12'}
BYTES_PER_PIXEL = {'rgb': 3, 'rgba': 4, 'bgr': 3, 'bgra': 4, 'nv12': 1, 'nv21': 1, 'i420': 1, 'yv12': 1, 'yuyv': 2, 'uyvy': 2, 'p010': 2}


def _flat(buf, layout):
    buf = np.asarray(buf)
    assert buf.dtype == np.uint8 and buf.size % layout.frame_bytes == 0, (buf.dtype, buf.shape, layout.frame_bytes)
    return buf.reshape(-1, layout.frame_bytes)


def _window(buf, start, pitch, rows, y0, h, b0, nbytes):
    """The [N, h, nbytes] view of a plane that starts at byte `start` of every frame with `rows` rows of `pitch` bytes: rows
    y0 .. y0 + h - 1, bytes b0 .. b0 + nbytes - 1 of each."""
    plane = buf[:, start:start + pitch * rows].reshape(buf.shape[0], rows, pitch)
    return plane[:, y0:y0 + h, b0:b0 + nbytes]


def _views(buf, L):
    """The writable views of buf [N, frame_bytes] that hold the visible region, per plane, as the format stores them."""
    f, W, H, P, x0, y0, bpp = L.format, L.width, L.height, L.pitch, L.x0, L.y0, BYTES_PER_PIXEL[L.format]
    first = _window(buf, 0, P, L.coded_height, y0, H, x0 * bpp, W * bpp)
    crows = (L.coded_height + 1) // 2
    if f in ('nv12', 'nv21', 'p010'):
        return first, _window(buf, L.plane_offsets[0], P, crows, y0 // 2, H // 2, x0 * bpp, W * bpp)
    if f in ('i420', 'yv12'):
        return (first,) + tuple(_window(buf, s_, P // 2, crows, y0 // 2, H // 2, x0 // 2, W // 2) for s_ in L.plane_offsets)
    return (first,)


def linear(buf, layout):
    """buf: uint8 [N, frame_bytes] (or anything that reshapes to it) -> the byte-linear frames of LINEAR_FORMAT[layout.format]:
    [N, H, W, 3] for the rgb / bgr kinds, [N, H*3/2, W] for nv12 / i420, [N, H, W, 2] for yuyv."""
    buf = _flat(buf, layout)
    N, f, W, H = buf.shape[0], layout.format, layout.width, layout.height
    v = _views(buf, layout)
    if f in ('rgb', 'rgba', 'bgr', 'bgra'):
        return np.ascontiguousarray(v[0].reshape(N, H, W, -1)[..., :3])                  # a fourth channel is dropped
    if f == 'yuyv':
        return np.ascontiguousarray(v[0].reshape(N, H, W, 2))
    if f == 'uyvy':
        return np.ascontiguousarray(v[0].reshape(N, H, W, 2)[..., ::-1])                 # U Y V Y -> Y U Y V
    if f in ('nv12', 'nv21', 'p010'):
        y, c = v
        if f == 'p010':                                                                  # little-endian words: the high byte
            y, c = y[..., 1::2], c[..., 1::2]
        if f == 'nv21':
            c = c.reshape(N, H // 2, W // 2, 2)[..., ::-1].reshape(N, H // 2, W)         # V U -> U V
        return np.ascontiguousarray(np.concatenate([y, c], axis=1))
    y, p1, p2 = v                                                                        # i420: U, V; yv12: V, U
    u, w = (p2, p1) if f == 'yv12' else (p1, p2)
    return np.concatenate([y.reshape(N, -1), u.reshape(N, -1), w.reshape(N, -1)], axis=1).reshape(N, H * 3 // 2, W)


def embed(frame, layout, fill):
    """The inverse of linear: frame as linear returns it -> uint8 [N, frame_bytes] with the visible bytes written and every other
    byte taken from fill (a scalar, or an array of the buffer's shape).  The bytes linear drops -- a fourth channel, P010's low
    bytes -- are padding like the rest: they keep the fill."""
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8
    N, f, W, H = frame.shape[0], layout.format, layout.width, layout.height
    buf = np.empty((N, layout.frame_bytes), dtype=np.uint8)
    buf[...] = fill
    v = _views(buf, layout)
    if f in ('rgb', 'rgba', 'bgr', 'bgra'):
        v[0].reshape(N, H, W, -1)[..., :3] = frame.reshape(N, H, W, 3)
    elif f == 'yuyv':
        v[0][...] = frame.reshape(N, H, W * 2)
    elif f == 'uyvy':
        v[0][...] = frame.reshape(N, H, W, 2)[..., ::-1].reshape(N, H, W * 2)
    elif f in ('nv12', 'nv21', 'p010'):
        rows = frame.reshape(N, H * 3 // 2, W)
        y, c = rows[:, :H], rows[:, H:]
        if f == 'nv21':
            c = c.reshape(N, H // 2, W // 2, 2)[..., ::-1].reshape(N, H // 2, W)
        if f == 'p010':
            v[0][..., 1::2], v[1][..., 1::2] = y, c
        else:
            v[0][...], v[1][...] = y, c
    else:
        flat = frame.reshape(N, -1)
        q = (H // 2) * (W // 2)
        y, u, w = flat[:, :H * W], flat[:, H * W:H * W + q], flat[:, H * W + q:]
        p1, p2 = (w, u) if f == 'yv12' else (u, w)
        v[0][...] = y.reshape(N, H, W)
        v[1][...], v[2][...] = p1.reshape(N, H // 2, W // 2), p2.reshape(N, H // 2, W // 2)
    return buf


def components(buf, layout):
    """The address rule on the descriptor alone: buf uint8 [N, frame_stride] -> uint8 [N, H, W, 3], the three components of every
    visible pixel (R, G, B for the rgb kinds; Y, U, V with chroma the nearest sample for the yuv ones).  Every index is asserted
    to lie below frame_bytes."""
    d = layout.descriptor()
    buf = np.asarray(buf).reshape(-1, d['frame_stride'])
    y, x = np.meshgrid(np.arange(d['height'], dtype=np.int64), np.arange(d['width'], dtype=np.int64), indexing='ij')
    out = np.empty((buf.shape[0], d['height'], d['width'], 3), dtype=np.uint8)
    for c in range(3):
        xs, ys = (d['xshift'], d['yshift']) if c and d['kind'] == 1 else (0, 0)
        at = d['offset'][c] + (y >> ys) * d['pitch'][c] + (x >> xs) * d['step'][c]
        assert at.min() >= 0 and at.max() < d['frame_bytes']
        out[..., c] = buf[:, at]
    return out


def linear_components(frame, fmt):
    """What components() must give, from the byte-linear frame linear() returned: [N, H, W, 3] R, G, B or Y, U, V."""
    if fmt == 'rgb':
        return np.asarray(frame)[..., :3]
    if fmt == 'bgr':
        return np.asarray(frame)[..., 2::-1]
    return np.stack(pref.planes(frame, fmt), axis=-1)


def random_surface(layout, N, seed):
    """-> (buf uint8 [N, frame_bytes] of uniform random bytes, padding included; its linear frames)."""
    buf = np.random.default_rng(seed).integers(0, 256, size=(N, layout.frame_bytes), dtype=np.uint8)
    return buf, linear(buf, layout)
