"""The tracking overlay of eve_overlay_render (include/eve_hip.h) in numpy: the contract the kernel must equal bit for bit.

Per output pixel (X, Y) of an IH x IW frame, in 8-bit RGB, the layers in this order:
  1. source    the capture pixel converted as pixel_format_ref.to_rgb converts it (chroma the nearest sample); rgb / rgba / bgra too
  2. heat map  q = rint(clamp(h, 0, 1) * 255) in float32 (NaN -> 0), up-sampled bilinearly (align_corners=False) in fixed point:
                   nx = (2X+1)*HW - IW;  fx = max(nx, 0)*128 // IW;  x0 = min(fx >> 8, HW-1);  x1 = min(x0+1, HW-1);  wx = fx & 255
               (the same in y), a = (q00*(256-wx)*(256-wy) + q01*wx*(256-wy) + q10*(256-wx)*wy + q11*wx*wy + 32768) >> 16,
               alpha = (a*amax + 127) // 255, and per channel v = (v*(255-alpha) + c*alpha + 127) // 255
  3. inset     an opaque replace of the z*h x z*w rectangle at (x0, y0) by inset[(Y-y0)//z, (X-x0)//z] (mirror: column w-1-j)
  4. markers   in index order, each its outline disc (r_outline > 0) and then its fill disc; centre q = rint((x * s) * 8) in float32;
               not drawn when valid == 0, a coordinate is not finite or |q| > 2^20; coverage of a disc of radius r
                   n = #{(i, j) in 0..3 : (8X+2i+1-qx)^2 + (8Y+2j+1-qy)^2 <= 64 r^2};   v = (v*(16-n) + c*n + 8) >> 4
  5. output    rgb, bgr, or nv12 / i420 by the forward integer matrix: Y per pixel, U and V from the 2 x 2 block's (sum + 2) >> 2
A frame with frame_valid == 0 is layer 1 and layer 5 alone.  Everything after the three quantisations is integer arithmetic."""
import numpy as np

import pixel_format_ref as pref

IN_FORMATS = ('rgb', 'rgba', 'bgr', 'bgra', 'nv12', 'i420', 'yuyv')
OUT_FORMATS = ('rgb', 'bgr', 'nv12', 'i420')
# matrix -> (y0, the Y row, the U row, the V row) of the forward (RGB -> YUV) direction
FORWARD = {'bt601': (16, (0.257, 0.504, 0.098), (-0.148, -0.291, 0.439), (0.439, -0.368, -0.071)),
           'bt709': (16, (0.183, 0.614, 0.062), (-0.101, -0.339, 0.439), (0.439, -0.399, -0.040)),
           'jfif': (0, (0.299, 0.587, 0.114), (-0.168736, -0.331264, 0.5), (0.5, -0.418688, -0.081312))}
MAX_MARKERS = 8
MAX_HEAT = 1024
Q_LIMIT = 2 ** 20


def K(c):
    """sign(c) * floor(|c| * 2^20 + 0.5)"""
    return int(np.sign(c)) * int(np.floor(abs(c) * 2.0 ** 20 + 0.5))


def forward_constants(matrix):
    """-> (y0, (KYR, KYG, KYB), (KUR, KUG, KUB), (KVR, KVG, KVB))"""
    if matrix not in FORWARD:
        raise ValueError('unknown matrix %r' % (matrix,))
    y0, *rows = FORWARD[matrix]
    return (y0,) + tuple(tuple(K(c) for c in row) for row in rows)


def _row(k, offset, rgb):
    rgb = rgb.astype(np.int64)
    s = k[0] * rgb[..., 0] + k[1] * rgb[..., 1] + k[2] * rgb[..., 2] + (offset << 20) + (1 << 19)
    assert np.abs(s).max(initial=0) < 2 ** 30
    return np.clip(s >> 20, 0, 255).astype(np.uint8)


def rgb_to_yuv(rgb, matrix):
    """uint8 [..., 3] -> (Y, U, V) uint8 [...], each pixel by itself (no sub-sampling)."""
    y0, ky, ku, kv = forward_constants(matrix)
    return _row(ky, y0, rgb), _row(ku, 128, rgb), _row(kv, 128, rgb)


def to_rgb(buf, fmt, matrix='bt601'):
    """Layer 1: a buffer uint8 [N, ...] of any input format -> uint8 [N, IH, IW, 3]."""
    buf = np.asarray(buf)
    assert buf.dtype == np.uint8
    if fmt in ('rgb', 'rgba'):
        assert buf.ndim == 4 and buf.shape[-1] == (4 if fmt == 'rgba' else buf.shape[-1]) and buf.shape[-1] in (3, 4)
        return np.ascontiguousarray(buf[..., :3])
    if fmt == 'bgra':
        assert buf.shape[-1] == 4
        fmt = 'bgr'
    return pref.to_rgb(buf, fmt, matrix)


def from_rgb(rgb, out_fmt, matrix='bt601'):
    """Layer 5: uint8 [N, IH, IW, 3] -> the output buffer ([N, IH, IW, 3] or [N, IH*3/2, IW])."""
    N, IH, IW, _ = rgb.shape
    if out_fmt == 'rgb':
        return np.ascontiguousarray(rgb)
    if out_fmt == 'bgr':
        return np.ascontiguousarray(rgb[..., ::-1])
    if out_fmt not in ('nv12', 'i420'):
        raise ValueError('unknown output format %r' % (out_fmt,))
    if IH % 2 or IW % 2:
        raise ValueError('%s output needs even IH and IW, got %d x %d' % (out_fmt, IH, IW))
    y0, ky, ku, kv = forward_constants(matrix)
    Y = _row(ky, y0, rgb)
    v = rgb.astype(np.int64)
    mean = (v[:, 0::2, 0::2] + v[:, 0::2, 1::2] + v[:, 1::2, 0::2] + v[:, 1::2, 1::2] + 2) >> 2
    return pref.pack(Y, _row(ku, 128, mean), _row(kv, 128, mean), out_fmt)


def out_shape(out_fmt, N, IH, IW):
    return (N, IH, IW, 3) if out_fmt in ('rgb', 'bgr') else (N, IH * 3 // 2, IW)


def quantise_heat(heat):
    """float32 [...] -> int64 0..255: rint(clamp(h, 0, 1) * 255) in float32, NaN -> 0."""
    h = np.asarray(heat, dtype=np.float32)
    h = np.where(np.isnan(h), np.float32(0), h)
    h = np.minimum(np.maximum(h, np.float32(0)), np.float32(1))
    return np.rint(h * np.float32(255)).astype(np.int64)


def _axis(I, H):
    """The fixed-point taps along one axis: I output pixels over H heat cells -> (i0, i1, w) int64 [I]."""
    X = np.arange(I, dtype=np.int64)
    n = (2 * X + 1) * H - I
    f = np.maximum(n, 0) * 128 // I
    i0 = np.minimum(f >> 8, H - 1)
    return i0, np.minimum(i0 + 1, H - 1), f & 255


def heat_alpha(heat, IH, IW, amax):
    """float32 [N, HH, HW] -> alpha int64 [N, IH, IW] in 0..amax."""
    q = quantise_heat(heat)
    y0, y1, wy = _axis(IH, q.shape[1])
    x0, x1, wx = _axis(IW, q.shape[2])
    wy, wx = wy[:, None], wx[None, :]
    a = (q[:, y0][:, :, x0] * (256 - wx) * (256 - wy) + q[:, y0][:, :, x1] * wx * (256 - wy) +
         q[:, y1][:, :, x0] * (256 - wx) * wy + q[:, y1][:, :, x1] * wx * wy + 32768) >> 16
    return (a * int(amax) + 127) // 255


def quantise_centres(centres, sx, sy):
    """float32 [N, M, 2] -> (q float32 [N, M, 2] = rint((c * s) * 8) with each product rounded, drawable bool [N, M])."""
    c = np.asarray(centres, dtype=np.float32)
    s = np.array([sx, sy], dtype=np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        q = np.rint((c * s).astype(np.float32) * np.float32(8)).astype(np.float32)
        ok = np.isfinite(c).all(axis=-1) & (np.abs(q) <= np.float32(Q_LIMIT)).all(axis=-1)
    return q, ok


def coverage(IH, IW, qx, qy, r):
    """The 4 x 4 sub-sample count of the disc of radius r (output pixels) about (qx, qy) (eighths of a pixel) -> int64 [IH, IW].
    Only the pixels with a sub-sample inside the disc's bounding box are evaluated: outside it one of |dx|, |dy| exceeds 8 r."""
    qx, qy, r = int(qx), int(qy), int(r)
    cov = np.zeros((IH, IW), dtype=np.int64)
    # pixel P has sub-samples 8P+1 .. 8P+7: it can be touched iff 8P+7 >= q-8r and 8P+1 <= q+8r
    x_lo, x_hi = max(-((7 - qx + 8 * r) // 8), 0), min((qx + 8 * r - 1) // 8, IW - 1)
    y_lo, y_hi = max(-((7 - qy + 8 * r) // 8), 0), min((qy + 8 * r - 1) // 8, IH - 1)
    if x_lo > x_hi or y_lo > y_hi:
        return cov
    sub = 2 * np.arange(4, dtype=np.int64) + 1
    dx = (8 * np.arange(x_lo, x_hi + 1, dtype=np.int64)[:, None] + sub[None, :] - qx) ** 2           # [w, 4]
    dy = (8 * np.arange(y_lo, y_hi + 1, dtype=np.int64)[:, None] + sub[None, :] - qy) ** 2           # [h, 4]
    cov[y_lo:y_hi + 1, x_lo:x_hi + 1] = (dy[:, None, :, None] + dx[None, :, None, :] <= 64 * r * r).sum(axis=(2, 3))
    return cov


def split_rgb(c):
    return (int(c) >> 16) & 255, (int(c) >> 8) & 255, int(c) & 255


def draw(rgb, markers=None, heat=None, inset=None, frame_valid=None):
    """Layers 2 to 4 on uint8 [N, IH, IW, 3] -> uint8 [N, IH, IW, 3].
    markers: dict(centres float32 [N, M, 2], valid uint8 [N, M] or None, table int32 [M, 4], sx, sy);
    heat: dict(heat float32 [N, HH, HW], color (r, g, b), amax);  inset: dict(inset uint8 [N, h, w, 3], x0, y0, zoom, mirror)."""
    N, IH, IW, _ = rgb.shape
    v = rgb.astype(np.int64)
    if heat is not None:
        h = np.asarray(heat['heat'])
        if h.ndim != 3 or h.shape[0] != N or not (1 <= h.shape[1] <= MAX_HEAT and 1 <= h.shape[2] <= MAX_HEAT):
            raise ValueError('heat must be [N, HH, HW] with HH, HW <= %d, got %s' % (MAX_HEAT, h.shape))
        if not 0 <= int(heat['amax']) <= 255:
            raise ValueError('amax must be in 0..255')
        alpha = heat_alpha(h, IH, IW, heat['amax'])[..., None]
        v = (v * (255 - alpha) + np.array(heat['color'], dtype=np.int64) * alpha + 127) // 255
    if inset is not None:
        p = np.asarray(inset['inset'])
        z, x0, y0 = int(inset.get('zoom', 1)), int(inset['x0']), int(inset['y0'])
        if p.dtype != np.uint8 or p.ndim != 4 or p.shape[0] != N or p.shape[3] != 3:
            raise ValueError('inset must be uint8 [N, h, w, 3]')
        if not 1 <= z <= 4:
            raise ValueError('zoom must be in 1..4')
        h, w = p.shape[1:3]
        if x0 < 0 or y0 < 0 or x0 + z * w > IW or y0 + z * h > IH:
            raise ValueError('the inset rectangle does not lie inside the frame')
        if inset.get('mirror', False):
            p = p[:, :, ::-1]
        v[:, y0:y0 + z * h, x0:x0 + z * w] = np.repeat(np.repeat(p, z, axis=1), z, axis=2)
    if markers is not None:
        table = np.asarray(markers['table'], dtype=np.int64).reshape(-1, 4)
        M = table.shape[0]
        if M > MAX_MARKERS:
            raise ValueError('at most %d markers' % MAX_MARKERS)
        if M and ((table[:, :2] < 0) | (table[:, :2] > 255)).any():
            raise ValueError('radii must be in 0..255')
        q, ok = quantise_centres(np.asarray(markers['centres']).reshape(N, M, 2), markers.get('sx', 1.0), markers.get('sy', 1.0))
        valid = markers.get('valid')
        if valid is not None:
            ok = ok & (np.asarray(valid).reshape(N, M) != 0)
        for n in range(N):
            for m in range(M):
                if not ok[n, m]:
                    continue
                r_fill, r_out, c_fill, c_out = (int(t) for t in table[m])
                for r, c in ((r_out, c_out), (r_fill, c_fill))[r_out <= 0:]:         # the fill disc at every radius, 0 included
                    cov = coverage(IH, IW, q[n, m, 0], q[n, m, 1], r)[..., None]
                    v[n] = (v[n] * (16 - cov) + np.array(split_rgb(c), dtype=np.int64) * cov + 8) >> 4
    out = v.astype(np.uint8)
    if frame_valid is not None:
        keep = np.asarray(frame_valid).reshape(N) != 0
        out[~keep] = rgb[~keep]
    return out


def render(frames, fmt, out_fmt, matrix='bt601', markers=None, heat=None, inset=None, frame_valid=None):
    """The whole contract: a capture buffer uint8 [N, ...] of format fmt -> the annotated buffer of out_fmt."""
    if fmt not in IN_FORMATS:
        raise ValueError('unknown input format %r' % (fmt,))
    return from_rgb(draw(to_rgb(frames, fmt, matrix), markers, heat, inset, frame_valid), out_fmt, matrix)
