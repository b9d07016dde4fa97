"""eve_screen_luminance (include/eve_hip.h) in numpy: the mean relative luminance of screen captures over the whole visible region
and over concentric discs around a per-frame centre.  Integers up to one float64 division, so there is nothing to agree on but the
formulas, and the device equals this bit for bit.

    rgb_of(buf, layout, matrix)      the 8-bit (R, G, B) of every visible pixel: surface_ref.linear, then pixel_format_ref.to_rgb --
                                     exactly what eve_screen_area_surface_to_nchw averages
    luminance(...)                   the contract: per pixel y = (kr*t[0][R] + kg*t[1][G] + kb*t[2][B] + 32768) >> 16, summed per region
    brute(...)                       the same from the descriptor's address rule alone, pixel by pixel in Python integers: shares no
                                     line with luminance() but the table
    mean_of_resized(rgb, ...)        the shortcut that is NOT the contract: average the gamma-encoded bytes down first (RefineNet's
                                     resized screen), then linearise the mean byte
    screen_luminance(self, ...)      the stand-in of HipKernels.screen_luminance for the torch-CPU FakeKernels"""
import numpy as np
import torch

import pixel_format_ref as pref
import surface_ref as sref

REC709 = (13933, 46871, 4732)
Q_MAX = 1 << 20


def srgb_table():
    """floor(65535 * eotf(v / 255) + 0.5) in float64, uint16 [3, 256]: written out here, not taken from the package."""
    v = np.arange(256, dtype=np.float64) / 255.0
    f = np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)
    return np.broadcast_to(np.floor(65535.0 * f + 0.5).astype(np.uint16), (3, 256)).copy()


def rgb_of(buf, layout, matrix='bt601'):
    """buf uint8 [N, frame_bytes] -> uint8 [N, H, W, 3]."""
    lin = sref.linear(buf, layout)
    fmt = sref.LINEAR_FORMAT[layout.format]
    return np.ascontiguousarray(lin[..., :3]) if fmt == 'rgb' else pref.to_rgb(lin, fmt, matrix)


def pixel_values(rgb, table, weights):
    """uint8 [..., 3] -> the per-pixel y, int64 [...] in 0 .. 65535."""
    t = np.asarray(table).astype(np.int64)
    kr, kg, kb = (int(w) for w in weights)
    s = kr * t[0][rgb[..., 0]] + kg * t[1][rgb[..., 1]] + kb * t[2][rgb[..., 2]] + 32768
    assert s.max(initial=0) < 2 ** 32
    return s >> 16


def quantise(centres, sx, sy):
    """float32 [N, 2] -> (qx, qy float32 [N]): rint((c * s) * 2) in float32, each product rounded, ties to even."""
    c = np.asarray(centres, dtype=np.float32).reshape(-1, 2)
    with np.errstate(over='ignore', invalid='ignore'):
        qx = np.rint((c[:, 0] * np.float32(sx)) * np.float32(2))
        qy = np.rint((c[:, 1] * np.float32(sy)) * np.float32(2))
    return qx.astype(np.float32), qy.astype(np.float32)


def delivered(B, T, lengths):
    if lengths is None:
        return np.ones(B * T, dtype=bool)
    n = np.clip(np.asarray(lengths).astype(np.int64), 0, T)
    return (np.arange(T)[None, :] < n[:, None]).reshape(-1)


def finish(sums, counts):
    with np.errstate(divide='ignore', invalid='ignore'):
        return (sums.astype(np.float64) / (counts.astype(np.float64) * 65535.0)).astype(np.float32)


def luminance(buf, layout, table, weights, B, T, radii=(), centres=None, sx=1.0, sy=1.0, centre_valid=None, lengths=None, matrix='bt601'):
    """-> (sums int64, counts int32, mean float32), each [B * T, 1 + R]."""
    N, R = B * T, len(radii)
    y = pixel_values(rgb_of(np.asarray(buf).reshape(N, -1), layout, matrix), table, weights)       # [N, H, W]
    H, W = y.shape[1:]
    sums, counts = np.zeros((N, 1 + R), dtype=np.int64), np.zeros((N, 1 + R), dtype=np.int32)
    live = delivered(B, T, lengths)
    sums[live, 0] = y[live].sum(axis=(1, 2))
    counts[live, 0] = W * H
    if R:
        qx, qy = quantise(centres, sx, sy)
        ok = live & (np.abs(qx) <= Q_MAX) & (np.abs(qy) <= Q_MAX)                                   # (a NaN compares False)
        if centre_valid is not None:
            ok &= np.asarray(centre_valid).reshape(-1) != 0
        X, Y = np.arange(W, dtype=np.int64)[None, :], np.arange(H, dtype=np.int64)[:, None]
        for n in np.nonzero(ok)[0]:
            dd = (2 * X + 1 - int(qx[n])) ** 2 + (2 * Y + 1 - int(qy[n])) ** 2
            for k, r in enumerate(radii):
                inside = dd <= 4 * int(r) * int(r)
                sums[n, 1 + k], counts[n, 1 + k] = y[n][inside].sum(), inside.sum()
    return sums, counts, finish(sums, counts)


def brute(buf, layout, table, weights, B, T, radii=(), centres=None, sx=1.0, sy=1.0, centre_valid=None, lengths=None, matrix='bt601'):
    """luminance() once more: every pixel's three bytes through the descriptor's address rule, the YUV matrix and the weighting in
    Python integers, one pixel at a time."""
    d = layout.descriptor()
    N, R, W, H = B * T, len(radii), d['width'], d['height']
    buf = np.asarray(buf).reshape(N, -1)
    t = [[int(v) for v in row] for row in np.asarray(table)]
    y0, CY, CVR, CUG, CVG, CUB = pref.constants(matrix)
    clamp = lambda s: min(255, max(0, s >> 20))
    sums, counts = [[0] * (1 + R) for _ in range(N)], [[0] * (1 + R) for _ in range(N)]
    qx, qy = quantise(centres, sx, sy) if R else (None, None)
    for n in range(N):
        b, f = divmod(n, T)
        if lengths is not None and f >= min(max(int(lengths[b]), 0), T):
            continue
        disc = R > 0 and (centre_valid is None or int(np.asarray(centre_valid).reshape(-1)[n]) != 0) and \
            bool(np.isfinite(qx[n]) and np.isfinite(qy[n]) and abs(float(qx[n])) <= Q_MAX and abs(float(qy[n])) <= Q_MAX)
        for Y in range(H):
            for X in range(W):
                c = []
                for ch in range(3):
                    xs, ys = (d['xshift'], d['yshift']) if ch and d['kind'] == 1 else (0, 0)
                    at = d['offset'][ch] + (Y >> ys) * d['pitch'][ch] + (X >> xs) * d['step'][ch]
                    assert 0 <= at < d['frame_bytes']
                    c.append(int(buf[n, at]))
                if d['kind'] == 1:
                    yy = max(0, c[0] - y0) * CY + (1 << 19)
                    u, v = c[1] - 128, c[2] - 128
                    c = [clamp(yy + CVR * v), clamp(yy - CVG * v - CUG * u), clamp(yy + CUB * u)]
                val = (weights[0] * t[0][c[0]] + weights[1] * t[1][c[1]] + weights[2] * t[2][c[2]] + 32768) >> 16
                sums[n][0] += val
                counts[n][0] += 1
                if disc:
                    dd = (2 * X + 1 - int(qx[n])) ** 2 + (2 * Y + 1 - int(qy[n])) ** 2
                    for k, r in enumerate(radii):
                        if dd <= 4 * r * r:
                            sums[n][1 + k] += val
                            counts[n][1 + k] += 1
    sums, counts = np.array(sums, dtype=np.int64).reshape(N, 1 + R), np.array(counts, dtype=np.int32).reshape(N, 1 + R)
    return sums, counts, finish(sums, counts)


def disc_count(W, H, r, qx, qy):
    """The visible pixels of a W x H frame inside the disc of radius r around (qx, qy) half pixels."""
    return sum(1 for Y in range(H) for X in range(W) if (2 * X + 1 - qx) ** 2 + (2 * Y + 1 - qy) ** 2 <= 4 * r * r)


def mean_of_resized(rgb, table, weights, factor):
    """The shortcut: box-average the gamma-encoded bytes of uint8 [H, W, 3] over factor x factor blocks, round to a byte, linearise
    and weigh that -- what a luminance taken from a down-sampled screen computes.  -> the frame's mean in 0 .. 1."""
    H, W, _ = rgb.shape
    assert H % factor == 0 and W % factor == 0
    small = rgb.astype(np.float64).reshape(H // factor, factor, W // factor, factor, 3).mean(axis=(1, 3))
    y = pixel_values(np.floor(small + 0.5).astype(np.int64), table, weights)
    return float(y.mean() / 65535.0)


def covariate(mean, to_pupil):
    """The left-to-right chain of float32 products and sums over the columns of weight != 0: float32 [N]."""
    cov = None
    for k, w in enumerate(to_pupil):
        if w == 0:
            continue
        term = (mean[:, k] * np.float32(w)).astype(np.float32)
        cov = term if cov is None else (cov + term).astype(np.float32)
    return cov


# ------------------------------------------------------------------------------------------------ stand-in for FakeKernels
def screen_luminance(self, frames, layout, response, weights, B, T, radii=(), centres=None, sx=1.0, sy=1.0, centre_valid=None, lengths=None,
                     matrix='bt601'):
    """Stand-in of HipKernels.screen_luminance: the wrapper's own checks, then luminance()."""
    from eve_amd.kernels import HipKernels
    HipKernels._surface_args('screen_luminance', frames, layout, matrix)
    if hasattr(self, 'calls'):
        self.calls.append('screen_luminance')
    n = lambda t: None if t is None else t.detach().numpy()
    sums, counts, mean = luminance(n(frames), layout, response.numpy().view(np.uint16), tuple(int(w) for w in weights), int(B), int(T),
                                   tuple(int(r) for r in radii), n(centres), float(np.float32(sx)), float(np.float32(sy)), n(centre_valid),
                                   n(lengths), matrix)
    return torch.from_numpy(sums), torch.from_numpy(counts), torch.from_numpy(mean)
