"""CPU: the tracking overlay's contract (tests/overlay_ref.py) against a brute-force per-pixel evaluation, the forward YUV constants
of csrc/yuv_rgb.h and their round trip, frames with exactly known results, the layer order, every refusal of
kernels.overlay_render's argument check (through a torch-CPU stand-in in the style of test_pixel_format_host.PixelFakes), and the
EVEStream plumbing of step(chunk, render=spec) on the stand-in kernels.  tests/test_gpu_overlay.py checks the HIP kernel."""
import math
import os
import re

import numpy as np
import pytest
import torch

import eve_amd
import overlay_ref as oref
import pixel_format_ref as pref
from eve_amd import kernels
from eve_amd.data import OverlaySpec, quantise_patches, render_overlay
from test_screen_formats_host import ScreenFormatFakes, capture
from test_stream_host import chunk_of, clip
from test_stream_mask_host import MaskFakes
from test_stream_ragged_host import CONFIGS, make_model

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPTURE = (144, 256)


class OverlayFakes(ScreenFormatFakes, MaskFakes):
    """The stand-in of HipKernels.overlay_render: the wrapper's own argument check, then the numpy contract."""

    def overlay_render(self, frames, format, out_format='nv12', matrix='bt601', centres=None, marker_valid=None, marker_table=None, sx=1.0,
                       sy=1.0, heat=None, heat_color=(255, 0, 0), amax=128, inset=None, inset_xy=(0, 0), zoom=1, mirror=False, frame_valid=None,
                       out=None):
        a = kernels.overlay_check(frames, format, out_format, matrix, centres, marker_valid, marker_table, sx, sy, heat, heat_color, amax,
                                  inset, inset_xy, zoom, mirror, frame_valid, out)
        self.calls.append('overlay_render')
        self.last_overlay = dict(frame_valid=None if frame_valid is None else frame_valid.clone(), sx=sx, sy=sy, matrix=matrix,
                                 format=a['in_name'], inset_xy=tuple(inset_xy), frames=frames)
        np_ = lambda t: None if t is None else t.numpy()
        res = oref.render(frames.numpy(), a['in_name'], out_format, matrix,
                          markers=None if centres is None else dict(centres=np_(centres), valid=np_(marker_valid), table=np_(marker_table), sx=sx, sy=sy),
                          heat=None if heat is None else dict(heat=np_(heat), color=heat_color, amax=amax),
                          inset=None if inset is None else dict(inset=np_(inset), x0=inset_xy[0], y0=inset_xy[1], zoom=zoom, mirror=mirror),
                          frame_valid=np_(frame_valid))
        res = torch.from_numpy(res)
        return res if out is None else out.copy_(res)


@pytest.fixture()
def fake():
    k = OverlayFakes()
    kernels.set_default_kernels(k)
    yield k
    kernels.set_default_kernels(None)
    eve_amd.reset_standalone_config()


# ------------------------------------------------------------------------------------------------ brute force, pixel by pixel
def brute(rgb, out_fmt, matrix, markers=None, heat=None, inset=None, frame_valid=None):
    """Layers 2 to 5 with Python integers, one pixel at a time, written from the issue's text and sharing no code with overlay_ref."""
    N, IH, IW, _ = rgb.shape
    img = [[[[int(c) for c in rgb[n, y, x]] for x in range(IW)] for y in range(IH)] for n in range(N)]
    f32 = np.float32
    for n in range(N):
        if frame_valid is not None and not frame_valid[n]:
            continue
        for Y in range(IH):
            for X in range(IW):
                v = img[n][Y][X]
                if heat is not None:
                    h = heat['heat'][n]
                    HH, HW = h.shape

                    def q(i, j):
                        t = f32(h[i, j])
                        if math.isnan(t):
                            return 0
                        return int(np.rint(f32(min(max(t, f32(0)), f32(1))) * f32(255)))

                    def taps(P, I, H):
                        f = max((2 * P + 1) * H - I, 0) * 128 // I
                        i0 = min(f >> 8, H - 1)
                        return i0, min(i0 + 1, H - 1), f & 255
                    x0, x1, wx = taps(X, IW, HW)
                    y0, y1, wy = taps(Y, IH, HH)
                    a = (q(y0, x0) * (256 - wx) * (256 - wy) + q(y0, x1) * wx * (256 - wy) + q(y1, x0) * (256 - wx) * wy + q(y1, x1) * wx * wy + 32768) >> 16
                    alpha = (a * heat['amax'] + 127) // 255
                    v = [(v[c] * (255 - alpha) + heat['color'][c] * alpha + 127) // 255 for c in range(3)]
                if inset is not None:
                    p, z = inset['inset'][n], inset['zoom']
                    dx, dy = X - inset['x0'], Y - inset['y0']
                    if 0 <= dx < z * p.shape[1] and 0 <= dy < z * p.shape[0]:
                        j = dx // z
                        v = [int(c) for c in p[dy // z, p.shape[1] - 1 - j if inset['mirror'] else j]]
                if markers is not None:
                    for m, (r_fill, r_out, c_fill, c_out) in enumerate(markers['table']):
                        cx, cy = markers['centres'][n, m]
                        if markers.get('valid') is not None and not markers['valid'][n, m]:
                            continue
                        if not (math.isfinite(cx) and math.isfinite(cy)):
                            continue
                        with np.errstate(over='ignore'):
                            qx = np.rint(f32(f32(cx) * f32(markers['sx'])) * f32(8))
                            qy = np.rint(f32(f32(cy) * f32(markers['sy'])) * f32(8))
                        if not (abs(qx) <= 2 ** 20 and abs(qy) <= 2 ** 20):
                            continue
                        qx, qy = int(qx), int(qy)
                        for r, col in ([(r_out, c_out)] if r_out > 0 else []) + [(r_fill, c_fill)]:
                            cnt = sum(1 for i in range(4) for j in range(4)
                                      if (8 * X + 2 * i + 1 - qx) ** 2 + (8 * Y + 2 * j + 1 - qy) ** 2 <= 64 * r * r)
                            ch = ((col >> 16) & 255, (col >> 8) & 255, col & 255)
                            v = [(v[c] * (16 - cnt) + ch[c] * cnt + 8) >> 4 for c in range(3)]
                img[n][Y][X] = v
    out = np.array(img, dtype=np.uint8)
    if out_fmt == 'rgb':
        return out
    if out_fmt == 'bgr':
        return out[..., ::-1].copy()
    y0, *rows = oref.FORWARD[matrix]
    Ks = [[int(math.copysign(math.floor(abs(c) * 2.0 ** 20 + 0.5), c)) for c in row] for row in rows]
    conv = lambda k, off, p: min(max((k[0] * p[0] + k[1] * p[1] + k[2] * p[2] + (off << 20) + (1 << 19)) >> 20, 0), 255)
    Yp = np.zeros((N, IH, IW), dtype=np.uint8)
    U, V = np.zeros((N, IH // 2, IW // 2), dtype=np.uint8), np.zeros((N, IH // 2, IW // 2), dtype=np.uint8)
    for n in range(N):
        for Y in range(IH):
            for X in range(IW):
                Yp[n, Y, X] = conv(Ks[0], y0, img[n][Y][X])
        for by in range(IH // 2):
            for bx in range(IW // 2):
                blk = [img[n][2 * by + i][2 * bx + j] for i in range(2) for j in range(2)]
                mean = [(sum(p[c] for p in blk) + 2) >> 2 for c in range(3)]
                U[n, by, bx], V[n, by, bx] = conv(Ks[1], 128, mean), conv(Ks[2], 128, mean)
    return pref.pack(Yp, U, V, out_fmt)


def layers(N, IH, IW, seed, M=3, heat_hw=(5, 7), inset_hw=(2, 3), zoom=2):
    rng = np.random.default_rng(seed)
    centres = (rng.random((N, M, 2)) * [IW, IH]).astype(np.float32)
    centres[0, 0] = (1.5625, 2.0625)                                      # q = 12.5 and 16.5: both on a tie of rint
    table = np.array([[2, 3, 0xb4b400, 0x000000], [1, 0, 0x00b400, 0xffffff], [3, 4, 0x2040c0, 0x101010]][:M], dtype=np.int32)
    valid = np.ones((N, M), dtype=np.uint8)
    valid[N - 1, M - 1] = 0
    heat = rng.random((N,) + heat_hw).astype(np.float32) * 1.4 - 0.2
    heat[0, 0, 0], heat[0, -1, -1] = np.nan, 2.0
    inset = rng.integers(0, 256, size=(N,) + inset_hw + (3,), dtype=np.uint8)
    return (dict(centres=centres, valid=valid, table=table, sx=1.0, sy=1.0), dict(heat=heat, color=(255, 32, 0), amax=200),
            dict(inset=inset, x0=IW - zoom * inset_hw[1], y0=IH - zoom * inset_hw[0], zoom=zoom, mirror=True))


@pytest.mark.parametrize('hw', [(6, 8), (18, 32)])
@pytest.mark.parametrize('fmt,out_fmt,matrix', [('rgb', 'rgb', 'bt601'), ('nv12', 'nv12', 'bt709'), ('yuyv', 'i420', 'jfif'), ('bgra', 'bgr', 'bt601')])
def test_the_contract_equals_a_per_pixel_evaluation(hw, fmt, out_fmt, matrix):
    N, (IH, IW) = 2, hw
    base = {'rgb': 'bgr', 'bgra': 'bgr'}.get(fmt, fmt)
    frames = pref.random_yuv_frames(base, N, IH, IW, seed=11, C=4 if fmt == 'bgra' else 3)
    markers, heat, inset = layers(N, IH, IW, seed=5)
    fv = np.array([1, 1], dtype=np.uint8)
    got = oref.render(frames, fmt, out_fmt, matrix, markers, heat, inset, fv)
    rgb = frames[..., :3] if fmt == 'rgb' else pref.to_rgb(frames, base, matrix)
    want = brute(rgb, out_fmt, matrix, markers, heat, inset, fv)
    assert got.dtype == np.uint8 and got.shape == oref.out_shape(out_fmt, N, IH, IW)
    assert np.array_equal(got, want)
    assert not np.array_equal(got, oref.render(frames, fmt, out_fmt, matrix))          # the layers do change the frame
    # each layer by itself, and a scale that is no power of two
    for kw in (dict(markers=dict(markers, sx=0.7, sy=1.3)), dict(heat=heat), dict(inset=inset)):
        assert np.array_equal(oref.render(frames, fmt, out_fmt, matrix, **kw), brute(rgb, out_fmt, matrix, **kw)), sorted(kw)


# ------------------------------------------------------------------------------------------------ the forward constants
def test_the_header_holds_the_forward_constants():
    text = open(os.path.join(REPO, 'eve_amd', 'csrc', 'yuv_rgb.h')).read()
    body = text[text.index('RGB_YUV_MATRICES[3]'):]
    rows = re.findall(r'^\s*\{(\d+), \{(-?\d+), (-?\d+), (-?\d+)\}, \{(-?\d+), (-?\d+), (-?\d+)\}, \{(-?\d+), (-?\d+), (-?\d+)\}\},', body, re.M)
    assert len(rows) == 3
    for row, name in zip(rows, ('bt601', 'bt709', 'jfif')):                # the order of EVE_YUV_*
        assert kernels.YUV_MATRICES[name] == ('bt601', 'bt709', 'jfif').index(name)
        y0, ky, ku, kv = oref.forward_constants(name)
        assert [int(v) for v in row] == [y0, *ky, *ku, *kv], name
        want = [int(math.copysign(math.floor(abs(c) * 2.0 ** 20 + 0.5), c)) for r in oref.FORWARD[name][1:] for c in r]
        assert [*ky, *ku, *kv] == want


@pytest.mark.parametrize('matrix,bound', [('bt601', (2, 1, 2)), ('bt709', (2, 1, 2)), ('jfif', (1, 1, 1))])
def test_the_round_trip_stays_within_its_bounds(matrix, bound):
    """RGB -> YUV (per pixel, 4:4:4) -> RGB by pixel_format_ref.yuv_to_rgb over the stride-3 lattice 0, 3, ..., 255 of every channel:
    off by at most (2, 1, 2) under the limited-range matrices and (1, 1, 1) under jfif (the same bounds hold over all 2^24 colours)."""
    axis = np.arange(0, 256, 3)
    assert axis[0] == 0 and axis[-1] == 255
    rgb = np.stack(np.meshgrid(axis, axis, axis, indexing='ij'), axis=-1).reshape(-1, 3).astype(np.uint8)
    back = pref.yuv_to_rgb(*oref.rgb_to_yuv(rgb, matrix), matrix)
    err = np.abs(back.astype(np.int64) - rgb.astype(np.int64)).max(axis=0)
    print(matrix, 'round trip error (R, G, B):', tuple(err))
    assert (err <= np.array(bound)).all(), (matrix, tuple(err))


# ------------------------------------------------------------------------------------------------ exactly known results
def test_constant_frames_have_exactly_known_results():
    N, IH, IW = 2, 16, 24
    frames = np.full((N, IH, IW, 3), (10, 200, 90), dtype=np.uint8)
    table = np.array([[3, 0, 0x123456, 0]], dtype=np.int32)
    centres = np.tile(np.array([[[12.5, 8.5]]], dtype=np.float32), (N, 1, 1))        # the centre of pixel (12, 8)
    got = oref.render(frames, 'rgb', 'rgb', markers=dict(centres=centres, table=table, valid=None, sx=1.0, sy=1.0))
    assert tuple(got[0, 8, 12]) == (0x12, 0x34, 0x56) and tuple(got[1, 9, 13]) == (0x12, 0x34, 0x56)       # n = 16: exactly the colour
    assert oref.coverage(IH, IW, 100, 68, 3)[8, 12] == 16 and oref.coverage(IH, IW, 100, 68, 3)[0, 0] == 0
    assert tuple(got[0, 0, 0]) == (10, 200, 90) and tuple(got[0, 8, 20]) == (10, 200, 90)
    edge = got[0, 8, 15]                                                               # the disc's rim: a blend, not either colour
    assert tuple(edge) != (10, 200, 90) and tuple(edge) != (0x12, 0x34, 0x56)
    heat = np.full((N, 4, 4), 0.75, dtype=np.float32)
    assert np.array_equal(oref.render(frames, 'rgb', 'rgb', heat=dict(heat=heat, color=(255, 0, 0), amax=0)), frames)
    assert np.array_equal(oref.render(frames, 'rgb', 'rgb', heat=dict(heat=heat * 0, color=(255, 0, 0), amax=255)), frames)
    full = oref.render(frames, 'rgb', 'rgb', heat=dict(heat=heat * 2, color=(255, 1, 2), amax=255))
    assert (full == np.array([255, 1, 2], dtype=np.uint8)).all()                       # q = 255 everywhere, alpha = 255: the colour
    assert (oref.quantise_heat(np.array([np.nan, -1, 0.5, 2, 0.1], dtype=np.float32)) == [0, 0, 128, 255, 26]).all()    # rint(127.5) = 128, rint(25.5) = 26: ties to even
    # frame_valid = 0: the converted capture alone
    markers, heat_l, inset = layers(N, IH, IW, seed=2)
    nv12 = pref.random_yuv_frames('nv12', N, IH, IW, seed=3)
    got = oref.render(nv12, 'nv12', 'bgr', 'bt709', markers, heat_l, inset, frame_valid=np.array([0, 1], dtype=np.uint8))
    assert np.array_equal(got[0], pref.to_rgb(nv12, 'nv12', 'bt709')[0, ..., ::-1])
    assert np.array_equal(got[1], oref.render(nv12, 'nv12', 'bgr', 'bt709', markers, heat_l, inset)[1])
    # no layer at all: pure conversion, and for same-format RGB the input bytes
    assert np.array_equal(oref.render(frames, 'rgb', 'rgb'), frames)
    assert np.array_equal(oref.render(nv12, 'nv12', 'rgb', 'jfif'), pref.to_rgb(nv12, 'nv12', 'jfif'))


def test_markers_that_are_not_drawn():
    frames = np.zeros((1, 8, 8, 3), dtype=np.uint8)
    table = np.array([[2, 3, 0xffffff, 0x808080]] * 5, dtype=np.int32)
    c = np.array([[[np.nan, 4], [4, np.inf], [4, 4], [140000.0, 4], [131072.0, 4]]], dtype=np.float32)
    q, ok = oref.quantise_centres(c, 1.0, 1.0)
    assert list(ok[0]) == [False, False, True, False, True]               # |q| = 2^20 is still drawn (nowhere near the frame)
    valid = np.array([[1, 1, 0, 1, 1]], dtype=np.uint8)
    assert not oref.render(frames, 'rgb', 'rgb', markers=dict(centres=c, table=table, valid=valid, sx=1.0, sy=1.0)).any()
    assert oref.render(frames, 'rgb', 'rgb', markers=dict(centres=c, table=table, valid=None, sx=1.0, sy=1.0)).any()
    q, ok = oref.quantise_centres(np.array([[[3.0e38, 1.0]]], dtype=np.float32), 4.0, 1.0)           # the product overflows: not drawn
    assert not ok.any()
    # ties go to even: 1.5625 * 8 = 12.5 -> 12, 2.0625 * 8 = 16.5 -> 16, 0.1875 * 8 = 1.5 -> 2
    q, _ = oref.quantise_centres(np.array([[[1.5625, 2.0625], [0.1875, -0.0625]]], dtype=np.float32), 1.0, 1.0)
    assert q.tolist() == [[[12.0, 16.0], [2.0, -0.0]]]


def test_the_layer_order():
    N, IH, IW = 1, 12, 16
    frames = np.full((N, IH, IW, 3), 50, dtype=np.uint8)
    inset = dict(inset=np.full((N, 6, 6, 3), 200, dtype=np.uint8), x0=4, y0=4, zoom=1, mirror=False)
    heat = dict(heat=np.ones((N, 3, 3), dtype=np.float32), color=(255, 0, 0), amax=255)
    first = [3, 0, 0xff0000, 0]
    second = [1, 0, 0x0000ff, 0]
    centres = np.array([[[6.5, 6.5], [6.5, 6.5]]], dtype=np.float32)
    both = lambda t: oref.render(frames, 'rgb', 'rgb', heat=heat, inset=inset,
                                 markers=dict(centres=centres, table=np.array(t, dtype=np.int32), valid=None, sx=1.0, sy=1.0))
    got = both([first, second])
    assert tuple(got[0, 0, 0]) == (255, 0, 0)                              # the heat covers the capture
    assert tuple(got[0, 9, 9]) == (200, 200, 200)                          # the inset is opaque: no heat shows through
    assert tuple(got[0, 6, 6]) == (0, 0, 255)                              # the marker listed later lies on top, both on top of the inset
    assert tuple(got[0, 6, 8]) == (255, 0, 0)                              # ... and where only the first reaches, it covers the inset
    assert tuple(both([second, first])[0, 6, 6]) == (255, 0, 0)
    ring = oref.render(frames, 'rgb', 'rgb', markers=dict(centres=centres[:, :1], table=np.array([[1, 3, 0x00ff00, 0x000000]], dtype=np.int32),
                                                         valid=None, sx=1.0, sy=1.0))
    assert tuple(ring[0, 6, 6]) == (0, 255, 0) and tuple(ring[0, 6, 8]) == (0, 0, 0)        # the outline first, the fill disc over it
    mirrored = np.arange(N * 2 * 3 * 3, dtype=np.uint8).reshape(N, 2, 3, 3)
    got = oref.render(frames, 'rgb', 'rgb', inset=dict(inset=mirrored, x0=10, y0=8, zoom=2, mirror=True))
    assert np.array_equal(got[0, 8:12, 10:16], np.repeat(np.repeat(mirrored[0, :, ::-1], 2, axis=0), 2, axis=1))


# ------------------------------------------------------------------------------------------------ the wrapper's refusals
def test_the_wrapper_refuses_what_the_contract_does_not_define(fake):
    N, IH, IW = 2, 8, 16
    rgb = torch.zeros((N, IH, IW, 3), dtype=torch.uint8)
    nv12 = torch.zeros((N, IH * 3 // 2, IW), dtype=torch.uint8)
    centres = torch.zeros((N, 2, 2))
    table = torch.tensor([[1, 2, 0, 0]] * 2, dtype=torch.int32)
    heat = torch.zeros((N, 3, 4))
    inset = torch.zeros((N, 2, 4, 3), dtype=torch.uint8)
    ok = fake.overlay_render(rgb, 'rgb', 'nv12', centres=centres, marker_table=table, heat=heat, inset=inset, inset_xy=(8, 4), zoom=2,
                             frame_valid=torch.ones(N, dtype=torch.uint8))
    assert tuple(ok.shape) == (N, IH * 3 // 2, IW) and ok.dtype == torch.uint8
    assert tuple(fake.overlay_render(nv12, 'nv12', 'bgr').shape) == (N, IH, IW, 3)
    assert tuple(fake.overlay_render(torch.zeros((N, IH, IW, 4), dtype=torch.uint8), 'bgra', 'rgb').shape) == (N, IH, IW, 3)
    odd = torch.zeros((N, 7, 15, 3), dtype=torch.uint8)
    assert tuple(fake.overlay_render(odd, 'rgb', 'bgr').shape) == (N, 7, 15, 3)         # odd sizes are fine between RGB formats
    cases = {
        'format': dict(format='nv21'), 'out_format': dict(out_format='yuyv'), 'matrix': dict(matrix='bt2020'),
        'frames': dict(frames=rgb.float()), 'frames must be contiguous': dict(frames=rgb.transpose(1, 2)),
        'frames of format rgba': dict(format='rgba'),
        'even IH and IW': dict(frames=odd, out_format='i420'),
        'come together': dict(centres=centres), 'at most 8': dict(centres=torch.zeros((N, 9, 2)), marker_table=torch.zeros((9, 4), dtype=torch.int32)),
        'marker_table': dict(centres=centres, marker_table=table.long()), 'centres': dict(centres=centres.double(), marker_table=table),
        'centres must': dict(centres=torch.zeros((N, 3, 2)), marker_table=table),
        'marker_valid': dict(centres=centres, marker_table=table, marker_valid=torch.ones((N, 2), dtype=torch.bool)),
        'marker_valid without': dict(marker_valid=torch.ones((N, 2), dtype=torch.uint8)),
        'sx and sy': dict(centres=centres, marker_table=table, sx=float('inf')),
        'heat must be at most': dict(heat=torch.zeros((N, 1025, 2))), 'heat must': dict(heat=heat.double()), 'heat ': dict(heat=heat[:1]),
        'amax': dict(heat=heat, amax=256), 'heat_color': dict(heat=heat, heat_color=(0, 0, 300)),
        'inset must': dict(inset=inset.float()), 'inset ': dict(inset=torch.zeros((N, 2, 4, 4), dtype=torch.uint8)),
        'zoom': dict(inset=inset, zoom=5), 'does not lie inside': dict(inset=inset, inset_xy=(13, 0)),
        'the inset rectangle': dict(inset=inset, inset_xy=(0, 5), zoom=2), 'inset rectangle': dict(inset=inset, inset_xy=(-1, 0)),
        'frame_valid': dict(frame_valid=torch.ones(N, dtype=torch.bool)), 'out must': dict(out=torch.zeros((N, IH, IW, 3), dtype=torch.uint8)),
    }
    for word, kw in cases.items():
        args = dict(dict(frames=rgb, format='rgb', out_format='nv12'), **kw)
        n = len(fake.calls)
        with pytest.raises(ValueError, match=re.escape(word.strip())):
            fake.overlay_render(**args)
        assert len(fake.calls) == n, word                                   # refused before any launch
    with pytest.raises(ValueError, match='yuyv frames need an even width'):
        fake.overlay_render(torch.zeros((N, 4, 5, 2), dtype=torch.uint8), 'yuyv', 'rgb')
    with pytest.raises(ValueError, match='IH and IW even'):
        fake.overlay_render(torch.zeros((N, 10, 6), dtype=torch.uint8), 'i420', 'rgb')


def test_render_overlay_is_the_contract(fake):
    N, IH, IW = 2, 18, 32
    markers, heat, inset = layers(N, IH, IW, seed=9)
    frames = pref.random_yuv_frames('i420', N, IH, IW, seed=4)
    t = torch.from_numpy
    got = render_overlay(t(frames), format='i420', out_format='nv12', matrix='bt709',
                         markers=dict(centres=t(markers['centres']), table=markers['table'].tolist(), valid=t(markers['valid']), sx=0.5, sy=2.0),
                         heat=dict(heat=t(heat['heat']), color=heat['color'], amax=heat['amax']),
                         inset=dict(inset=t(inset['inset']), zoom=2, mirror=True), frame_valid=t(np.array([1, 0], dtype=np.uint8)))
    want = oref.render(frames, 'i420', 'nv12', 'bt709', dict(markers, sx=0.5, sy=2.0), heat, inset, np.array([1, 0]))
    assert np.array_equal(got.numpy(), want) and fake.last_overlay['inset_xy'] == (IW - 6, IH - 4)      # flush in the bottom-right corner
    plain = render_overlay(t(frames), format='i420', out_format='rgb', heat=t(heat['heat']), inset=t(inset['inset']))
    assert np.array_equal(plain.numpy(), oref.render(frames, 'i420', 'rgb', 'bt601', None, dict(heat=heat['heat'], color=(255, 0, 0), amax=128),
                                                     dict(inset=inset['inset'], x0=IW - 3, y0=IH - 2, zoom=1, mirror=False)))
    for bad in (dict(markers=dict(centres=t(markers['centres']))), dict(heat=dict(color=(1, 2, 3))), dict(inset=dict(zoom=2)),
                dict(markers=dict(centres=t(markers['centres']), table=[[1, 2, 3, 4]], radius=3))):
        with pytest.raises(ValueError):
            render_overlay(t(frames), format='i420', **bad)


# ------------------------------------------------------------------------------------------------ EVEStream plumbing
def spec_of(**kw):
    return OverlaySpec(**dict(dict(markers=[dict(key='PoG_px_initial', fill=(180, 180, 0), r_fill=3, r_outline=5),
                                           dict(key='PoG_px_final', fill=(0, 180, 0), r_fill=3, r_outline=5)], heat=True, inset='eyes'), **kw))


def stream_chunk(B, Tc, fmt='nv12', seed=3):
    batch = {k_: v for k_, v in clip(B, Tc, seed=seed).items() if k_ != 'screen_frame'}
    key = 'screen_frame' if fmt == 'rgb' else 'screen_frame_' + fmt
    cap = capture('bgr', B, Tc, seed=1) if fmt == 'rgb' else capture(fmt, B, Tc, seed=1)
    return dict(chunk_of(batch, 0, Tc), **{key: cap})


def expected(chunk, out, spec, fmt, model, frame_valid=None, matrix='bt601'):
    """overlay_ref on the capture and THE STEP'S OWN results."""
    key = 'screen_frame' if fmt == 'rgb' else 'screen_frame_' + fmt
    cap = chunk[key]
    B, Tc = cap.shape[:2]
    N = B * Tc
    IH, IW = CAPTURE
    flat = cap.reshape((N,) + tuple(cap.shape[2:])).numpy()
    src = dict(chunk, **out)
    table = np.array(spec.marker_table(), dtype=np.int32).reshape(-1, 4)
    markers = None
    if spec.markers:
        valid = None
        if any(m[1] for m in spec.markers):
            valid = np.stack([np.ones(N, dtype=np.uint8) if m[1] is None else (src[m[1]].reshape(N).numpy() != 0).astype(np.uint8) for m in spec.markers], axis=1)
        markers = dict(centres=np.stack([src[m[0]].reshape(N, 2).numpy() for m in spec.markers], axis=1), table=table, valid=valid,
                       sx=np.float32(IW / 1920.0), sy=np.float32(IH / 1080.0))
    heat = None
    if spec.heat:
        hm = out['heatmap_final']
        heat = dict(heat=hm.reshape((N,) + tuple(hm.shape[-2:])).float().numpy(), color=spec.heat_color, amax=spec.heat_amax)
    inset = None
    if spec.inset == 'eyes':
        q = lambda p: (p[..., :3] if p.dtype == torch.uint8 else quantise_patches(p))
        left, right = q(chunk['left_eye_patch']), q(chunk['right_eye_patch'])
        eyes = torch.cat([right, left], dim=3).reshape((N,) + (left.shape[2], 2 * left.shape[3], 3)).numpy()
        z = spec.inset_zoom
        inset = dict(inset=eyes, x0=IW - z * eyes.shape[2], y0=IH - z * eyes.shape[1], zoom=z, mirror=spec.inset_mirror)
    res = oref.render(flat, fmt, spec.out_format, matrix, markers, heat, inset, frame_valid)
    return res.reshape((B, Tc) + res.shape[1:])


@pytest.mark.parametrize('out_format', ['nv12', 'i420', 'rgb', 'bgr'])
def test_stream_renders_its_own_results(fake, out_format):
    B, Tc = 2, 2
    model = make_model(*CONFIGS['gru-cgru'])
    stream = eve_amd.EVEStream(model, B, use_graph=False)
    ch = stream_chunk(B, Tc)
    spec = spec_of(out_format=out_format)
    out = stream.step(ch, render=spec, return_heatmaps=True)
    IH, IW = CAPTURE
    want_shape = (B, Tc, IH, IW, 3) if out_format in ('rgb', 'bgr') else (B, Tc, IH * 3 // 2, IW)
    assert out['rendered'].dtype == torch.uint8 and tuple(out['rendered'].shape) == want_shape
    assert fake.calls.count('overlay_render') == 1
    assert fake.last_overlay['frame_valid'] is None and fake.last_overlay['format'] == 'nv12'
    assert fake.last_overlay['frames'].data_ptr() == ch['screen_frame_nv12'].data_ptr()                 # the capture where it lies: no copy
    assert (fake.last_overlay['sx'], fake.last_overlay['sy']) == (IW / 1920.0, IH / 1080.0)
    want = expected(ch, out, spec, 'nv12', model)
    assert np.array_equal(out['rendered'].numpy(), want)
    bare = oref.render(ch['screen_frame_nv12'].reshape((B * Tc,) + tuple(ch['screen_frame_nv12'].shape[2:])).numpy(), 'nv12', out_format)
    assert not np.array_equal(want.reshape(bare.shape), bare)
    # the heat map is this step's whether it is returned or not, and the other results are the unrendered step's
    stream2 = eve_amd.EVEStream(model, B, use_graph=False)
    plain = stream2.step(ch)
    stream3 = eve_amd.EVEStream(model, B, use_graph=False)
    again = stream3.step(ch, render=spec)
    assert 'heatmap_final' not in again and 'rendered' not in plain
    assert torch.equal(again['rendered'], out['rendered'])
    for key in plain:
        assert torch.equal(plain[key], again[key]), key


def test_stream_hands_valid_to_the_launch(fake):
    B, Tc = 2, 2
    model = make_model(*CONFIGS['gru-cgru'])
    ch = stream_chunk(B, Tc)
    ch['PoG_px_gt'] = torch.tensor([[[100.0, 200.0], [900.5, 500.25]], [[1919.0, 1079.0], [float('nan'), 3.0]]])
    ch['gt_ok'] = torch.tensor([[True, True], [False, True]])
    spec = spec_of(markers=[dict(key='PoG_px_gt', valid='gt_ok', r_fill=4, r_outline=0, fill=0x0000ff), dict(key='PoG_px_final')],
                   inset=None, matrix='bt709', out_format='rgb')
    stream = eve_amd.EVEStream(model, B, use_graph=False)
    out = stream.step(ch, lengths=[1, 2], render=spec, return_heatmaps=True)
    assert fake.last_overlay['frame_valid'].tolist() == [1, 0, 1, 1] and out['valid'].tolist() == [[True, False], [True, True]]
    assert fake.last_overlay['matrix'] == 'bt709'                            # the spec's matrix; None takes the capture's
    want = expected(ch, out, spec, 'nv12', model, frame_valid=np.array([1, 0, 1, 1]), matrix='bt709')
    assert np.array_equal(out['rendered'].numpy(), want)
    bare = pref.to_rgb(ch['screen_frame_nv12'][0, 1:2].numpy(), 'nv12', 'bt709')
    assert np.array_equal(out['rendered'][0, 1].numpy(), bare[0])            # stream 0's second frame: the bare converted capture
    # masked: the step's valid
    stream = eve_amd.EVEStream(model, B, use_graph=False)
    mask = np.ones((B, Tc, 2), dtype=bool)
    mask[1, 0] = False
    out = stream.step(ch, eye_mask=mask, render=spec)
    assert fake.last_overlay['frame_valid'].tolist() == [1, 1, 0, 1] and out['valid'].tolist() == [[True, True], [False, True]]
    model.refine_net.yuv_matrix = 'jfif'
    eve_amd.EVEStream(model, B, use_graph=False).step(ch, render=spec_of(inset=None, heat=False))
    assert fake.last_overlay['matrix'] == 'jfif'


@pytest.mark.parametrize('fmt', ['rgb', 'bgr', 'i420', 'yuyv'])
def test_stream_renders_every_capture_key(fake, fmt):
    B, Tc = 1, 2
    model = make_model(*CONFIGS['gru-cgru'])
    ch = stream_chunk(B, Tc, fmt)
    g = torch.Generator().manual_seed(5)
    for side in ('left', 'right'):                                                        # a uint8 patch chunk is used as it is
        ch[side + '_eye_patch'] = torch.randint(0, 256, (B, Tc, 64, 64, 3), generator=g, dtype=torch.uint8)
    spec = spec_of(inset_zoom=2, heat=False, out_format='rgb')
    out = eve_amd.EVEStream(model, B, use_graph=False).step(ch, render=spec)
    assert fake.last_overlay['format'] == fmt
    want = expected(ch, out, spec, fmt, model)
    assert np.array_equal(out['rendered'].numpy(), want)
    eyes = torch.cat([ch['right_eye_patch'], ch['left_eye_patch']], dim=3)[0, 1].numpy()[:, ::-1]      # [right | left], mirrored
    region = out['rendered'][0, 1].numpy()[-128:, -256:]
    zoomed = np.repeat(np.repeat(eyes, 2, axis=0), 2, axis=1)
    far = np.ones((128, 256), dtype=bool)                                                  # (away from where a marker may lie on the inset)
    for m in ('PoG_px_initial', 'PoG_px_final'):
        x, y = out[m][0, 1].numpy() * [256 / 1920.0, 144 / 1080.0] - [0, 16]
        yy, xx = np.mgrid[0:128, 0:256]
        far &= (xx - x) ** 2 + (yy - y) ** 2 > 8 ** 2
    assert far.any() and np.array_equal(region[far], zoomed[far])


def test_the_graph_key_holds_the_spec(fake):
    model = make_model(*CONFIGS['gru-cgru'])
    ch = stream_chunk(2, 2)
    stream = eve_amd.EVEStream(model, 2, use_graph=False)
    captured = []
    stream._capture = lambda chunk, *a, **k_: captured.append(a[-1]) or {'n': len(captured)}
    plan = lambda spec: stream._render_plan(ch, spec)
    bare = stream._graph_for(ch, False)
    first = stream._graph_for(ch, False, False, False, plan(spec_of()))
    assert first is not bare and captured[0] is None and captured[1]['spec'] == spec_of()
    assert stream._graph_for(dict(ch), False, False, False, plan(spec_of())) is first             # an equal spec: the same graph
    other = stream._graph_for(ch, False, False, False, plan(spec_of(heat_amax=64)))
    assert other is not first and len(stream._graphs) == 3
    assert stream._graph_for(ch, False) is bare and len(captured) == 3
    assert spec_of() == spec_of() and hash(spec_of()) == hash(spec_of()) and spec_of() != spec_of(out_format='i420')
    assert stream._graph_key(ch, False, False, False, plan(spec_of())) != stream._graph_key(ch, False, False, False, plan(spec_of(inset_mirror=False)))
    assert plan(spec_of())['table'] is plan(spec_of())['table']                                     # made once, before any capture


def test_the_default_spec_is_the_reference_look():
    spec = OverlaySpec()
    assert spec.out_format == 'nv12' and spec.inset == 'eyes' and spec.inset_mirror and not spec.heat and spec.inset_xy is None
    assert spec.marker_table() == [[10, 14, (180 << 16) | (180 << 8), 0], [10, 14, 180 << 8, 0]]
    assert [m[0] for m in spec.markers] == ['PoG_px_initial', 'PoG_px_final']
    for bad in (dict(out_format='yuyv'), dict(matrix='bt2020'), dict(markers=[dict(key='a')] * 9), dict(markers=[dict(r_fill=3)]),
                dict(markers=[dict(key='a', r_fill=256)]), dict(markers=[dict(key='a', fill=(0, 0, 256))]), dict(heat_amax=300),
                dict(inset=3), dict(inset_zoom=0), dict(markers=[dict(key='a', colour=1)])):
        with pytest.raises(ValueError):
            OverlaySpec(**bad)


def test_stream_refuses_what_it_cannot_render(fake):
    B, Tc = 2, 2
    model = make_model(*CONFIGS['gru-cgru'])
    stream = eve_amd.EVEStream(model, B, use_graph=False)
    full = clip(B, Tc, seed=3)
    ch = stream_chunk(B, Tc)
    n = len(fake.calls)
    with pytest.raises(ValueError, match='capture is needed|needs a full-resolution uint8 capture'):
        stream.step(chunk_of(full, 0, Tc), render=spec_of())                                       # the float 72 x 128 screen_frame
    small = dict(ch)
    del small['screen_frame_nv12']
    with pytest.raises(ValueError, match='needs a full-resolution uint8 capture'):
        stream.step(dict(small, screen_frame=torch.zeros((B, Tc, 72, 128, 3), dtype=torch.uint8)), render=spec_of())
    with pytest.raises(ValueError, match='holds none'):
        stream.step(small, render=spec_of())
    with pytest.raises(ValueError, match='OverlaySpec'):
        stream.step(ch, render=dict(out_format='nv12'))
    with pytest.raises(ValueError, match='marker key'):
        stream.step(ch, render=spec_of(markers=[dict(key='PoG_px_gt')]))
    with pytest.raises(ValueError, match='inset'):
        stream.step(ch, render=spec_of(inset='thumbnail'))
    with pytest.raises(ValueError, match='does not lie inside'):
        stream.step(ch, render=spec_of(inset_zoom=3))                                              # 192 x 384 of eyes on 144 x 256
    with pytest.raises(ValueError, match='does not lie inside'):
        stream.step(ch, render=spec_of(inset_xy=(200, 0)))
    with pytest.raises(ValueError, match='even size'):
        stream.step(dict(small, screen_frame=torch.zeros((B, Tc, 145, 255, 3), dtype=torch.uint8)), render=spec_of())
    assert len(fake.calls) == n                                                                    # refused before any kernel call
    eye_only = eve_amd.EVEStream(make_eye_only(), B, use_graph=False)
    with pytest.raises(ValueError, match='RefineNet'):
        eye_only.step(ch, render=spec_of(heat=False))
    with pytest.raises(ValueError, match='RefineNet'):
        eye_only.step(ch, render=spec_of(markers=[dict(key='PoG_px_initial')]))                    # heat=True


def make_eye_only():
    model = make_model(*CONFIGS['gru-cgru'])
    model.refine_net = None
    return model
