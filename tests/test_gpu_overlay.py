"""GPU: eve_overlay_render (csrc/overlay.hip) bit for bit against its contract in numpy (tests/overlay_ref.py), through the raw C
ABI into an output with a guard of sentinel bytes behind it, in the vector and the byte form, for every input and output format;
and EVEStream.step(chunk, render=spec) under graph replay against the contract applied to the capture and the step's own results.

Frames: uniform random bytes.  For the YUV captures their conversion holds 0 and 255 in every channel (both clamps of the inverse
conversion act: asserted, the seeds searched on the CPU).  The forward conversion's clamps cannot act on 8-bit RGB under bt601 and
bt709 (Y stays in 16..235, U and V in 16..240) and only at the top under jfif, where pure blue gives U = 256 and pure red V = 256
before the clamp and the smallest value is 1: test_the_forward_clamp_acts_under_jfif holds that one case.
No test here provokes a fault: the markers centred outside the frame are ordinary inputs the contract defines."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import eve_amd
import overlay_ref as oref
import pixel_format_ref as pref
import screen_format_ref as fref
from eve_amd.data import OverlaySpec, quantise_patches, render_overlay
from eve_amd.kernels import OVERLAY_IN_FORMATS, OVERLAY_OUT_FORMATS, YUV_MATRICES, default_kernels
from test_gpu_pixel_formats import both_forms
from test_gpu_stream import gpu_clip, make_model

pytestmark = pytest.mark.gpu
GUARD = 4096                  # bytes behind the output that no launch may touch
SENTINEL = 0xA5
YUV_IN = ('nv12', 'i420', 'yuyv')
# random_yuv_frames seeds whose converted frames hold 0 and 255 in every channel, per (format, N, IH, IW); every other shape: seed 0
SEEDS = {('nv12', 3, 2, 2): 1, ('i420', 3, 2, 2): 1, ('yuyv', 3, 2, 2): 3}


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def random_frames(fmt, N, IH, IW, matrix='bt601', seed=None):
    """Uniform bytes in the layout of fmt ('rgb' / 'bgr' / 'rgba' / 'bgra' included)."""
    base = {'rgb': 'bgr', 'rgba': 'bgr', 'bgra': 'bgr'}.get(fmt, fmt)
    seed = SEEDS.get((fmt, N, IH, IW), 0) if seed is None else seed
    buf = pref.random_yuv_frames(base, N, IH, IW, seed, C=4 if fmt in ('rgba', 'bgra') else 3)
    if fmt in YUV_IN:
        assert fref.both_clamps(buf, fmt, matrix), (fmt, N, IH, IW, matrix)
    return buf


def gpu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def raw_call(k, fmt, out_fmt, matrix, frames, out, IH, IW, markers=None, heat=None, inset=None, frame_valid=None):
    """The C entry point on GPU tensors; the layers as overlay_ref takes them (numpy)."""
    N = frames.shape[0]
    keep = []                                              # the device copies live until the call has been issued

    def dev(a, dtype):
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()
        keep.append(t)
        return t
    M, centres, valid, table, sx, sy = 0, None, None, None, 1.0, 1.0
    if markers is not None:
        table = dev(markers['table'], np.int32)
        M = table.shape[0]
        centres = dev(markers['centres'], np.float32)
        valid = None if markers.get('valid') is None else dev(markers['valid'], np.uint8)
        sx, sy = float(markers.get('sx', 1.0)), float(markers.get('sy', 1.0))
    h, HH, HW, color, amax = None, 0, 0, 0, 0
    if heat is not None:
        h = dev(heat['heat'], np.float32)
        HH, HW = h.shape[1:]
        color, amax = (heat['color'][0] << 16) | (heat['color'][1] << 8) | heat['color'][2], heat['amax']
    p, ih, iw, x0, y0, zoom, mirror = None, 0, 0, 0, 0, 1, 0
    if inset is not None:
        p = dev(inset['inset'], np.uint8)
        ih, iw = p.shape[1:3]
        x0, y0, zoom, mirror = inset['x0'], inset['y0'], inset['zoom'], int(inset['mirror'])
    fv = None if frame_valid is None else dev(frame_valid, np.uint8)
    rc = k.lib.eve_overlay_render(OVERLAY_IN_FORMATS[fmt], OVERLAY_OUT_FORMATS[out_fmt], YUV_MATRICES[matrix], N, IH, IW, ptr(frames), ptr(out),
                                  M, ptr(centres), ptr(valid), ptr(table), sx, sy, ptr(h), HH, HW, color, amax, ptr(p), ih, iw, x0, y0, zoom,
                                  mirror, ptr(fv), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def check(k, buf, fmt, out_fmt, hw, vec, matrix='bt601', **layers):
    """Two launches into a guarded buffer, each == the numpy contract exactly; the guard untouched; the kernel's name.  -> want"""
    N, (IH, IW) = buf.shape[0], hw
    want = oref.render(buf, fmt, out_fmt, matrix, layers.get('markers'), layers.get('heat'), layers.get('inset'), layers.get('frame_valid'))
    n_out = want.size
    frames = gpu(buf)
    name = ('overlay_kernel<%s,%s,%s>' % (fmt, out_fmt, 'true' if vec else 'false')).encode()
    for _ in range(2):
        out = torch.full((n_out + GUARD,), SENTINEL, dtype=torch.uint8, device='cuda')
        assert raw_call(k, fmt, out_fmt, matrix, frames, out, IH, IW, **layers) == 0, k.lib.eve_last_error()
        assert k.lib.eve_last_kernel() == name, k.lib.eve_last_kernel()
        got = out.cpu().numpy()
        assert (got[n_out:] == SENTINEL).all(), 'guard overwritten'
        got = got[:n_out].reshape(want.shape)
        bad = got != want
        assert not bad.any(), ('%d of %d bytes differ, first at %s: got %d want %d' % (
            int(bad.sum()), n_out, tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0]))
    return want


def some_markers(N, IH, IW, M, seed, r=(2, 3)):
    """M overlapping markers per frame around the middle of the frame, each frame its own."""
    rng = np.random.default_rng(seed)
    centres = (np.array([IW, IH]) * (0.3 + 0.4 * rng.random((N, M, 2)))).astype(np.float32)
    table = np.array([[r[0] + m % 3, (r[1] + m % 4) * (m % 3 != 1), int(rng.integers(0, 1 << 24)), int(rng.integers(0, 1 << 24))] for m in range(M)], dtype=np.int32)
    return dict(centres=centres, valid=None, table=table, sx=1.0, sy=1.0)


def test_one_chroma_sample_under_an_off_frame_marker():
    """2 x 2, N = 3, NV12 out: a marker of radius 3 centred at (-1.25, 0.5), outside the frame, still covers its pixels."""
    k = default_kernels()
    N = 3
    markers = dict(centres=np.tile(np.array([[[-1.25, 0.5]]], dtype=np.float32), (N, 1, 1)), valid=None,
                   table=np.array([[3, 0, 0xff8000, 0]], dtype=np.int32), sx=1.0, sy=1.0)
    for fmt in ('nv12', 'rgb', 'yuyv'):
        buf = random_frames(fmt, N, 2, 2)
        want = check(k, buf, fmt, 'nv12', (2, 2), False, markers=markers)
        assert not np.array_equal(want, oref.render(buf, fmt, 'nv12'))


def test_the_byte_form_at_the_edges_and_on_ties():
    """10 x 12: centres exactly on a tie of rint, markers hanging over all four edges, a NaN centre and one with valid = 0."""
    k = default_kernels()
    N, IH, IW = 2, 10, 12
    c = np.array([[1.5625, 2.0625],                       # q = 12.5, 16.5: both ties, to even
                  [-0.5, 5.0], [6.0, -1.0], [12.4, 4.0], [5.0, 10.3],     # over the left, top, right and bottom edge
                  [np.nan, 3.0], [6.0, 6.0], [np.inf, 1.0]], dtype=np.float32)
    centres = np.tile(c[None], (N, 1, 1))
    centres[1, :, 0] += 0.1875
    valid = np.ones((N, 8), dtype=np.uint8)
    valid[:, 6] = 0
    table = np.array([[1, 2, 0xff0000, 0x00ff00], [2, 3, 0x0000ff, 0], [2, 0, 0xffff00, 0], [3, 3, 0x00ffff, 0x101010], [2, 4, 0xff00ff, 0xffffff],
                      [4, 5, 0xffffff, 0], [4, 5, 0xffffff, 0], [4, 5, 0xffffff, 0]], dtype=np.int32)
    markers = dict(centres=centres, valid=valid, table=table, sx=1.0, sy=1.0)
    q, ok = oref.quantise_centres(centres, 1.0, 1.0)
    assert q[0, 0].tolist() == [12.0, 16.0] and ok[0].tolist() == [True] * 5 + [False, True, False]
    for fmt, out_fmt in (('rgb', 'rgb'), ('nv12', 'i420'), ('yuyv', 'bgr'), ('bgra', 'nv12')):
        buf = random_frames(fmt, N, IH, IW)
        want = check(k, buf, fmt, out_fmt, (IH, IW), False, markers=markers)
        only5 = dict(markers, centres=centres[:, :5], valid=valid[:, :5], table=table[:5])
        assert np.array_equal(want, oref.render(buf, fmt, out_fmt, markers=only5))        # the last three draw nothing


def test_heat_quantisation_and_edge_clamps():
    """18 x 32, the vector form, a 5 x 7 heat map holding NaN, -1, 0.5 and 2: both clamps of the quantisation, and both edge clamps of
    the up-sampling (the first and last output pixels lie outside the heat cells' centres)."""
    k = default_kernels()
    N, IH, IW = 2, 18, 32
    heat = np.random.default_rng(3).random((N, 5, 7)).astype(np.float32)
    heat[0, 0, 0], heat[0, 0, 1], heat[0, 4, 6], heat[0, 2, 3] = np.nan, -1.0, 2.0, 0.5
    heat[1, 4, 0], heat[1, 0, 6] = np.nan, 2.0
    layer = dict(heat=heat, color=(255, 64, 0), amax=255)
    x0, x1, wx = oref._axis(IW, 7)
    y0, y1, wy = oref._axis(IH, 5)
    assert wx[0] == 0 and x0[0] == 0 and x0[-1] == 6 and x1[-1] == 6 and y0[0] == 0 and y1[-1] == 4 and (wx > 0).any() and (wy > 0).any()
    for fmt, out_fmt in (('rgb', 'rgb'), ('nv12', 'nv12'), ('i420', 'bgr')):
        buf = random_frames(fmt, N, IH, IW)
        want = check(k, buf, fmt, out_fmt, (IH, IW), True, heat=layer)
        assert not np.array_equal(want, oref.render(buf, fmt, out_fmt))
        check(k, buf, fmt, out_fmt, (IH, IW), True, heat=dict(layer, amax=0))
    check(k, random_frames('rgb', N, 10, 12), 'rgb', 'bgr', (10, 12), False, heat=layer)                 # the byte form reads the same taps


@pytest.mark.parametrize('out_fmt', list(OVERLAY_OUT_FORMATS))
@pytest.mark.parametrize('fmt', list(oref.IN_FORMATS))
def test_every_format_pair(fmt, out_fmt):
    """18 x 32, M = 8 overlapping markers, heat and a mirrored inset, in the vector form; all three matrices for one pair each."""
    k = default_kernels()
    N, IH, IW = 2, 18, 32
    markers = some_markers(N, IH, IW, 8, seed=7)
    heat = dict(heat=np.random.default_rng(5).random((N, 4, 6)).astype(np.float32), color=(0, 255, 32), amax=160)
    inset = dict(inset=np.random.default_rng(6).integers(0, 256, (N, 3, 5, 3), dtype=np.uint8), x0=IW - 15, y0=IH - 9, zoom=3, mirror=True)
    for matrix in (YUV_MATRICES if (fmt, out_fmt) in (('nv12', 'nv12'), ('yuyv', 'i420'), ('rgb', 'nv12'), ('i420', 'rgb')) else ('bt601',)):
        buf = random_frames(fmt, N, IH, IW, matrix)
        check(k, buf, fmt, out_fmt, (IH, IW), True, matrix, markers=markers, heat=heat, inset=inset, frame_valid=np.array([1, 1], dtype=np.uint8))
    check(k, buf, fmt, out_fmt, (IH, IW), True, markers=markers, heat=heat, inset=inset, frame_valid=np.array([0, 1], dtype=np.uint8))


def test_an_inset_flush_in_the_corner_under_a_marker():
    """36 x 64: an 8 x 16 inset at zoom 2, mirrored, flush in the bottom-right corner, a marker on top of it."""
    k = default_kernels()
    N, IH, IW = 2, 36, 64
    inset = dict(inset=np.random.default_rng(2).integers(0, 256, (N, 8, 16, 3), dtype=np.uint8), x0=IW - 32, y0=IH - 16, zoom=2, mirror=True)
    markers = dict(centres=np.array([[[50.0, 28.5]], [[63.5, 35.5]]], dtype=np.float32), valid=None, table=np.array([[4, 6, 0x00b400, 0]], dtype=np.int32),
                   sx=1.0, sy=1.0)
    for fmt, out_fmt in (('rgb', 'rgb'), ('nv12', 'nv12'), ('bgr', 'i420')):
        buf = random_frames(fmt, N, IH, IW)
        want = check(k, buf, fmt, out_fmt, (IH, IW), True, markers=markers, inset=inset)
        if out_fmt == 'rgb':
            zoomed = np.repeat(np.repeat(inset['inset'][0, :, ::-1], 2, axis=0), 2, axis=1)
            assert np.array_equal(want[0, -16:, -32:-20], zoomed[:, :12])                  # the inset, mirrored, left of the marker
            assert tuple(want[0, 28, 50]) == (0, 0xb4, 0)                                   # the marker on top of it
    for zoom in (1, 3, 4):
        small = dict(inset=inset['inset'][:, :, :15], x0=1, y0=2, zoom=zoom, mirror=False)
        check(k, random_frames('rgb', N, IH, IW), 'rgb', 'bgr', (IH, IW), True, inset=small)


def test_a_width_that_is_no_multiple_of_the_tile():
    """768 x 1366 RGB in to BGR out: the byte form, a last tile of six columns."""
    k = default_kernels()
    N, IH, IW = 1, 768, 1366
    markers = dict(centres=np.array([[[1364.0, 400.0], [683.0, 766.5]]], dtype=np.float32), valid=None,
                   table=np.array([[10, 14, 0xb4b400, 0], [10, 14, 0x00b400, 0]], dtype=np.int32), sx=1.0, sy=1.0)
    heat = dict(heat=np.random.default_rng(1).random((N, 9, 16)).astype(np.float32), color=(255, 0, 0), amax=128)
    check(k, random_frames('rgb', N, IH, IW), 'rgb', 'bgr', (IH, IW), False, markers=markers, heat=heat)


def test_the_real_case_1080p_nv12():
    """1080 x 1920, N = 2, NV12 in and out: the default look, a 72 x 128 heat map, the 128 x 256 eyes inset."""
    k = default_kernels()
    N, IH, IW = 2, 1080, 1920
    spec = OverlaySpec(heat=True)
    rng = np.random.default_rng(8)
    centres = np.array([[[960.0, 540.0], [1000.25, 560.5]], [[1800.0, 1000.0], [5.0, 3.0]]], dtype=np.float32)       # (one on the inset, one at a corner)
    markers = dict(centres=centres, valid=None, table=np.array(spec.marker_table(), dtype=np.int32), sx=1.0, sy=1.0)
    yy, xx = np.mgrid[0:72, 0:128]
    heat = np.stack([np.exp(-((xx - cx / 15.0) ** 2 + (yy - cy / 15.0) ** 2) / 18.0) for cx, cy in centres[:, 1]]).astype(np.float32)
    inset = dict(inset=rng.integers(0, 256, (N, 128, 256, 3), dtype=np.uint8), x0=IW - 256, y0=IH - 128, zoom=1, mirror=True)
    check(k, random_frames('nv12', N, IH, IW), 'nv12', 'nv12', (IH, IW), True,
          markers=markers, heat=dict(heat=heat, color=spec.heat_color, amax=spec.heat_amax), inset=inset)


def test_items_past_the_grid():
    """4 x 16, N = 2100: 4 200 (frame, row pair) items, past the grid's 4 096 workgroups: the grid-stride loop."""
    k = default_kernels()
    N, IH, IW = 2100, 4, 16
    markers = some_markers(N, IH, IW, 2, seed=4, r=(1, 1))
    fv = (np.arange(N) % 7 != 3).astype(np.uint8)
    check(k, random_frames('nv12', N, IH, IW), 'nv12', 'nv12', (IH, IW), True, markers=markers, frame_valid=fv)


@pytest.mark.parametrize('fmt', list(oref.IN_FORMATS))
def test_no_layer_is_pure_conversion(fmt):
    """M = 0, heat absent, inset absent: the converted capture; for same-format RGB the input bytes.  In both forms."""
    k = default_kernels()
    for (IH, IW), vec in (((18, 32), True), ((10, 12), False)):
        buf = random_frames(fmt, 3, IH, IW)
        rgb = oref.to_rgb(buf, fmt)
        assert np.array_equal(check(k, buf, fmt, 'rgb', (IH, IW), vec), rgb)
        assert np.array_equal(check(k, buf, fmt, 'bgr', (IH, IW), vec), rgb[..., ::-1])
        check(k, buf, fmt, 'nv12', (IH, IW), vec)
        if fmt == 'rgb':
            assert np.array_equal(check(k, buf, 'rgb', 'rgb', (IH, IW), vec), buf)
    odd = random_frames('rgb' if fmt in ('nv12', 'i420', 'yuyv') else fmt, 2, 7, 9)        # odd sizes between the RGB formats
    if fmt not in YUV_IN:
        check(k, odd, fmt, 'bgr', (7, 9), False)


def test_the_forward_clamp_acts_under_jfif():
    """Pure blue gives U = 256 and pure red V = 256 before the clamp under jfif: the only clamp the forward matrices can reach."""
    k = default_kernels()
    buf = np.zeros((2, 4, 8, 3), dtype=np.uint8)
    buf[0, ..., 2], buf[1, ..., 0] = 255, 255
    want = check(k, buf, 'rgb', 'i420', (4, 8), True, 'jfif')
    flat = want.reshape(2, -1)
    assert (flat[0, 32:40] == 255).all() and (flat[1, 40:48] == 255).all()
    y0, ky, ku, kv = oref.forward_constants('jfif')
    assert (ku[2] * 255 + (128 << 20) + (1 << 19)) >> 20 == 256 and (kv[0] * 255 + (128 << 20) + (1 << 19)) >> 20 == 256


def test_an_unaligned_base_takes_the_byte_form():
    k = default_kernels()
    N, IH, IW = 2, 18, 32
    buf = random_frames('nv12', N, IH, IW)
    want = oref.render(buf, 'nv12', 'nv12', markers=some_markers(N, IH, IW, 2, seed=1))
    big = torch.zeros((buf.size + 16,), dtype=torch.uint8, device='cuda')
    big[2:2 + buf.size] = gpu(buf).reshape(-1)
    out = torch.full((want.size + GUARD,), SENTINEL, dtype=torch.uint8, device='cuda')
    assert raw_call(k, 'nv12', 'nv12', 'bt601', big[2:2 + buf.size].view(buf.shape), out, IH, IW, markers=some_markers(N, IH, IW, 2, seed=1)) == 0
    assert k.lib.eve_last_kernel() == b'overlay_kernel<nv12,nv12,false>'
    got = out.cpu().numpy()
    assert np.array_equal(got[:want.size].reshape(want.shape), want) and (got[want.size:] == SENTINEL).all()


def test_the_library_refuses_without_a_launch():
    k = default_kernels()
    frames = torch.zeros((2 * 18 * 32 * 4,), dtype=torch.uint8, device='cuda')
    out = torch.full((2 * 18 * 32 * 3 + GUARD,), SENTINEL, dtype=torch.uint8, device='cuda')
    k.stream_state_rows(torch.zeros((2, 8), device='cuda'), torch.zeros((2, 8), device='cuda'))      # the last named launch
    before = k.lib.eve_last_kernel()
    assert b'overlay' not in before
    c = torch.zeros((2, 9, 2), device='cuda')
    t = torch.zeros((9, 4), dtype=torch.int32, device='cuda')
    h = torch.zeros((2, 4, 4), device='cuda')
    p = torch.zeros((2, 4, 4, 3), dtype=torch.uint8, device='cuda')
    F, O = OVERLAY_IN_FORMATS, OVERLAY_OUT_FORMATS
    S = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(fmt=F['rgb'], out_fmt=O['nv12'], matrix=0, N=2, IH=18, IW=32, src=frames, dst=out, M=0, centres=None, table=None, sx=1.0, sy=1.0,
             heat=None, HH=4, HW=4, color=0, amax=128, inset=None, ih=4, iw=4, x0=0, y0=0, zoom=1):
        return k.lib.eve_overlay_render(fmt, out_fmt, matrix, N, IH, IW, ptr(src), ptr(dst), M, ptr(centres), None, ptr(table), sx, sy, ptr(heat),
                                        HH, HW, color, amax, ptr(inset), ih, iw, x0, y0, zoom, 0, None, S)
    cases = {'unknown format': dict(fmt=7), 'negative format': dict(fmt=-1), 'unknown output': dict(out_fmt=F['yuyv']), 'unknown matrix': dict(matrix=3),
             'no frames': dict(N=0), 'null src': dict(src=None), 'null dst': dict(dst=None), 'too large': dict(IW=16386),
             'odd capture': dict(fmt=F['nv12'], IH=17, out_fmt=O['rgb']), 'odd yuyv': dict(fmt=F['yuyv'], IW=31, out_fmt=O['rgb']),
             'odd output': dict(IH=17), 'nine markers': dict(M=9, centres=c, table=t), 'no table': dict(M=2, centres=c),
             'sx': dict(M=2, centres=c, table=t, sx=float('nan')), 'heat too large': dict(heat=h, HW=1025), 'amax': dict(heat=h, amax=256),
             'zoom': dict(inset=p, zoom=5), 'inset outside': dict(inset=p, x0=29), 'inset below': dict(inset=p, y0=7, zoom=3)}
    words = {'unknown format': 'unknown format', 'negative format': 'unknown format', 'unknown output': 'unknown output format', 'unknown matrix': 'unknown matrix',
             'no frames': 'bad arguments', 'null src': 'bad arguments', 'null dst': 'bad arguments', 'too large': 'frame too large', 'odd capture': 'even',
             'odd yuyv': 'even', 'odd output': 'even', 'nine markers': 'M must be', 'no table': 'centres and marker_table', 'sx': 'finite',
             'heat too large': 'heat map too large', 'amax': 'amax', 'zoom': 'zoom', 'inset outside': 'inside the frame', 'inset below': 'inside the frame'}
    for name, kw in cases.items():
        assert call(**kw) != 0, name
        msg = k.lib.eve_last_error().decode()
        assert msg.startswith('overlay_render:') and words[name] in msg, (name, msg)
        assert k.lib.eve_last_kernel() == before, name
    torch.cuda.synchronize()
    assert (out.cpu() == SENTINEL).all()
    with pytest.raises(ValueError, match='out_format'):
        k.overlay_render(frames.view(2, 18, 32, 4), 'rgb', 'yuyv')
    with pytest.raises(ValueError, match='inset'):
        render_overlay(frames.view(2, 18, 32, 4), inset=dict(inset=p, xy=(30, 0)))
    assert k.lib.eve_last_kernel() == before


def test_the_wrappers_are_the_contract():
    """kernels.overlay_render / data.render_overlay on tensors, with an output buffer of the caller's."""
    N, IH, IW = 2, 18, 32
    buf = random_frames('yuyv', N, IH, IW)
    markers = some_markers(N, IH, IW, 3, seed=2)
    heat = np.random.default_rng(5).random((N, 4, 6)).astype(np.float32)
    inset = np.random.default_rng(6).integers(0, 256, (N, 3, 5, 3), dtype=np.uint8)
    out = torch.zeros((N, IH * 3 // 2, IW), dtype=torch.uint8, device='cuda')
    got = render_overlay(gpu(buf), format='yuyv', out_format='i420', matrix='bt709',
                         markers=dict(centres=gpu(markers['centres']), table=markers['table'].tolist(), sx=0.75, sy=1.25),
                         heat=dict(heat=gpu(heat), color=(9, 200, 30), amax=77), inset=dict(inset=gpu(inset), zoom=2, mirror=True),
                         frame_valid=gpu(np.array([1, 0], dtype=np.uint8)), out=out)
    assert got.data_ptr() == out.data_ptr()
    want = oref.render(buf, 'yuyv', 'i420', 'bt709', dict(markers, sx=0.75, sy=1.25), dict(heat=heat, color=(9, 200, 30), amax=77),
                       dict(inset=inset, x0=IW - 10, y0=IH - 6, zoom=2, mirror=True), np.array([1, 0]))
    assert np.array_equal(got.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ EVEStream
SPEC = dict(markers=[dict(key='PoG_px_initial', fill=(180, 180, 0), r_fill=3, r_outline=5), dict(key='PoG_px_final', fill=(0, 180, 0), r_fill=3, r_outline=5)],
            heat=True, inset='eyes')
CAPTURE = (144, 256)


@functools.lru_cache(maxsize=None)
def nv12_capture(seed, B=2, T=4):
    buf = pref.random_yuv_frames('nv12', B * T, CAPTURE[0], CAPTURE[1], seed)
    return torch.from_numpy(buf).view((B, T) + buf.shape[1:]).cuda()


def expected(chunk, out, spec, inset, frame_valid=None, matrix='bt601'):
    """overlay_ref on the capture and THE STEP'S OWN returned PoG_px_*, heatmap_final and valid -> [B, Tc, ...]."""
    cap = chunk['screen_frame_nv12']
    B, Tc = cap.shape[:2]
    N, (IH, IW) = B * Tc, CAPTURE
    markers = dict(centres=np.stack([out[m[0]].reshape(N, 2).float().cpu().numpy() for m in spec.markers], axis=1), valid=None,
                   table=np.array(spec.marker_table(), dtype=np.int32), sx=np.float32(IW / 1920.0), sy=np.float32(IH / 1080.0))
    hm = out['heatmap_final']
    heat = dict(heat=hm.reshape((N,) + tuple(hm.shape[-2:])).float().cpu().numpy(), color=spec.heat_color, amax=spec.heat_amax)
    inset = dict(inset=inset, x0=IW - inset.shape[2], y0=IH - inset.shape[1], zoom=1, mirror=True)
    res = oref.render(cap.reshape((N,) + tuple(cap.shape[2:])).cpu().numpy(), 'nv12', spec.out_format, matrix, markers, heat, inset, frame_valid)
    return res.reshape((B, Tc) + res.shape[1:])


def test_stream_renders_under_graph_replay():
    """bf16, B = 2, Tc = 2, a 144 x 256 screen_frame_nv12 capture, initial and final markers, heat, inset='eyes' from a uint8 patch chunk:
    two chunks through one graph, `rendered` == the contract on the step's own results, exactly; then lengths = [1, 2]."""
    model, _ = make_model(dtype=torch.bfloat16)
    _, d, _ = gpu_clip(2, 4, seed=5)
    g_ = torch.Generator().manual_seed(3)
    eyes = {side + '_eye_patch': torch.randint(0, 256, (2, 4, 128, 128, 3), generator=g_, dtype=torch.uint8).cuda() for side in ('left', 'right')}
    src = dict({k_: v for k_, v in d.items() if k_ not in ('screen_frame', 'left_eye_patch', 'right_eye_patch')}, screen_frame_nv12=nv12_capture(41), **eyes)
    ch = lambda i: {k_: v[:, 2 * i:2 * i + 2].contiguous() for k_, v in src.items()}
    spec = OverlaySpec(**SPEC)
    g = eve_amd.EVEStream(model, 2)
    rendered = []
    for i, lengths in enumerate((None, None, [1, 2])):
        chunk = ch(i % 2)
        out = {k_: v.clone() for k_, v in g.step(chunk, return_heatmaps=True, lengths=lengths, render=spec).items()}
        assert out['rendered'].dtype == torch.uint8 and tuple(out['rendered'].shape) == (2, 2, 216, 256)
        inset = torch.cat([chunk['right_eye_patch'], chunk['left_eye_patch']], dim=3).reshape(4, 128, 256, 3).cpu().numpy()
        fv = None
        if lengths is not None:
            assert out['valid'].tolist() == [[True, False], [True, True]]
            fv = out['valid'].reshape(4).cpu().numpy().astype(np.uint8)
        want = expected(chunk, out, spec, inset, fv)
        assert np.array_equal(out['rendered'].cpu().numpy(), want), i
        if lengths is not None:                                        # stream 0's second frame: the bare converted capture
            bare = oref.render(chunk['screen_frame_nv12'][0, 1:2].cpu().numpy(), 'nv12', 'nv12')
            assert np.array_equal(out['rendered'][0, 1].cpu().numpy(), bare[0])
        rendered.append(out['rendered'])
        assert len(g._graphs) == (1 if i < 2 else 2)                   # the second chunk replays the first one's graph
    assert not torch.equal(rendered[0], rendered[1])
    # the unrendered step is its own graph, and returns what the rendered one returned beside `rendered`
    plain = g.step(ch(0), return_heatmaps=True)
    assert 'rendered' not in plain and len(g._graphs) == 3
    with pytest.raises(ValueError, match='capture'):
        g.step({k_: v[:, :2].contiguous() for k_, v in d.items()}, render=spec)


def test_stream_cuts_the_inset_in_the_camera_form():
    """camera_frame + warps: the inset region equals the quantised eye_warp_u8_to_nchw patches, [right | left], mirrored."""
    model, _ = make_model(dtype=torch.bfloat16)
    _, d, _ = gpu_clip(2, 2, seed=5)
    _, cam = both_forms({k_: v for k_, v in d.items() if k_ != 'screen_frame'}, 'nv12', 33, 2)
    chunk = dict(cam, screen_frame_nv12=nv12_capture(42)[:, :2].contiguous())
    spec = OverlaySpec(**SPEC)
    g = eve_amd.EVEStream(model, 2)
    out = {k_: v.clone() for k_, v in g.step(chunk, return_heatmaps=True, render=spec).items()}
    k = default_kernels()
    frames = chunk['camera_frame'].reshape((4,) + tuple(chunk['camera_frame'].shape[2:]))
    cut = lambda side: quantise_patches(k.eye_warp_u8_to_nchw(frames, chunk[side + '_eye_warp'].reshape(4, 3, 3).contiguous(), (128, 128)))
    inset = torch.cat([cut('right'), cut('left')], dim=2).cpu().numpy()
    assert inset.shape == (4, 128, 256, 3) and inset.dtype == np.uint8 and inset.min() < inset.max()
    want = expected(chunk, out, spec, inset)
    assert np.array_equal(out['rendered'].cpu().numpy(), want)
    rgb = render_overlay(chunk['screen_frame_nv12'].reshape(4, 216, 256), format='nv12', out_format='rgb', inset=dict(inset=torch.from_numpy(inset).cuda(), mirror=True))
    assert np.array_equal(rgb[:, -128:, :].cpu().numpy(), inset[:, :, ::-1])
