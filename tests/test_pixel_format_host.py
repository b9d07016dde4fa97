"""CPU: the pixel formats of the eye-patch warp -- the integer YUV -> RGB conversion of eve_eye_warp_fmt_to_nchw / _to_stem
(tests/pixel_format_ref.py) over all 2^24 byte triples against its float64 formula, its constants and fixed points, the three YUV
layouts against each other, and the keys camera_frame_bgr / _nv12 / _i420 / _yuyv and screen_frame_bgr from eye_input through
EyeNet, EVE and EVEStream on the torch-CPU stand-in kernels.  tests/test_gpu_pixel_formats.py checks the HIP kernels and the
graph mode."""
import numpy as np
import pytest
import torch

import eve_amd
from eve_amd import data, kernels
from eve_amd.eye_net import eye_input
import eye_warp_lens_ref as lref
import eye_warp_ref as ref
import pixel_format_ref as pref
import screen_resize_ref as sref
from test_eye_warp_host import FRAME, SIZE, SMALL_EYES, camera_batch, warps_for
from test_stream_host import chunk_of, clip
from test_stream_ragged_host import CONFIGS, RaggedFakes, make_model

SCREEN = (72, 128)


class PixelFakes(RaggedFakes):
    eye_warp_u8_to_nchw = ref.eye_warp_u8_to_nchw
    eye_warp_u8_to_stem = ref.eye_warp_u8_to_stem
    eye_warp_lens_u8_to_nchw = lref.eye_warp_lens_u8_to_nchw
    eye_warp_lens_u8_to_stem = lref.eye_warp_lens_u8_to_stem
    eye_warp_fmt_to_nchw = pref.eye_warp_fmt_to_nchw
    eye_warp_fmt_to_stem = pref.eye_warp_fmt_to_stem
    screen_u8_area_to_nchw = sref.screen_u8_area_to_nchw
    screen_u8_area_bgr_to_nchw = pref.screen_u8_area_bgr_to_nchw


@pytest.fixture()
def fake():
    k = PixelFakes()
    kernels.set_default_kernels(k)
    yield k
    kernels.set_default_kernels(None)
    eve_amd.reset_standalone_config()


def yuv_camera(fmt, B, T, seed):
    """Random frames of FRAME size in the layout of fmt -> uint8 [B, T, ...]."""
    v = pref.random_yuv_frames(fmt, B * T, FRAME[0], FRAME[1], seed)
    return torch.from_numpy(v).view((B, T) + v.shape[1:])


def converted(frames, fmt, matrix='bt601'):
    """[B, T, ...] of fmt -> camera_frame uint8 [B, T, IH, IW, 3]."""
    B, T = frames.shape[:2]
    rgb = pref.to_rgb(frames.numpy().reshape((B * T,) + tuple(frames.shape[2:])), fmt, matrix)
    return torch.from_numpy(rgb).view((B, T) + rgb.shape[1:])


def fmt_batch(batch, key, frames, lw, rw):
    b = {k_: v for k_, v in batch.items() if k_ not in ('left_eye_patch', 'right_eye_patch')}
    return dict(b, left_eye_warp=lw, right_eye_warp=rw, **{key: frames})


# ------------------------------------------------------------------------------------------------ the conversion
@pytest.mark.parametrize('matrix', list(pref.COEFFICIENTS))
def test_the_integer_conversion_against_float64_over_all_triples(matrix):
    """All 2^24 (Y, U, V): the integer result differs from clip(floor(float64 formula + 0.5)) by at most 1, in fewer than 0.5 % of
    the triples (the constants are the coefficients rounded to 20 fractional bits: a difference needs a value within 2^-20 * 255
    of a rounding boundary)."""
    c, y0 = pref.COEFFICIENTS[matrix]
    Y, U, V = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing='ij', sparse=True)
    got = pref.yuv_to_rgb(*np.broadcast_arrays(Y, U, V), matrix).astype(np.int16)
    yy = c[0] * np.maximum(0, Y.astype(np.float64) - y0)
    u, v = U.astype(np.float64) - 128.0, V.astype(np.float64) - 128.0
    want = [yy + c[1] * v + 0.0 * u, yy - c[3] * v - c[2] * u, yy + c[4] * u + 0.0 * v]
    differs = np.zeros((256, 256, 256), dtype=bool)
    for ch, w in enumerate(want):
        d = np.abs(got[..., ch] - np.clip(np.floor(w + 0.5), 0, 255).astype(np.int16))
        assert d.max() <= 1, (matrix, ch, int(d.max()))
        differs |= d != 0
    share = 100.0 * differs.mean()
    print('%s: %.3f %% of the triples differ by one' % (matrix, share))
    assert share < 0.5, (matrix, share)


def test_constants_and_fixed_points():
    assert pref.constants('bt601') == (16, 1220542, 1673527, 409993, 852492, 2116026)
    assert pref.constants('bt709') == (16, 1220542, 1880097, 223347, 558891, 2214593)
    assert pref.constants('jfif') == (0, 1048576, 1470104, 360853, 748826, 1858077)
    assert kernels.YUV_MATRICES == {'bt601': 0, 'bt709': 1, 'jfif': 2}
    Y = np.arange(256, dtype=np.uint8)
    grey = np.full(256, 128, dtype=np.uint8)
    for matrix in pref.COEFFICIENTS:
        rgb = pref.yuv_to_rgb(Y, grey, grey, matrix)
        assert (rgb[:, 0] == rgb[:, 1]).all() and (rgb[:, 1] == rgb[:, 2]).all(), matrix      # U = V = 128: R == G == B
    for matrix in ('bt601', 'bt709'):                          # limited range: 16 -> 0, 235 -> 255, below 16 black, above 235 white
        rgb = pref.yuv_to_rgb(Y, grey, grey, matrix)
        assert rgb[16, 0] == 0 and rgb[235, 0] == 255 and not rgb[:16].any() and (rgb[235:] == 255).all()
        assert rgb[17, 0] == 1 and rgb[234, 0] == 254
    assert np.array_equal(pref.yuv_to_rgb(Y, grey, grey, 'jfif')[:, 1], Y)                     # full range: the identity on grey
    with pytest.raises(ValueError):
        pref.constants('nonsense')
    # a pure chroma swing: V drives red up and green down, U blue up and green down
    base, red, blue = (pref.yuv_to_rgb(np.uint8(128), np.uint8(u_), np.uint8(v_), 'bt601').astype(int) for u_, v_ in ((128, 128), (128, 200), (200, 128)))
    assert red[0] > base[0] and red[1] < base[1] and red[2] == base[2]
    assert blue[2] > base[2] and blue[1] < base[1] and blue[0] == base[0]


@pytest.mark.parametrize('matrix', list(pref.COEFFICIENTS))
def test_the_three_yuv_layouts_of_the_same_planes_convert_alike(matrix):
    g = np.random.default_rng(3)
    N, IH, IW = 2, 6, 10
    Y = g.integers(0, 256, size=(N, IH, IW), dtype=np.uint8)
    U, V = (g.integers(0, 256, size=(N, IH // 2, IW // 2), dtype=np.uint8) for _ in range(2))
    rgb = [pref.to_rgb(pref.pack(Y, U, V, fmt), fmt, matrix) for fmt in ('nv12', 'i420', 'yuyv')]
    assert rgb[0].shape == (N, IH, IW, 3) and rgb[0].dtype == np.uint8
    assert np.array_equal(rgb[0], rgb[1]) and np.array_equal(rgb[0], rgb[2])
    # the byte offsets of the layouts, as include/eve_hip.h states them
    y, x = 3, 7
    nv12, i420, yuyv = (pref.pack(Y, U, V, fmt).reshape(N, -1) for fmt in ('nv12', 'i420', 'yuyv'))
    q = (IH // 2) * (IW // 2)
    assert nv12[1, IH * IW + (y >> 1) * IW + (x & ~1)] == U[1, 1, 3] and nv12[1, IH * IW + (y >> 1) * IW + (x & ~1) + 1] == V[1, 1, 3]
    assert i420[1, IH * IW + (y >> 1) * (IW // 2) + (x >> 1)] == U[1, 1, 3] and i420[1, IH * IW + q + (y >> 1) * (IW // 2) + (x >> 1)] == V[1, 1, 3]
    assert yuyv[1, (y * IW + x) * 2] == Y[1, y, x] and yuyv[1, (y * IW + (x & ~1)) * 2 + 1] == U[1, 1, 3] and yuyv[1, (y * IW + (x | 1)) * 2 + 1] == V[1, 1, 3]
    want = pref.yuv_to_rgb(Y[1, y, x], U[1, 1, 3], V[1, 1, 3], matrix)
    assert np.array_equal(rgb[0][1, y, x], want)
    bgr = g.integers(0, 256, size=(N, IH, IW, 4), dtype=np.uint8)
    assert np.array_equal(pref.to_rgb(bgr, 'bgr'), bgr[..., [2, 1, 0]])


def test_the_chroma_checkerboard_alternates_per_chroma_sample():
    for fmt in ('nv12', 'i420', 'yuyv'):
        Y, U, V = pref.planes(pref.chroma_checkerboard(fmt, 2, 8, 12), fmt)
        assert (Y == 128).all() and set(np.unique(U)) == {16, 240}
        assert (U[:, :, 0:-2:2] != U[:, :, 2::2]).all() and (U[:, :, 0::2] == U[:, :, 1::2]).all()      # per pair along x
        step = 1 if fmt == 'yuyv' else 2
        assert (U[:, 0:-step:step] != U[:, step::step]).all() and (U[0] != U[1]).all() and (U != V).all()


# ------------------------------------------------------------------------------------------------ eye_input and the wrappers' checks
def test_eye_input_takes_one_frame_key_and_checks_its_shape():
    batch = clip(2, 3, seed=3, size=SIZE)
    lw, rw = warps_for(2, 3, seed=5)
    for fmt in pref.FORMATS:
        frames = yuv_camera(fmt, 2, 3, seed=4)
        cam = fmt_batch(batch, 'camera_frame_' + fmt, frames, lw, rw)
        assert eye_input(cam) is frames and tuple(eye_input(cam).shape[:2]) == (2, 3)
    nv12, yuyv, bgr = (yuv_camera(f_, 2, 3, seed=4) for f_ in ('nv12', 'yuyv', 'bgr'))
    cam = fmt_batch(batch, 'camera_frame_nv12', nv12, lw, rw)
    with pytest.raises(ValueError, match='one camera frame key'):
        eye_input(dict(cam, camera_frame=converted(nv12, 'nv12')))
    with pytest.raises(ValueError, match='one camera frame key'):
        eye_input(dict(cam, camera_frame_yuyv=yuyv))
    with pytest.raises(ValueError, match='not both'):
        eye_input(dict(cam, left_eye_patch=batch['left_eye_patch'], right_eye_patch=batch['right_eye_patch']))
    with pytest.raises(ValueError, match='missing left_eye_warp'):
        eye_input({k_: v for k_, v in cam.items() if k_ != 'left_eye_warp'})
    odd_rows = torch.zeros((2, 3, 141, 120), dtype=torch.uint8)           # IH = 94 is fine; 141 rows = 94 * 3 / 2
    assert eye_input(fmt_batch(batch, 'camera_frame_i420', odd_rows, lw, rw)) is odd_rows
    for key, bad in (('camera_frame_nv12', torch.zeros((2, 3, 142, 120), dtype=torch.uint8)),       # rows not divisible by 3: IH odd
                     ('camera_frame_i420', torch.zeros((2, 3, 144, 121), dtype=torch.uint8)),       # IW odd
                     ('camera_frame_yuyv', torch.zeros((2, 3, 96, 121, 2), dtype=torch.uint8))):
        with pytest.raises(ValueError, match=key):
            eye_input(fmt_batch(batch, key, bad, lw, rw))
    for key, bad in (('camera_frame_yuyv', yuyv[..., :1]), ('camera_frame_yuyv', bgr), ('camera_frame_bgr', yuyv), ('camera_frame_nv12', yuyv),
                     ('camera_frame_nv12', nv12.float()), ('camera_frame_i420', nv12[0]), ('camera_frame_bgr', bgr.numpy())):
        with pytest.raises(TypeError, match=key):
            eye_input(fmt_batch(batch, key, bad, lw, rw))
    with pytest.raises(ValueError, match='camera_lens'):
        eye_input(dict(batch, camera_lens=torch.zeros((2, 3, 12))))


def test_warp_eye_patches_takes_a_format(fake):
    lw, _ = warps_for(2, 3, seed=2)
    for fmt in pref.FORMATS:
        frames = yuv_camera(fmt, 2, 3, seed=1)
        got = data.warp_eye_patches(frames, lw, size=(36, 60), format=fmt, matrix='bt709')
        want = data.warp_eye_patches(converted(frames, fmt, 'bt709'), lw, size=(36, 60))
        assert got.dtype == torch.float32 and tuple(got.shape) == (2, 3, 3, 36, 60) and torch.equal(got, want)
        assert torch.equal(data.warp_eye_patches(frames[1], lw[1], size=(36, 60), format=fmt, matrix='bt709'), got[1])
        if fmt != 'bgr':
            assert not torch.equal(got, data.warp_eye_patches(frames, lw, size=(36, 60), format=fmt))
    nv12 = yuv_camera('nv12', 2, 3, seed=1)
    with pytest.raises(ValueError):
        data.warp_eye_patches(nv12, lw, format='nv21')
    with pytest.raises(ValueError):
        data.warp_eye_patches(nv12, lw, format='nv12', matrix='nonsense')
    with pytest.raises(ValueError):
        data.warp_eye_patches(nv12[:, :, :-1], lw, format='nv12')
    with pytest.raises(TypeError):
        data.warp_eye_patches(nv12.float(), lw, format='nv12')
    with pytest.raises(TypeError):
        data.warp_eye_patches(nv12, lw.double(), format='nv12')


# ------------------------------------------------------------------------------------------------ EyeNet / EVE / EVEStream
def same(got, want):
    assert set(got) == set(want)
    for key in want:
        if torch.is_tensor(want[key]):
            assert torch.equal(got[key], want[key]), key


@pytest.mark.parametrize('fmt', ['nv12', 'yuyv', 'i420', 'bgr'])
def test_eyenet_takes_the_frame_as_the_camera_delivers_it(fake, fmt):
    model = make_model(dict(CONFIGS['gru-cgru'][0], **SMALL_EYES))
    B, T = 2, 2
    batch = clip(B, T, seed=3, size=SIZE)
    frames, (lw, rw) = yuv_camera(fmt, B, T, seed=6), warps_for(B, T, seed=7)
    cam = fmt_batch(batch, 'camera_frame_' + fmt, frames, lw, rw)
    with torch.no_grad():
        got = model.eye_net.forward_sequence(cam)
        want = model.eye_net.forward_sequence(camera_batch(batch, converted(frames, fmt), lw, rw))
    assert tuple(got['left_g_initial'].shape) == (B, T, 2)
    same(got, want)
    if fmt == 'bgr':
        return
    model.eye_net.yuv_matrix = 'bt709'                           # the matrix is the module's attribute
    with torch.no_grad():
        hd = model.eye_net.forward_sequence(cam)
        hd_want = model.eye_net.forward_sequence(camera_batch(batch, converted(frames, fmt, 'bt709'), lw, rw))
    same(hd, hd_want)
    assert not torch.equal(hd['left_g_initial'], got['left_g_initial'])
    model.eye_net.yuv_matrix = 'nonsense'
    with pytest.raises(ValueError, match='yuv_matrix'):
        model.eye_net.forward_sequence(cam)
    with torch.no_grad():                                        # ... which the RGB key never reads
        model.eye_net.forward_sequence(camera_batch(batch, converted(frames, fmt), lw, rw))


def test_the_packed_route_and_the_lens_go_through_the_format_calls(fake):
    """A 16-bit trunk on 128-wide patches: two eye_warp_fmt_to_stem calls (here with a lens) give what the lens calls give on the
    converted frame."""
    eve_amd.get_config().import_dict(dict(eyes_size=[128, 32]))
    net = eve_amd.EyeNet()
    net.compute_dtype = torch.bfloat16
    net.eval()
    batch = clip(1, 2, seed=3, size=SIZE)
    wide = torch.from_numpy(pref.random_yuv_frames('nv12', 2, 48, 160, seed=8)).view(1, 2, 72, 160)
    shifts = torch.from_numpy(np.stack([ref.shift(3.5, 2.25), ref.shift(30, 16)])).view(1, 2, 3, 3)
    wl = torch.from_numpy(np.stack([lref.lens_row(150, 150, 80, 24, k1=-0.2, k2=0.05), lref.lens_row(150, 150, 80, 24)])).view(1, 2, 12)
    rest = dict(left_eye_warp=shifts, right_eye_warp=shifts.flip(1).contiguous(), camera_lens=wl, left_h=batch['left_h'], right_h=batch['right_h'])
    with torch.no_grad():
        got = net.forward_sequence(dict(rest, camera_frame_nv12=wide))
        want = net.forward_sequence(dict(rest, camera_frame=converted(wide, 'nv12')))
    same(got, want)


def test_eve_eval_takes_nv12(fake):
    model = make_model(dict(CONFIGS['gru-cgru'][0], **SMALL_EYES))
    B, T = 1, 2
    batch = clip(B, T, seed=3, size=SIZE)
    frames, (lw, rw) = yuv_camera('nv12', B, T, seed=9), warps_for(B, T, seed=10)
    with torch.no_grad():
        got = model(fmt_batch(batch, 'camera_frame_nv12', frames, lw, rw))
        want = model(camera_batch(batch, converted(frames, 'nv12'), lw, rw))
    same(got, want)
    assert 'PoG_px_final' in got


@pytest.mark.parametrize('lengths', [None, [1, 2]], ids=['uniform', 'ragged'])
def test_stream_steps_take_nv12_in_two_chunks(fake, lengths):
    model = make_model(dict(CONFIGS['gru-cgru'][0], **SMALL_EYES))
    B, T = 2, 4
    batch = clip(B, T, seed=3, size=SIZE)
    frames, (lw, rw) = yuv_camera('nv12', B, T, seed=11), warps_for(B, T, seed=12)
    cam = fmt_batch(batch, 'camera_frame_nv12', frames, lw, rw)
    rgb = camera_batch(batch, converted(frames, 'nv12'), lw, rw)
    a, b = eve_amd.EVEStream(model, B, use_graph=False), eve_amd.EVEStream(model, B, use_graph=False)
    part = lambda src, t0: dict(chunk_of(src, t0, t0 + 2), **{k_: src[k_][:, t0:t0 + 2].contiguous() for k_ in src if k_.startswith(('camera_frame', 'left_eye_warp', 'right_eye_warp'))})
    for t0 in (0, 2):
        got = a.step(part(cam, t0), return_heatmaps=True, lengths=lengths)
        want = b.step(part(rgb, t0), return_heatmaps=True, lengths=lengths)
        assert 'heatmap_final' in got and ('valid' in got) == (lengths is not None)
        same(got, want)
    sa, sb = a.get_state(), b.get_state()
    for key in sb:
        for x, y in zip(sa[key] if isinstance(sa[key], tuple) else (sa[key],), sb[key] if isinstance(sb[key], tuple) else (sb[key],)):
            assert torch.equal(x, y), key
    with pytest.raises(ValueError, match='one camera frame key'):
        a.step(dict(part(cam, 0), camera_frame=part(rgb, 0)['camera_frame']))


# ------------------------------------------------------------------------------------------------ the screen
@pytest.mark.parametrize('shape', [(144, 256, 3), (100, 171, 4), (72, 128, 3)], ids=['144x256x3', '100x171x4', 'same-size'])
def test_screen_frame_bgr_equals_the_reversed_capture(fake, shape):
    model = make_model(*CONFIGS['gru-cgru'])
    B, T = 2, 2
    batch = clip(B, T, seed=3)
    ch = chunk_of(batch, 0, T)
    cap = torch.from_numpy(np.random.default_rng(7).integers(0, 256, size=(B, T) + shape, dtype=np.uint8))
    rev = cap[..., [2, 1, 0]].contiguous()
    a = data.preprocess_screen_frames(cap, size=SCREEN, bgr=True)
    assert a.dtype == torch.float32 and tuple(a.shape) == (B, T, 3) + SCREEN
    assert torch.equal(a, data.preprocess_screen_frames(rev, size=SCREEN)) and not torch.equal(a, data.preprocess_screen_frames(cap, size=SCREEN))
    heat = torch.rand((B, T, 1) + SCREEN, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        got, _ = model.refine_net.forward_sequence(heat, screen_frame_bgr=cap)
        want, _ = model.refine_net.forward_sequence(heat, rev)
        assert torch.equal(got, want)
        whole = {k_: v for k_, v in batch.items() if k_ != 'screen_frame'}
        same(model(dict(whole, screen_frame_bgr=cap)), model(dict(whole, screen_frame=rev)))
        rest = {k_: v for k_, v in ch.items() if k_ != 'screen_frame'}
        s1, s2 = eve_amd.EVEStream(model, B, use_graph=False), eve_amd.EVEStream(model, B, use_graph=False)
        same(s1.step(dict(rest, screen_frame_bgr=cap), return_heatmaps=True), s2.step(dict(rest, screen_frame=rev), return_heatmaps=True))
        with pytest.raises(ValueError, match='not both'):
            s1.step(dict(ch, screen_frame_bgr=cap))
        with pytest.raises(ValueError, match='not both'):
            model.refine_net.forward_sequence(heat, rev, screen_frame_bgr=cap)
        with pytest.raises(TypeError, match='screen_frame_bgr'):
            model.refine_net.forward_sequence(heat, screen_frame_bgr=cap.float())
