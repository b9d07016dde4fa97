"""CPU: surfaces -- data.SurfaceLayout's descriptors against hand-written ones and against the address rule in numpy
(tests/surface_ref.py), linear / embed as inverses, the refusals of the layout and of the wrappers, and the keys camera_surface /
screen_surface through EyeNet, RefineNet, EVE and EVEStream on torch-CPU stand-ins that linearise the surface and call the existing
stand-ins.  tests/test_gpu_surfaces.py checks the HIP kernels and the graph mode."""
import ctypes

import numpy as np
import pytest
import torch

import eve_amd
from eve_amd import _lib, data, kernels
from eve_amd.data import SurfaceLayout
from eve_amd.eye_net import EYE_SURFACE_KEY, camera_frame_key, eye_input
from eve_amd.refine_net import SCREEN_SURFACE_KEY, screen_frame_key
import surface_ref as sref
from test_eye_warp_host import FRAME, SIZE, SMALL_EYES, warps_for
from test_pixel_format_host import same
from test_screen_formats_host import ScreenFormatFakes
from test_stream_host import chunk_of, clip
from test_stream_ragged_host import CONFIGS, make_model

SCREEN = (72, 128)
CAPTURE = (144, 256)


def _linear_call(frames, layout):
    """The stand-ins' first step: the surface tensor [N, frame_stride] -> (the byte-linear frames as a tensor, their format)."""
    return torch.from_numpy(sref.linear(frames.numpy(), layout)), sref.LINEAR_FORMAT[layout.format]


class SurfaceFakes(ScreenFormatFakes):
    """The three surface calls as linear() plus the existing stand-ins, behind the real wrapper's own argument checks."""

    def eye_warp_surface_to_nchw(self, frames, warps, out_hw, layout, matrix='bt601', lens=None):
        kernels.HipKernels._surface_args('eye_warp_surface_to_nchw', frames, layout, matrix)
        lin, fmt = _linear_call(frames, layout)
        if fmt != 'rgb':
            return self.eye_warp_fmt_to_nchw(lin, warps, out_hw, fmt, matrix=matrix, lens=lens)
        return self.eye_warp_u8_to_nchw(lin, warps, out_hw) if lens is None else self.eye_warp_lens_u8_to_nchw(lin, warps, lens, out_hw)

    def eye_warp_surface_to_stem(self, frames, warps, out_hw, layout, matrix='bt601', lens=None, out=None, dtype=torch.bfloat16):
        return self.stem_pack_input(self.eye_warp_surface_to_nchw(frames, warps, out_hw, layout, matrix, lens), out=out, dtype=dtype)

    def screen_area_surface_to_nchw(self, frames, out_hw, layout, matrix='bt601'):
        kernels.HipKernels._surface_args('screen_area_surface_to_nchw', frames, layout, matrix)
        lin, fmt = _linear_call(frames, layout)
        return self.screen_u8_area_to_nchw(lin, out_hw) if fmt == 'rgb' else self.screen_area_fmt_to_nchw(lin, out_hw, fmt, matrix=matrix)


@pytest.fixture()
def fake():
    k = SurfaceFakes()
    kernels.set_default_kernels(k)
    yield k
    kernels.set_default_kernels(None)
    eve_amd.reset_standalone_config()


def padded(fmt, W, H):
    """A layout of every kind of padding the format can have: a pitch beyond the row, coded rows below the picture, an even crop
    origin, and (where the format has planes) plane starts pushed to a 64-byte boundary."""
    bpp = sref.BYTES_PER_PIXEL[fmt]
    pitch, coded, x0, y0 = (W + 22) * bpp + (bpp * 2 if fmt not in ('rgb', 'bgr') else 1), H + 10, 6, 4
    pitch += pitch % 2
    offsets = None
    if fmt in ('nv12', 'nv21', 'p010'):
        offsets = (-(-pitch * coded // 64) * 64 + 64,)
    elif fmt in ('i420', 'yv12'):
        first = -(-pitch * coded // 64) * 64
        offsets = (first, -(-(first + pitch // 2 * (coded // 2)) // 64) * 64 + 64)
    return SurfaceLayout(fmt, W, H, pitch=pitch, coded_height=coded, x0=x0, y0=y0, plane_offsets=offsets)


# ------------------------------------------------------------------------------------------------ the descriptor
def test_hand_written_descriptors():
    hd = SurfaceLayout('nv12', 1920, 1080, pitch=2048, coded_height=1088).descriptor()
    assert hd == dict(kind=1, width=1920, height=1080, frame_stride=2048 * 1632, frame_bytes=2048 * 1632, offset=(0, 2048 * 1088, 2048 * 1088 + 1),
                      pitch=(2048, 2048, 2048), step=(1, 2, 2), xshift=1, yshift=1)
    nv21 = SurfaceLayout('nv21', 1920, 1080, pitch=2048, coded_height=1088).descriptor()
    assert nv21['offset'] == (0, 2048 * 1088 + 1, 2048 * 1088) and {k_: v for k_, v in nv21.items() if k_ != 'offset'} == {k_: v for k_, v in hd.items() if k_ != 'offset'}
    # P010: 16-bit little-endian words, read as their high byte: offset + 1, luma step 2, chroma step 4 (U word, V word)
    p010 = SurfaceLayout('p010', 1920, 1080, pitch=4096, coded_height=1088).descriptor()
    assert p010 == dict(kind=1, width=1920, height=1080, frame_stride=4096 * 1632, frame_bytes=4096 * 1632, offset=(1, 4096 * 1088 + 1, 4096 * 1088 + 3),
                        pitch=(4096, 4096, 4096), step=(2, 4, 4), xshift=1, yshift=1)
    crop = SurfaceLayout('p010', 64, 48, pitch=192, coded_height=56, x0=2, y0=4).descriptor()
    assert crop['offset'] == (4 * 192 + 2 * 2 + 1, 192 * 56 + 2 * 192 + 2 * 2 + 1, 192 * 56 + 2 * 192 + 2 * 2 + 3) and crop['frame_bytes'] == 192 * 84
    # UYVY is U Y V Y per pixel pair, YUYV Y U Y V
    assert SurfaceLayout('uyvy', 64, 48).descriptor() == dict(kind=1, width=64, height=48, frame_stride=128 * 48, frame_bytes=128 * 48, offset=(1, 0, 2),
                                                              pitch=(128, 128, 128), step=(2, 4, 4), xshift=1, yshift=0)
    assert SurfaceLayout('yuyv', 64, 48).descriptor()['offset'] == (0, 1, 3)
    # a window of a pitched BGRA desktop texture: R is byte 2 of the pixel, the alpha byte is never addressed
    bgra = SurfaceLayout('bgra', 640, 360, pitch=7680, coded_height=1080, x0=100, y0=50).descriptor()
    at = 50 * 7680 + 100 * 4
    assert bgra == dict(kind=0, width=640, height=360, frame_stride=7680 * 1080, frame_bytes=7680 * 1080, offset=(at + 2, at + 1, at),
                        pitch=(7680, 7680, 7680), step=(4, 4, 4), xshift=0, yshift=0)
    assert SurfaceLayout('rgb', 5, 3).descriptor() == dict(kind=0, width=5, height=3, frame_stride=45, frame_bytes=45, offset=(0, 1, 2), pitch=(15, 15, 15),
                                                           step=(3, 3, 3), xshift=0, yshift=0)
    # I420 / YV12: chroma planes at half the pitch; plane_offsets moves them, in memory order
    i420 = SurfaceLayout('i420', 64, 48, pitch=96, coded_height=56, x0=2, y0=4).descriptor()
    assert i420['offset'] == (4 * 96 + 2, 96 * 56 + 2 * 48 + 1, 96 * 56 + 48 * 28 + 2 * 48 + 1) and i420['pitch'] == (96, 48, 48) and i420['step'] == (1, 1, 1)
    yv12 = SurfaceLayout('yv12', 64, 48, pitch=96, coded_height=56, x0=2, y0=4).descriptor()
    assert yv12['offset'] == (i420['offset'][0], i420['offset'][2], i420['offset'][1])
    moved = SurfaceLayout('i420', 64, 48, pitch=96, coded_height=56, plane_offsets=(8192, 12288))
    assert moved.descriptor()['offset'] == (0, 8192, 12288) and moved.frame_bytes == 12288 + 48 * 28


def test_the_ctypes_mirror_and_value_semantics():
    a, b = SurfaceLayout('nv12', 64, 48, pitch=96, coded_height=56, x0=2, y0=4), SurfaceLayout('nv12', 64, 48, pitch=96, coded_height=56, x0=2, y0=4)
    assert a == b and hash(a) == hash(b) and a != SurfaceLayout('nv21', 64, 48, pitch=96, coded_height=56, x0=2, y0=4) and len({a, b}) == 1
    assert a != SurfaceLayout('nv12', 64, 48, pitch=96, coded_height=56, x0=2, y0=6) and 'nv12' in repr(a)
    s = a.as_ctypes()
    d = a.descriptor()
    assert isinstance(s, _lib.Surface) and s.struct_bytes == ctypes.sizeof(_lib.Surface) == 88
    assert (s.kind, s.width, s.height, s.frame_stride, s.frame_bytes, s.xshift, s.yshift) == tuple(
        d[k_] for k_ in ('kind', 'width', 'height', 'frame_stride', 'frame_bytes', 'xshift', 'yshift'))
    assert tuple(s.offset) == d['offset'] and tuple(s.pitch) == d['pitch'] and tuple(s.step) == d['step']
    for name in ('eve_eye_warp_surface_to_nchw', 'eve_eye_warp_surface_to_stem', 'eve_screen_area_surface_to_nchw'):
        assert name in _lib.SIGNATURES
    assert eve_amd.SurfaceLayout is SurfaceLayout


@pytest.mark.parametrize('fmt', sref.FORMATS)
def test_linear_and_embed_are_inverses_and_the_descriptor_addresses_the_same_bytes(fmt):
    """linear / embed slice planes by the layout's parameters; components() reads the descriptor alone.  All three agree, on a
    tight layout and on one with every kind of padding; and embed leaves every byte it does not own at the fill."""
    W, H, N = 20, 12, 2
    for L in (SurfaceLayout(fmt, W, H), padded(fmt, W, H)):
        buf, frame = sref.random_surface(L, N, seed=len(fmt))
        lin_fmt = sref.LINEAR_FORMAT[fmt]
        assert frame.dtype == np.uint8 and frame.shape == {'rgb': (N, H, W, 3), 'bgr': (N, H, W, 3), 'nv12': (N, H * 3 // 2, W), 'i420': (N, H * 3 // 2, W),
                                                           'yuyv': (N, H, W, 2)}[lin_fmt]
        assert np.array_equal(sref.components(buf, L), sref.linear_components(frame, lin_fmt))
        for fill in (0, 255):
            again = sref.embed(frame, L, fill)
            assert again.shape == buf.shape and np.array_equal(sref.linear(again, L), frame)
        a, b = sref.embed(frame, L, 0), sref.embed(frame, L, 255)
        owned = a == b                                                  # the bytes embed wrote
        want = frame.size
        assert int(owned[0].sum()) * N == want and np.array_equal(a[owned], buf[owned])
        other = np.random.default_rng(1).integers(0, 256, size=(N,) + tuple(frame.shape[1:]), dtype=np.uint8)
        assert np.array_equal(sref.linear(sref.embed(other, L, buf), L), other)


def test_layouts_that_cannot_be_are_refused():
    with pytest.raises(ValueError, match='format'):
        SurfaceLayout('nv16', 64, 48)
    for fmt, kw in (('nv12', dict(x0=1)), ('nv12', dict(y0=3)), ('i420', dict(x0=3)), ('yv12', dict(y0=1)), ('p010', dict(x0=5)), ('nv21', dict(y0=1)),
                    ('yuyv', dict(x0=1)), ('uyvy', dict(x0=7))):
        with pytest.raises(ValueError, match='chroma phase'):
            SurfaceLayout(fmt, 64, 48, pitch=512, coded_height=64, **kw)
    SurfaceLayout('yuyv', 64, 48, pitch=512, coded_height=64, y0=3)        # 4:2:2 has a chroma sample in every row
    SurfaceLayout('bgra', 64, 48, pitch=512, coded_height=64, x0=3, y0=5)  # no subsampling: any origin
    with pytest.raises(ValueError, match='even'):
        SurfaceLayout('nv12', 63, 48)
    with pytest.raises(ValueError, match='even'):
        SurfaceLayout('i420', 64, 47)
    with pytest.raises(ValueError, match='pitch'):
        SurfaceLayout('nv12', 64, 48, pitch=60)
    with pytest.raises(ValueError, match='pitch'):
        SurfaceLayout('bgra', 64, 48, pitch=4 * 64 + 4, x0=2)
    with pytest.raises(ValueError, match='pitch'):
        SurfaceLayout('i420', 64, 48, pitch=65)
    with pytest.raises(ValueError, match='coded_height'):
        SurfaceLayout('nv12', 64, 48, coded_height=50, y0=4)
    with pytest.raises(ValueError, match='plane_offsets'):
        SurfaceLayout('nv12', 64, 48, plane_offsets=(4096, 8192))
    with pytest.raises(ValueError, match='plane_offsets'):
        SurfaceLayout('i420', 64, 48, plane_offsets=(4096,))
    with pytest.raises(ValueError, match='plane_offsets'):
        SurfaceLayout('rgb', 64, 48, plane_offsets=(4096,))
    with pytest.raises(ValueError, match='plane_offsets'):
        SurfaceLayout('nv12', 64, 48, plane_offsets=(-64,))
    for bad in (dict(width=0), dict(height=-2), dict(x0=-2), dict(width=64.0)):
        with pytest.raises(ValueError):
            SurfaceLayout('rgb', **dict(dict(width=64, height=48), **bad))


def test_the_wrappers_check_the_tensor_against_the_layout(fake):
    L = SurfaceLayout('nv12', 64, 48, pitch=96, coded_height=56, x0=2, y0=4)
    buf = torch.zeros((2, L.frame_bytes), dtype=torch.uint8)
    warps = torch.eye(3).repeat(2, 1, 1)
    for k in (fake, kernels.HipKernels.__new__(kernels.HipKernels)):      # the stand-in and the real wrapper: refused before the library is touched
        with pytest.raises(ValueError, match='stride'):
            k.screen_area_surface_to_nchw(buf[:, :-1].contiguous(), (8, 6), L)
        with pytest.raises(ValueError, match='stride'):
            k.eye_warp_surface_to_nchw(torch.zeros((2, 56, 100), dtype=torch.uint8), warps, (8, 8), L)
        with pytest.raises(TypeError, match='uint8'):
            k.eye_warp_surface_to_nchw(buf.float(), warps, (8, 8), L)
        with pytest.raises(TypeError, match='SurfaceLayout'):
            k.screen_area_surface_to_nchw(buf, (8, 6), 'nv12')
        with pytest.raises(ValueError, match='matrix'):
            k.screen_area_surface_to_nchw(buf, (8, 6), L, matrix='nonsense')
        with pytest.raises(RuntimeError, match='non-contiguous'):
            k.screen_area_surface_to_nchw(torch.zeros((2, 2 * L.frame_bytes), dtype=torch.uint8)[:, ::2], (8, 6), L)
    real = kernels.HipKernels.__new__(kernels.HipKernels)
    with pytest.raises(TypeError, match='warps'):
        real.eye_warp_surface_to_nchw(buf, warps.double(), (8, 8), L)
    with pytest.raises(TypeError, match='lens'):
        real.eye_warp_surface_to_stem(buf, warps, (8, 8), L, lens=torch.zeros((2, 5)))


@pytest.mark.parametrize('fmt', sref.FORMATS)
def test_the_data_functions_take_a_layout(fake, fmt):
    """warp_eye_patches / preprocess_screen_frames with layout= equal the existing call on the linearised frames, with the frame
    as [rows-of-pitch] where the layout allows it and flat otherwise."""
    B, T = 2, 2
    L = padded(fmt, FRAME[1], FRAME[0])
    buf, frame = sref.random_surface(L, B * T, seed=3)
    lin_fmt = sref.LINEAR_FORMAT[fmt]
    surf = torch.from_numpy(buf).view(B, T, -1)
    lin = torch.from_numpy(frame).view((B, T) + frame.shape[1:])
    lw, _ = warps_for(B, T, seed=2)
    got = data.warp_eye_patches(surf, lw, size=(36, 60), layout=L, matrix='bt709')
    want = data.warp_eye_patches(lin, lw, size=(36, 60), format=lin_fmt, matrix='bt709')
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, T, 3, 36, 60) and torch.equal(got, want)
    assert torch.equal(data.warp_eye_patches(surf[1], lw[1], size=(36, 60), layout=L, matrix='bt709'), got[1])
    scr = data.preprocess_screen_frames(surf, size=(9, 16), layout=L, matrix='jfif')
    if lin_fmt in ('rgb', 'bgr'):
        rgb = lin if lin_fmt == 'rgb' else lin[..., [2, 1, 0]].contiguous()
        want_scr = data.preprocess_screen_frames(rgb, size=(9, 16))
    else:
        want_scr = data.preprocess_screen_frames(lin, size=(9, 16), format=lin_fmt, matrix='jfif')
    assert tuple(scr.shape) == (B, T, 3, 9, 16) and torch.equal(scr, want_scr)
    if L.frame_bytes % L.pitch == 0:
        rows = surf.view(B, T, L.frame_bytes // L.pitch, L.pitch)
        assert torch.equal(data.preprocess_screen_frames(rows, size=(9, 16), layout=L, matrix='jfif'), scr)
        assert torch.equal(data.warp_eye_patches(rows, lw, size=(36, 60), layout=L, matrix='bt709'), got)
    own = data.preprocess_screen_frames(surf[0], layout=L)                # size=None: the visible region's own
    assert tuple(own.shape) == (T, 3) + FRAME
    with pytest.raises(ValueError, match='layout'):
        data.warp_eye_patches(surf, lw, layout=L, format='nv12')
    with pytest.raises(ValueError, match='layout'):
        data.preprocess_screen_frames(surf, layout=L, bgr=True)
    with pytest.raises(ValueError, match='frame_stride'):
        data.warp_eye_patches(surf[..., :-1].contiguous(), lw, layout=L)
    with pytest.raises(TypeError):
        data.warp_eye_patches(surf, lw, layout='nv12')


# ------------------------------------------------------------------------------------------------ EyeNet / RefineNet / EVE / EVEStream
def camera_surface_batch(batch, fmt, B, T, seed, warp_seed):
    """-> (the layout, the batch with camera_surface, the batch with the linearised frames under their existing key)."""
    L = padded(fmt, FRAME[1], FRAME[0])
    buf, frame = sref.random_surface(L, B * T, seed)
    lw, rw = warps_for(B, T, seed=warp_seed)
    rest = {k_: v for k_, v in batch.items() if k_ not in ('left_eye_patch', 'right_eye_patch')}
    rest = dict(rest, left_eye_warp=lw, right_eye_warp=rw)
    lin_fmt = sref.LINEAR_FORMAT[fmt]
    key = 'camera_frame' if lin_fmt == 'rgb' else 'camera_frame_' + lin_fmt
    lin = torch.from_numpy(frame).view((B, T) + frame.shape[1:])
    return L, dict(rest, camera_surface=torch.from_numpy(buf).view(B, T, -1)), dict(rest, **{key: lin})


def screen_surface_pair(fmt, B, T, seed):
    """-> (the layout, screen_surface [B, T, frame_bytes], {the existing key: the linearised capture})."""
    L = padded(fmt, CAPTURE[1], CAPTURE[0])
    buf, frame = sref.random_surface(L, B * T, seed)
    lin_fmt = sref.LINEAR_FORMAT[fmt]
    key = 'screen_frame' if lin_fmt == 'rgb' else 'screen_frame_' + lin_fmt
    return L, torch.from_numpy(buf).view(B, T, -1), {key: torch.from_numpy(frame).view((B, T) + frame.shape[1:])}


def test_the_surface_keys_join_the_frame_keys():
    assert EYE_SURFACE_KEY == 'camera_surface' and SCREEN_SURFACE_KEY == 'screen_surface'
    assert camera_frame_key({'camera_surface': 0, 'screen_surface': 0}) == 'camera_surface' and screen_frame_key({'screen_surface': 0}) == 'screen_surface'
    with pytest.raises(ValueError, match='one camera frame key'):
        camera_frame_key({'camera_surface': 0, 'camera_frame_nv12': 0})
    with pytest.raises(ValueError, match='not both'):
        screen_frame_key({'screen_surface': 0, 'screen_frame': 0})
    assert eve_amd.EyeNet.camera_layout is None and eve_amd.RefineNet.screen_layout is None
    batch = clip(2, 2, seed=3, size=SIZE)
    _, surf, _ = camera_surface_batch(batch, 'nv12', 2, 2, 1, 2)
    assert eye_input(surf) is surf['camera_surface']
    with pytest.raises(TypeError, match='camera_surface'):
        eye_input(dict(surf, camera_surface=surf['camera_surface'].float()))
    with pytest.raises(TypeError, match='camera_surface'):
        eye_input(dict(surf, camera_surface=surf['camera_surface'][0, 0]))


@pytest.mark.parametrize('fmt', ['nv12', 'nv21', 'yv12', 'uyvy', 'p010', 'bgra', 'rgb'])
def test_eyenet_takes_the_surface_as_it_lies(fake, fmt):
    model = make_model(dict(CONFIGS['gru-cgru'][0], **SMALL_EYES))
    B, T = 2, 2
    L, surf, lin = camera_surface_batch(clip(B, T, seed=3, size=SIZE), fmt, B, T, seed=6, warp_seed=7)
    with pytest.raises(ValueError, match='camera_layout'):              # a surface key without its layout
        model.eye_net.forward_sequence(surf)
    model.eye_net.camera_layout = L
    with torch.no_grad():
        got = model.eye_net.forward_sequence(surf)
        want = model.eye_net.forward_sequence(lin)
    assert tuple(got['left_g_initial'].shape) == (B, T, 2)
    same(got, want)
    with pytest.raises(ValueError, match='one camera frame key'):
        model.eye_net.forward_sequence(dict(surf, **{k_: v for k_, v in lin.items() if k_.startswith('camera_frame')}))
    with pytest.raises(ValueError, match='frame_stride'):
        model.eye_net.forward_sequence(dict(surf, camera_surface=surf['camera_surface'][..., :-1].contiguous()))
    if L.kind == 'yuv':
        model.eye_net.yuv_matrix = 'bt709'
        with torch.no_grad():
            hd = model.eye_net.forward_sequence(surf)
            same(hd, model.eye_net.forward_sequence(lin))
        assert not torch.equal(hd['left_g_initial'], got['left_g_initial'])
        model.eye_net.yuv_matrix = 'nonsense'
        with pytest.raises(ValueError, match='yuv_matrix'):
            model.eye_net.forward_sequence(surf)


@pytest.mark.parametrize('fmt', ['nv12', 'p010', 'uyvy', 'bgra'])
def test_refinenet_and_eve_take_the_screen_surface(fake, fmt):
    model = make_model(*CONFIGS['gru-cgru'])
    B, T = 1, 2
    heat = torch.rand((B, T, 1) + SCREEN, generator=torch.Generator().manual_seed(5))
    L, surf, lin = screen_surface_pair(fmt, B, T, seed=7)
    with torch.no_grad():
        with pytest.raises(ValueError, match='screen_layout'):
            model.refine_net.forward_sequence(heat, screen_surface=surf)
        model.refine_net.screen_layout = L
        got, gst = model.refine_net.forward_sequence(heat, screen_surface=surf)
        (key, cap), = lin.items()
        want, wst = model.refine_net.forward_sequence(heat, cap) if key == 'screen_frame' else model.refine_net.forward_sequence(heat, **lin)
        assert tuple(got.shape) == (B, T, 1) + SCREEN and torch.equal(got, want)
        for a, b in zip(gst, wst):
            assert torch.equal(a, b)
        with pytest.raises(ValueError, match='not both'):
            model.refine_net.forward_sequence(heat, screen_surface=surf, screen_frame_bgr=torch.zeros((B, T) + CAPTURE + (3,), dtype=torch.uint8))
        with pytest.raises(TypeError, match='screen_surface'):
            model.refine_net.forward_sequence(heat, screen_surface=surf.float())
        with pytest.raises(ValueError, match='screen_surface'):
            model.refine_net.forward_sequence(heat, screen_surface=surf[..., :-1].contiguous())
        batch = {k_: v for k_, v in clip(B, T, seed=3).items() if k_ != 'screen_frame'}
        full = model(dict(batch, screen_surface=surf))
        assert 'PoG_px_final' in full
        same(full, {k_: v for k_, v in model(dict(batch, **lin)).items() if k_ != 'screen_frame'})
        with pytest.raises(ValueError, match='not both'):
            model(dict(batch, screen_surface=surf, **lin))


@pytest.mark.parametrize('lengths', [None, [1, 2]], ids=['uniform', 'ragged'])
def test_stream_steps_take_both_surfaces_in_two_chunks(fake, lengths):
    """camera_surface (NV12, pitched and cropped) + screen_surface (BGRA, pitched) equal camera_frame_nv12 + screen_frame_bgr on the
    linearised chunk, state included; render= on a screen_surface chunk is refused."""
    model = make_model(dict(CONFIGS['gru-cgru'][0], **SMALL_EYES))
    B, T = 2, 4
    batch = {k_: v for k_, v in clip(B, T, seed=3, size=SIZE).items() if k_ != 'screen_frame'}
    cl, cam, cam_lin = camera_surface_batch(batch, 'nv12', B, T, seed=11, warp_seed=12)
    sl, scr, scr_lin = screen_surface_pair('bgra', B, T, seed=13)
    model.eye_net.camera_layout, model.refine_net.screen_layout = cl, sl
    surf, lin = dict(cam, screen_surface=scr), dict(cam_lin, **scr_lin)
    assert set(lin) - set(surf) == {'camera_frame_nv12', 'screen_frame_bgr'}
    extra = ('camera_surface', 'screen_surface', 'camera_frame_nv12', 'screen_frame_bgr', 'left_eye_warp', 'right_eye_warp')
    part = lambda src, t0: dict(chunk_of(src, t0, t0 + 2), **{k_: src[k_][:, t0:t0 + 2].contiguous() for k_ in src if k_ in extra})
    a, b = eve_amd.EVEStream(model, B, use_graph=False), eve_amd.EVEStream(model, B, use_graph=False)
    for t0 in (0, 2):
        got = a.step(part(surf, t0), return_heatmaps=True, lengths=lengths)
        want = b.step(part(lin, t0), return_heatmaps=True, lengths=lengths)
        assert 'heatmap_final' in got and ('valid' in got) == (lengths is not None)
        same(got, want)
    sa, sb = a.get_state(), b.get_state()
    for key in sb:
        for x, y in zip(sa[key] if isinstance(sa[key], tuple) else (sa[key],), sb[key] if isinstance(sb[key], tuple) else (sb[key],)):
            assert torch.equal(x, y), key
    with pytest.raises(ValueError, match='one camera frame key'):
        a.step(dict(part(surf, 0), camera_frame_nv12=part(lin, 0)['camera_frame_nv12']))
    with pytest.raises(ValueError, match='not both'):
        a.step(dict(part(surf, 0), screen_frame_bgr=part(lin, 0)['screen_frame_bgr']))
    with pytest.raises(ValueError, match='screen_surface'):
        a.step(part(surf, 0), render=eve_amd.OverlaySpec())
    model.refine_net.screen_layout = None
    with pytest.raises(ValueError, match='screen_layout'):
        a.step(part(surf, 0))
    model.refine_net.screen_layout, model.eye_net.camera_layout = sl, None
    with pytest.raises(ValueError, match='camera_layout'):
        a.step(part(surf, 0))


def test_the_chunk_key_holds_both_layouts(fake):
    """A graph is keyed by the two layouts by value: an equal layout is a replay, another one another graph."""
    model = make_model(dict(CONFIGS['gru-cgru'][0], **SMALL_EYES))
    B, T = 2, 2
    batch = {k_: v for k_, v in clip(B, T, seed=3, size=SIZE).items() if k_ != 'screen_frame'}
    cl, cam, _ = camera_surface_batch(batch, 'nv12', B, T, seed=11, warp_seed=12)
    sl, scr, _ = screen_surface_pair('bgra', B, T, seed=13)
    ch = dict(chunk_of(cam, 0, T), camera_surface=cam['camera_surface'], left_eye_warp=cam['left_eye_warp'], right_eye_warp=cam['right_eye_warp'],
              screen_surface=scr)
    model.eye_net.camera_layout, model.refine_net.screen_layout = cl, sl
    stream = eve_amd.EVEStream(model, B, use_graph=False)
    captured = []
    stream._capture = lambda chunk, *a, **k_: captured.append(1) or {'n': len(captured)}
    first = stream._graph_for(ch, False)
    model.eye_net.camera_layout = padded('nv12', FRAME[1], FRAME[0])               # an equal layout: the same graph
    assert stream._graph_for(dict(ch), False) is first and len(captured) == 1
    # the same bytes per frame read as another format: the tensors' shapes do not change, the key does
    model.eye_net.camera_layout = SurfaceLayout('nv21', cl.width, cl.height, pitch=cl.pitch, coded_height=cl.coded_height, x0=cl.x0, y0=cl.y0,
                                                plane_offsets=cl.plane_offsets)
    assert model.eye_net.camera_layout.frame_bytes == cl.frame_bytes
    second = stream._graph_for(ch, False)
    assert second is not first and len(captured) == 2
    model.refine_net.screen_layout = SurfaceLayout('rgba', sl.width, sl.height, pitch=sl.pitch, coded_height=sl.coded_height, x0=sl.x0, y0=sl.y0)
    assert stream._graph_for(ch, False) is not second and len(captured) == 3 and len(stream._graphs) == 3
    model.eye_net.camera_layout, model.refine_net.screen_layout = cl, sl
    assert stream._graph_for(ch, False) is first and len(captured) == 3
