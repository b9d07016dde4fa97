"""CPU: NV12, I420 and YUYV screen captures -- the contract of eve_screen_area_fmt_to_nchw (tests/screen_format_ref.py) against an
independent brute-force evaluation and against the shortcut it must not be, the errors of the wrapper and of
data.preprocess_screen_frames, and the keys screen_frame_nv12 / _i420 / _yuyv through RefineNet, EVE and EVEStream on the torch-CPU
stand-in kernels.  tests/test_gpu_screen_formats.py checks the HIP kernel and the graph mode."""
import numpy as np
import pytest
import torch

import eve_amd
from eve_amd import data, kernels
from eve_amd.refine_net import SCREEN_FRAME_KEYS, screen_frame_key
import pixel_format_ref as pref
import screen_format_ref as fref
from test_pixel_format_host import PixelFakes, same
from test_stream_host import chunk_of, clip
from test_stream_ragged_host import CONFIGS, make_model

SCREEN = (72, 128)
CAPTURE = (144, 256)          # (IH, IW) of the captures the network-level tests feed


class ScreenFormatFakes(PixelFakes):
    screen_area_fmt_to_nchw = fref.screen_area_fmt_to_nchw


@pytest.fixture()
def fake():
    k = ScreenFormatFakes()
    kernels.set_default_kernels(k)
    yield k
    kernels.set_default_kernels(None)
    eve_amd.reset_standalone_config()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def capture(fmt, B, T, seed, hw=CAPTURE):
    """Random frames of the capture size in the layout of fmt -> uint8 [B, T, ...]."""
    v = pref.random_yuv_frames(fmt, B * T, hw[0], hw[1], seed)
    return torch.from_numpy(v).view((B, T) + v.shape[1:])


def converted(frames, fmt, matrix='bt601'):
    """[B, T, ...] of fmt -> the RGB capture uint8 [B, T, IH, IW, 3]."""
    B, T = frames.shape[:2]
    rgb = pref.to_rgb(frames.numpy().reshape((B * T,) + tuple(frames.shape[2:])), fmt, matrix)
    return torch.from_numpy(rgb).view((B, T) + rgb.shape[1:])


# ------------------------------------------------------------------------------------------------ the contract
SHAPES = [((2, 2), (1, 1)), ((10, 12), (3, 5)), ((30, 48), (2, 16))]


@pytest.mark.parametrize('fmt', fref.FORMATS)
@pytest.mark.parametrize('hw,out_hw', SHAPES, ids=['%dx%d-%dx%d' % (s + o) for s, o in SHAPES])
def test_the_contract_equals_a_brute_force_evaluation(fmt, hw, out_hw):
    matrices = list(pref.COEFFICIENTS) if hw == (30, 48) else ['bt601']
    buf = np.concatenate([pref.random_yuv_frames(fmt, 1, hw[0], hw[1], seed=hw[0] + hw[1]), pref.chroma_checkerboard(fmt, 1, hw[0], hw[1])])
    for matrix in matrices:
        got = fref.screen_area(buf, out_hw, fmt, matrix)
        assert got.dtype == np.float32 and got.shape == (2, 3) + out_hw and got.min() >= 0.0 and got.max() <= 1.0
        assert np.array_equal(bits(got), bits(fref.brute_force(buf, out_hw, fmt, matrix))), matrix


def test_the_header_constants_are_the_reference_constants():
    for matrix in pref.COEFFICIENTS:
        assert fref.HEADER_CONSTANTS[matrix] == pref.constants(matrix)


@pytest.mark.parametrize('fmt', fref.FORMATS)
def test_averaging_before_converting_is_seen_by_the_test_frames(fmt):
    """On the chroma checkerboard every converted pixel is clamped in red and blue, so the mean of the converted pixels and the
    conversion of the mean planes (grey) differ at every output; a kernel that took the shortcut could not pass."""
    buf = pref.chroma_checkerboard(fmt, 2, 30, 48)
    want, short = fref.screen_area(buf, (2, 16), fmt), fref.average_then_convert(buf, (2, 16), fmt)
    assert want.shape == short.shape and (bits(want)[:, [0, 2]] != bits(short)[:, [0, 2]]).all()
    rnd = pref.random_yuv_frames(fmt, 2, 30, 48, seed=1)
    assert not np.array_equal(bits(fref.screen_area(rnd, (2, 16), fmt)), bits(fref.average_then_convert(rnd, (2, 16), fmt)))


def test_constant_frames_give_exact_values():
    for fmt in fref.FORMATS:
        black = fref.screen_area(pref.constant_frames(fmt, 1, 10, 12, 16, 128, 128), (3, 5), fmt)
        white = fref.screen_area(pref.constant_frames(fmt, 1, 10, 12, 235, 128, 128), (3, 5), fmt)
        assert (bits(black) == 0).all() and (white == np.float32(255.0) * np.float32(1.0 / 255.0)).all()


# ------------------------------------------------------------------------------------------------ the wrapper and data.py
def test_the_wrapper_checks_its_arguments(fake):
    nv12 = capture('nv12', 1, 2, seed=1)[0]
    for k in (fake, kernels.HipKernels.__new__(kernels.HipKernels)):      # the stand-in and the real wrapper: refused before the library is touched
        with pytest.raises(ValueError, match='matrix'):
            k.screen_area_fmt_to_nchw(nv12, SCREEN, 'nv12', matrix='nonsense')
        with pytest.raises(ValueError):
            k.screen_area_fmt_to_nchw(nv12, SCREEN, 'nv21')
        with pytest.raises(ValueError):
            k.screen_area_fmt_to_nchw(nv12[:, :-1], SCREEN, 'nv12')                       # 215 rows: no IH * 3 / 2
        with pytest.raises(ValueError):
            k.screen_area_fmt_to_nchw(torch.zeros((1, 4, 5, 2), dtype=torch.uint8), (2, 2), 'yuyv')      # odd width
        with pytest.raises(TypeError):
            k.screen_area_fmt_to_nchw(nv12.float(), SCREEN, 'nv12')
        with pytest.raises(TypeError):
            k.screen_area_fmt_to_nchw(nv12[0], SCREEN, 'nv12')
        with pytest.raises(RuntimeError, match='non-contiguous'):
            k.screen_area_fmt_to_nchw(torch.zeros((2, 216, 512), dtype=torch.uint8)[:, :, ::2], SCREEN, 'nv12')
        with pytest.raises(ValueError):
            k.screen_area_fmt_to_nchw(torch.zeros((1, 4, 4, 3), dtype=torch.uint8), (2, 2), 'rgb')


@pytest.mark.parametrize('fmt', fref.FORMATS)
def test_preprocess_screen_frames_takes_a_format(fake, fmt):
    cap = capture(fmt, 2, 2, seed=3)
    got = data.preprocess_screen_frames(cap, size=SCREEN, format=fmt, matrix='bt709')
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 2, 3) + SCREEN
    assert torch.equal(got, data.preprocess_screen_frames(converted(cap, fmt, 'bt709'), size=SCREEN))
    assert not torch.equal(got, data.preprocess_screen_frames(cap, size=SCREEN, format=fmt))            # the matrix is read
    assert torch.equal(data.preprocess_screen_frames(cap[1], size=SCREEN, format=fmt, matrix='bt709'), got[1])
    own = data.preprocess_screen_frames(cap, format=fmt)                                                # size=None: the frames' own
    assert tuple(own.shape) == (2, 2, 3) + CAPTURE
    assert np.array_equal(bits(own.numpy()), bits(converted(cap, fmt).numpy().transpose(0, 1, 4, 2, 3).astype(np.float32) * np.float32(1.0 / 255.0)))


def test_preprocess_screen_frames_errors(fake):
    nv12 = capture('nv12', 1, 2, seed=1)
    with pytest.raises(ValueError, match='bgr'):
        data.preprocess_screen_frames(nv12, size=SCREEN, bgr=True, format='nv12')
    with pytest.raises(ValueError, match='format'):
        data.preprocess_screen_frames(nv12, size=SCREEN, format='nv21')
    with pytest.raises(ValueError, match='format'):
        data.preprocess_screen_frames(nv12, size=SCREEN, format='bgr')                   # BGR goes through bgr=True
    with pytest.raises(ValueError, match='matrix'):
        data.preprocess_screen_frames(nv12, size=SCREEN, format='nv12', matrix='nonsense')
    with pytest.raises(ValueError):
        data.preprocess_screen_frames(nv12[:, :, :-1], size=SCREEN, format='nv12')
    with pytest.raises(TypeError):
        data.preprocess_screen_frames(nv12.float(), size=SCREEN, format='nv12')
    with pytest.raises((ValueError, RuntimeError)):
        data.preprocess_screen_frames(capture('nv12', 1, 1, seed=1, hw=(60, 128)), size=SCREEN, format='nv12')     # 60 rows -> 72


# ------------------------------------------------------------------------------------------------ RefineNet / EVE / EVEStream
def test_the_screen_keys_mirror_the_camera_keys():
    assert SCREEN_FRAME_KEYS == {'screen_frame': 'rgb', 'screen_frame_bgr': 'bgr', 'screen_frame_nv12': 'nv12', 'screen_frame_i420': 'i420',
                                 'screen_frame_yuyv': 'yuyv'}
    assert {k_.replace('screen', 'camera'): v for k_, v in SCREEN_FRAME_KEYS.items()} == eve_amd.eye_net.EYE_FRAME_KEYS
    assert screen_frame_key({}) is None and screen_frame_key({'screen_frame_i420': 0, 'camera_frame_nv12': 0}) == 'screen_frame_i420'
    with pytest.raises(ValueError, match='not both'):
        screen_frame_key({'screen_frame_nv12': 0, 'screen_frame_yuyv': 0})
    assert eve_amd.RefineNet.yuv_matrix == 'bt601'


@pytest.mark.parametrize('fmt', fref.FORMATS)
def test_refinenet_takes_the_capture_as_the_decoder_delivers_it(fake, fmt):
    model = make_model(*CONFIGS['gru-cgru'])
    B, T = 1, 2
    heat = torch.rand((B, T, 1) + SCREEN, generator=torch.Generator().manual_seed(5))
    cap = capture(fmt, B, T, seed=7)
    key = 'screen_frame_' + fmt
    with torch.no_grad():
        got, gst = model.refine_net.forward_sequence(heat, **{key: cap})
        want, wst = model.refine_net.forward_sequence(heat, converted(cap, fmt))
        assert tuple(got.shape) == (B, T, 1) + SCREEN and torch.equal(got, want)
        for a, b in zip(gst, wst):
            assert torch.equal(a, b)
        model.refine_net.yuv_matrix = 'bt709'                    # the matrix is the module's attribute
        hd, _ = model.refine_net.forward_sequence(heat, **{key: cap})
        hd_want, _ = model.refine_net.forward_sequence(heat, converted(cap, fmt, 'bt709'))
        assert torch.equal(hd, hd_want) and not torch.equal(hd, got)
        model.refine_net.yuv_matrix = 'nonsense'
        with pytest.raises(ValueError, match='yuv_matrix'):
            model.refine_net.forward_sequence(heat, **{key: cap})
        model.refine_net.forward_sequence(heat, converted(cap, fmt))          # ... which the RGB key never reads
        model.refine_net.yuv_matrix = 'bt601'
        with pytest.raises(ValueError, match='not both'):
            model.refine_net.forward_sequence(heat, converted(cap, fmt), **{key: cap})
        with pytest.raises(ValueError, match='not both'):
            model.refine_net.forward_sequence(heat, screen_frame_bgr=converted(cap, fmt), **{key: cap})
        with pytest.raises(TypeError, match=key):
            model.refine_net.forward_sequence(heat, **{key: cap.float()})
        with pytest.raises(ValueError, match=key):                # an odd size: 215 rows are no IH * 3 / 2, 255 pixels no pairs
            model.refine_net.forward_sequence(heat, **{key: cap[:, :, :, :-1] if fmt == 'yuyv' else cap[:, :, :-1]})


def test_eve_eval_takes_the_capture_and_does_not_echo_it(fake):
    model = make_model(*CONFIGS['gru-cgru'])
    batch = {k_: v for k_, v in clip(1, 2, seed=3).items() if k_ != 'screen_frame'}
    cap = capture('nv12', 1, 2, seed=9)
    with torch.no_grad():
        got = model(dict(batch, screen_frame_nv12=cap), create_images=True)
        want = model(dict(batch, screen_frame=converted(cap, 'nv12')), create_images=True)
    assert 'screen_frame' in want and 'screen_frame' not in got and not any(k_.startswith('screen_frame_') for k_ in got)
    for key in ('PoG_px_final', 'g_final', 'PoG_px_initial', 'final_heatmap', 'full_loss'):
        assert torch.equal(got[key], want[key]), key
    with pytest.raises(ValueError, match='not both'):
        model(dict(batch, screen_frame_nv12=cap, screen_frame_i420=cap))
    with pytest.raises(ValueError, match='not both'):
        model(dict(batch, screen_frame_nv12=cap, screen_frame=converted(cap, 'nv12')))


@pytest.mark.parametrize('fmt,lengths', [('nv12', None), ('nv12', [1, 2]), ('i420', [2, 0]), ('yuyv', None)])
def test_stream_steps_take_the_capture_in_two_chunks(fake, fmt, lengths):
    model = make_model(*CONFIGS['gru-cgru'])
    B, T = 2, 4
    batch = {k_: v for k_, v in clip(B, T, seed=3).items() if k_ != 'screen_frame'}
    cap = capture(fmt, B, T, seed=11)
    rgb = converted(cap, fmt)
    a, b = eve_amd.EVEStream(model, B, use_graph=False), eve_amd.EVEStream(model, B, use_graph=False)
    fake.calls.clear()
    for t0 in (0, 2):
        ch = chunk_of(batch, t0, t0 + 2)
        got = a.step(dict(ch, **{'screen_frame_' + fmt: cap[:, t0:t0 + 2].contiguous()}), return_heatmaps=True, lengths=lengths)
        want = b.step(dict(ch, screen_frame=rgb[:, t0:t0 + 2].contiguous()), return_heatmaps=True, lengths=lengths)
        assert 'heatmap_final' in got and ('valid' in got) == (lengths is not None)
        same(got, want)
    sa, sb = a.get_state(), b.get_state()
    for key in sb:
        for x, y in zip(sa[key] if isinstance(sa[key], tuple) else (sa[key],), sb[key] if isinstance(sb[key], tuple) else (sb[key],)):
            assert torch.equal(x, y), key
    ch = chunk_of(batch, 0, 2)
    with pytest.raises(ValueError, match='not both'):
        a.step(dict(ch, screen_frame_nv12=capture('nv12', B, 2, seed=1), screen_frame_yuyv=capture('yuyv', B, 2, seed=1)))
    with pytest.raises(ValueError, match='not both'):
        a.step(dict(ch, screen_frame=rgb[:, :2].contiguous(), **{'screen_frame_' + fmt: cap[:, :2].contiguous()}))


def test_the_chunk_key_holds_the_screen_matrix(fake):
    """A graph is keyed by refine_net.yuv_matrix beside eye_net.yuv_matrix: another matrix is another graph, the same one a replay."""
    model = make_model(*CONFIGS['gru-cgru'])
    batch = {k_: v for k_, v in clip(2, 2, seed=3).items() if k_ != 'screen_frame'}
    ch = dict(chunk_of(batch, 0, 2), screen_frame_nv12=capture('nv12', 2, 2, seed=1))
    stream = eve_amd.EVEStream(model, 2, use_graph=False)
    captured = []
    stream._capture = lambda chunk, *a, **k_: captured.append(model.refine_net.yuv_matrix) or {'matrix': model.refine_net.yuv_matrix}
    first = stream._graph_for(ch, False)
    assert stream._graph_for(dict(ch), False) is first and captured == ['bt601']
    model.refine_net.yuv_matrix = 'bt709'
    hd = stream._graph_for(ch, False)
    assert hd is not first and captured == ['bt601', 'bt709'] and len(stream._graphs) == 2
    model.refine_net.yuv_matrix = 'bt601'
    assert stream._graph_for(ch, False) is first and len(captured) == 2
    assert all('bt709' in key or 'bt601' in key for key in stream._graphs)
