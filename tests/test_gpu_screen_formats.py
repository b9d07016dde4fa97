"""GPU: eve_screen_area_fmt_to_nchw (csrc/screen_resize.hip) bit for bit against its contract in numpy (tests/screen_format_ref.py:
the area average of the frame pixel_format_ref.to_rgb converts) for NV12, I420 and YUYV captures, in the vector and the byte form;
the BGR(A) codes against eve_screen_u8_area_bgr_to_nchw; the refusals; and the keys screen_frame_nv12 / _i420 through EVEStream
under graph replay against screen_frame on the converted capture.

Frames: uniform random bytes whose converted frame holds 0 and 255 in every channel (both clamps act; the seeds were searched
for that on the CPU, and every test asserts it), the chroma checkerboard (a chroma index off by one, or averaging before converting,
changes every output), and constant frames with exactly known results."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import eve_amd
from eve_amd.kernels import PIXEL_FORMATS, YUV_MATRICES, default_kernels
import pixel_format_ref as pref
import screen_format_ref as fref
from test_gpu_pixel_formats import both_forms, same
from test_gpu_stream import gpu_clip, make_model

pytestmark = pytest.mark.gpu
SCREEN = (72, 128)
GUARD = 1024                  # floats behind the output that no launch may touch
SENTINEL = -7.0

# (N, IH, IW, OH, OW, the form that takes it): True reads 16-byte vectors, False single bytes
CASES = [
    (3, 2, 2, 1, 1, False),                    # one chroma sample, the byte form
    (3, 10, 12, 3, 5, False),                  # the byte form, fractional on both axes
    (3, 18, 32, 5, 7, True),                   # the vector form, source rows shared by two output rows
    (3, 30, 48, 2, 16, True),                  # output row 1 begins on odd source row 15; three columns per output across chroma pairs
    (3, 72, 128, 72, 128, True),               # conversion only
    (1, 768, 1366, 72, 128, False),            # a width that is no multiple of 16, I420 chroma rows of 683 bytes
    (2, 1080, 1920, 72, 128, True),            # the real case
    (2100, 4, 16, 2, 8, True),                 # 4 200 items, past the grid's 4 096: the grid-stride loop
]
IDS = ['%dx%dx%d-%dx%d' % c[:5] for c in CASES]
# random_yuv_frames seeds whose converted frames hold 0 and 255 in every channel under all three matrices, per (format, N, IH, IW):
# the 2 x 2 frames (one chroma sample each) needed a search, every other shape of this file does so with seed 0
SEEDS = {('nv12', 3, 2, 2): 1, ('i420', 3, 2, 2): 1, ('yuyv', 3, 2, 2): 3}


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def raw_call(k, fmt, matrix, N, IH, IW, frames, out_hw, out):
    return k.lib.eve_screen_area_fmt_to_nchw(PIXEL_FORMATS[fmt], YUV_MATRICES[matrix], N, IH, IW, ptr(frames), out_hw[0], out_hw[1], ptr(out),
                                             stream_ptr())


def kernel_name(fmt, vec):
    return ('screen_area_fmt_kernel<%s,%s>' % (fmt, 'true' if vec else 'false')).encode()


def random_frames(fmt, N, IH, IW, matrices=('bt601',)):
    buf = pref.random_yuv_frames(fmt, N, IH, IW, SEEDS.get((fmt, N, IH, IW), 0))
    for matrix in matrices:
        assert fref.both_clamps(buf, fmt, matrix), (fmt, N, IH, IW, matrix)
    return buf


def check(k, buf, fmt, out_hw, vec, matrix='bt601', frames=None):
    """Two launches into a guarded buffer, each == the numpy contract with no tolerance; the guard untouched; the kernel's name.
    -> (the frames on the GPU, want)."""
    N = buf.shape[0]
    IH, IW = pref.frame_hw(buf.shape, fmt)
    want = torch.from_numpy(fref.screen_area(buf, out_hw, fmt, matrix))
    n_out = want.numel()
    frames = torch.from_numpy(buf).cuda() if frames is None else frames
    for _ in range(2):
        out = torch.full((n_out + GUARD,), SENTINEL, dtype=torch.float32, device='cuda')
        assert raw_call(k, fmt, matrix, N, IH, IW, frames, out_hw, out) == 0, k.lib.eve_last_error()
        assert k.lib.eve_last_kernel() == kernel_name(fmt, vec)
        got = out.cpu()
        assert torch.equal(got[n_out:], torch.full((GUARD,), SENTINEL)), 'guard overwritten'
        got = got[:n_out].view(N, 3, out_hw[0], out_hw[1])
        bad = got.view(torch.int32) != want.view(torch.int32)
        assert not bad.any(), ('%d of %d outputs differ, first at %s: got %r want %r' % (
            int(bad.sum()), n_out, tuple(bad.nonzero()[0].tolist()), float(got[bad][0]), float(want[bad][0])))
    return frames, want


@pytest.mark.parametrize('fmt', fref.FORMATS)
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_kernel_equals_the_contract(case, fmt):
    N, IH, IW, OH, OW, vec = case
    k = default_kernels()
    frames, want = check(k, random_frames(fmt, N, IH, IW), fmt, (OH, OW), vec)
    check(k, pref.chroma_checkerboard(fmt, N, IH, IW), fmt, (OH, OW), vec)
    via = k.screen_area_fmt_to_nchw(frames, (OH, OW), fmt)                  # the tensor-level wrapper
    assert via.dtype == torch.float32 and tuple(via.shape) == (N, 3, OH, OW) and torch.equal(via.cpu(), want)
    if (IH, IW) == (OH, OW):                                                # conversion only: the plain normalisation of to_rgb
        rgb = torch.from_numpy(pref.to_rgb(frames.cpu().numpy(), fmt)).cuda()
        assert torch.equal(via, k.frames_u8_to_nchw(rgb, 1.0 / 255.0, None))


@pytest.mark.parametrize('fmt', fref.FORMATS)
def test_every_matrix(fmt):
    k = default_kernels()
    buf = random_frames(fmt, 3, 30, 48, matrices=tuple(YUV_MATRICES))
    wants = [check(k, buf, fmt, (2, 16), True, matrix)[1] for matrix in YUV_MATRICES]
    assert not torch.equal(wants[0], wants[1]) and not torch.equal(wants[0], wants[2]) and not torch.equal(wants[1], wants[2])
    for matrix in ('bt709', 'jfif'):
        check(k, pref.chroma_checkerboard(fmt, 3, 30, 48), fmt, (2, 16), True, matrix)


@pytest.mark.parametrize('fmt', fref.FORMATS)
@pytest.mark.parametrize('hw,out_hw,vec', [((10, 12), (3, 5), False), ((18, 32), (5, 7), True)], ids=['bytes', 'vector'])
def test_constant_frames_give_exact_values(fmt, hw, out_hw, vec):
    """(16, 128, 128) under bt601 is exactly 0.0 and (235, 128, 128) what the RGB kernel gives on a constant 255."""
    k = default_kernels()
    _, black = check(k, pref.constant_frames(fmt, 3, hw[0], hw[1], 16, 128, 128), fmt, out_hw, vec)
    assert (black.view(torch.int32) == 0).all()
    frames, white = check(k, pref.constant_frames(fmt, 3, hw[0], hw[1], 235, 128, 128), fmt, out_hw, vec)
    rgb = torch.full((3, hw[0], hw[1], 3), 255, dtype=torch.uint8, device='cuda')
    assert torch.equal(k.screen_u8_area_to_nchw(rgb, out_hw).cpu(), white)


@pytest.mark.parametrize('fmt', fref.FORMATS)
def test_unaligned_base_takes_the_byte_form(fmt):
    """A width that is a multiple of 16 behind a base two bytes into a larger buffer must not be read as vectors: same bits."""
    k = default_kernels()
    v = random_frames(fmt, 3, 18, 32)
    big = torch.zeros((v.size + 16,), dtype=torch.uint8, device='cuda')
    frames = big[2:2 + v.size].view(v.shape)
    frames.copy_(torch.from_numpy(v))
    assert frames.data_ptr() % 16 == 2 and frames.is_contiguous()
    _, want = check(k, v, fmt, (5, 7), False, frames=frames)
    aligned, same_bits = check(k, v, fmt, (5, 7), True)
    assert torch.equal(want, same_bits)
    assert torch.equal(k.screen_area_fmt_to_nchw(frames, (5, 7), fmt), k.screen_area_fmt_to_nchw(aligned, (5, 7), fmt))


@pytest.mark.parametrize('shape,vec', [((90, 160, 3), True), ((100, 171, 4), False)], ids=['bgr', 'bgra'])
def test_the_bgr_codes_go_to_the_bgr_kernel(shape, vec):
    k = default_kernels()
    cap = torch.from_numpy(np.random.default_rng(shape[1]).integers(0, 256, size=(2,) + shape, dtype=np.uint8)).cuda()
    want = k.screen_u8_area_bgr_to_nchw(cap, SCREEN)
    n_out = want.numel()
    out = torch.full((n_out + GUARD,), SENTINEL, dtype=torch.float32, device='cuda')
    code = PIXEL_FORMATS['bgra' if shape[2] == 4 else 'bgr']
    assert k.lib.eve_screen_area_fmt_to_nchw(code, 99, 2, shape[0], shape[1], ptr(cap), SCREEN[0], SCREEN[1], ptr(out), stream_ptr()) == 0   # (matrix ignored)
    assert k.lib.eve_last_kernel() == (b'screen_u8_area_bgr_kernel<true>' if vec else b'screen_u8_area_bgr_kernel<false>')
    assert (out[n_out:] == SENTINEL).all() and torch.equal(out[:n_out].view(torch.int32), want.reshape(-1).view(torch.int32))
    assert torch.equal(k.screen_area_fmt_to_nchw(cap, SCREEN, 'bgr'), want)


def test_refused_requests_launch_nothing():
    k = default_kernels()
    frames = torch.zeros((1, 135, 160), dtype=torch.uint8, device='cuda')          # 90 x 160 as NV12 / I420; YUYV reads 90 x 120 of it
    k.stream_state_rows(torch.zeros((2, 8), device='cuda'), torch.zeros((2, 8), device='cuda'))     # the last named launch
    before = k.lib.eve_last_kernel()
    assert b'screen' not in before
    out = torch.full((3 * 72 * 128 + GUARD,), SENTINEL, dtype=torch.float32, device='cuda')
    p, o, F, M = ptr(frames), ptr(out), PIXEL_FORMATS, YUV_MATRICES
    call = lambda fmt, mat, N, IH, IW, OH, OW, a=p, b=o: k.lib.eve_screen_area_fmt_to_nchw(fmt, mat, N, IH, IW, a, OH, OW, b, stream_ptr())
    cases = {'no frames': ((F['nv12'], 0, 0, 90, 160, 72, 128), 'bad arguments'), 'no rows': ((F['yuyv'], 0, 1, 0, 160, 72, 128), 'bad arguments'),
             'format': ((7, 0, 1, 90, 160, 72, 128), 'unknown format'), 'negative format': ((-1, 0, 1, 90, 160, 72, 128), 'unknown format'),
             'matrix': ((F['nv12'], 3, 1, 90, 160, 72, 128), 'unknown matrix'), 'negative matrix': ((F['yuyv'], -1, 1, 90, 120, 72, 120), 'unknown matrix'),
             'nv12 odd rows': ((F['nv12'], 0, 1, 91, 160, 72, 128), 'even'), 'i420 odd width': ((F['i420'], 0, 1, 90, 159, 72, 128), 'even'),
             'yuyv odd width': ((F['yuyv'], 0, 1, 90, 119, 72, 100), 'even'),
             'rows upscaled': ((F['nv12'], 0, 1, 60, 160, 72, 128), 'upscaling'), 'columns upscaled': ((F['i420'], 0, 1, 90, 100, 72, 128), 'upscaling'),
             'oversize': ((F['nv12'], 0, 1, 4106, 4104, 72, 128), 'too large'), 'row too wide': ((F['yuyv'], 0, 1, 72, 13656, 72, 128), 'too wide'),
             'items': ((F['i420'], 0, 29826162, 90, 160, 72, 128), '31 bits'),
             'bgr upscaled': ((F['bgr'], 0, 1, 20, 160, 72, 128), 'upscaling'), 'bgra no frames': ((F['bgra'], 0, 0, 20, 160, 72, 128), 'bad arguments')}
    for name, (args, word) in cases.items():
        assert call(*args) != 0, name
        msg = k.lib.eve_last_error().decode()
        assert msg.startswith('screen_area_fmt_to_nchw:') and word in msg, (name, msg)
        assert k.lib.eve_last_kernel() == before, name
    for fmt in ('nv12', 'bgr'):
        assert call(F[fmt], 0, 1, 90, 160, 72, 128, None, o) != 0 and call(F[fmt], 0, 1, 90, 160, 72, 128, p, None) != 0
        assert k.lib.eve_last_error().decode().startswith('screen_area_fmt_to_nchw: bad arguments') and k.lib.eve_last_kernel() == before
    with pytest.raises(RuntimeError, match='upscaling'):
        k.screen_area_fmt_to_nchw(frames, (91, 128), 'nv12')
    with pytest.raises(ValueError, match='matrix'):
        k.screen_area_fmt_to_nchw(frames, SCREEN, 'nv12', matrix='nonsense')
    with pytest.raises(RuntimeError, match='non-contiguous'):
        k.screen_area_fmt_to_nchw(torch.zeros((1, 135, 320), dtype=torch.uint8, device='cuda')[:, :, ::2], SCREEN, 'nv12')
    assert k.lib.eve_last_kernel() == before
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.full((out.numel(),), SENTINEL))
    assert call(F['nv12'], M['jfif'], 1, 90, 160, 72, 128) == 0                     # the same call with sound arguments is taken: a zero
    want = pref.yuv_to_rgb(np.uint8(0), np.uint8(0), np.uint8(0), 'jfif').astype(np.float32) * np.float32(1.0 / 255.0)  # frame, a green
    got = out[:3 * 72 * 128].view(3, -1).cpu()
    assert all((got[c] == float(want[c])).all() for c in range(3)) and (out[3 * 72 * 128:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ EVEStream
@functools.lru_cache(maxsize=None)
def screens(fmt, seed, B=2, T=6, hw=(144, 256)):
    """-> (the capture uint8 [B, T, ...] of fmt, the converted RGB capture uint8 [B, T, IH, IW, 3]), both on the GPU."""
    buf = pref.random_yuv_frames(fmt, B * T, hw[0], hw[1], seed)
    rgb = pref.to_rgb(buf, fmt)
    return torch.from_numpy(buf).view((B, T) + buf.shape[1:]).cuda(), torch.from_numpy(rgb).view((B, T) + rgb.shape[1:]).cuda()


def test_stream_replays_a_graph_over_an_nv12_capture():
    """bf16, B = 2, Tc = 2, 144 x 256 captures as screen_frame_nv12: three steps with different frames, the last with lengths, equal
    the eager stream fed screen_frame = to_rgb(...) in every returned tensor; the second step replays the first step's graph."""
    model, _ = make_model(dtype=torch.bfloat16)
    _, d, _ = gpu_clip(2, 6, seed=5)
    rest = {k_: v for k_, v in d.items() if k_ != 'screen_frame'}
    raw, rgb = screens('nv12', 41)
    ch = lambda src, i: {k_: v[:, 2 * i:2 * i + 2].contiguous() for k_, v in src.items()}
    g, e = eve_amd.EVEStream(model, 2), eve_amd.EVEStream(model, 2, use_graph=False)
    outs = []
    for i, lengths in enumerate((None, None, [1, 2])):
        og = {k_: v.clone() for k_, v in g.step(ch(dict(rest, screen_frame_nv12=raw), i), return_heatmaps=True, lengths=lengths).items()}
        same(og, e.step(ch(dict(rest, screen_frame=rgb), i), return_heatmaps=True, lengths=lengths), i)
        assert 'heatmap_final' in og and ('valid' in og) == (lengths is not None)
        outs.append(og)
        assert len(g._graphs) == (1 if i < 2 else 2)                  # the second step reuses the first step's graph
    assert not torch.equal(outs[0]['heatmap_final'], outs[1]['heatmap_final'])
    entry = next(iter(g._graphs.values()))
    assert entry['inputs']['screen_frame_nv12'].numel() * 2 == rgb[:, :2].numel() and 'screen_frame' not in entry['inputs']
    with pytest.raises(ValueError, match='not both'):
        g.step(ch(dict(d, screen_frame_nv12=raw), 0))


def test_stream_takes_an_i420_screen_beside_an_nv12_camera():
    model, _ = make_model(dtype=torch.bfloat16)
    _, d, _ = gpu_clip(2, 2, seed=5)
    cam_raw, cam_rgb = both_forms({k_: v for k_, v in d.items() if k_ != 'screen_frame'}, 'nv12', 33, 2)
    raw, rgb = screens('i420', 42)
    g, e = eve_amd.EVEStream(model, 2), eve_amd.EVEStream(model, 2, use_graph=False)
    got = g.step(dict(cam_raw, screen_frame_i420=raw[:, :2].contiguous()), return_heatmaps=True)
    same(got, e.step(dict(cam_rgb, screen_frame=rgb[:, :2].contiguous()), return_heatmaps=True))
    assert len(g._graphs) == 1 and 'heatmap_final' in got
