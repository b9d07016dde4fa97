"""GPU: eve_eye_warp_surface_to_nchw / _to_stem (csrc/eye_warp.hip) and eve_screen_area_surface_to_nchw (csrc/screen_resize.hip) bit
for bit against the existing format entry points on the linearised frame (tests/surface_ref.linear) and against the numpy contracts
of tests/pixel_format_ref.py, for every SurfaceLayout format, in the vector and in the byte form; padding that is never read; the
form that ran; a lens and an eye_pose case; more items than the grid; 64-bit frame strides; every refusal; and camera_surface /
screen_surface through EVEStream under graph replay.  Everything is exact: there is no tolerance in this file.

Shapes: visible 64 x 48 at crop (x0, y0) = (2, 4) inside rows of 96 pixels and 56 coded rows (every pitch a multiple of 8 bytes: the
vector form of the 4:2:0 layouts, with a skew of 2), and visible 70 x 46 inside rows of 100 pixels (NV12 / I420 pitches of 100 and
50 bytes: the byte form).  Patches of 24 x 32 from eye_warp_ref.WARPS plus the NaN and the off-frame matrix, one frame per matrix;
screen targets 16 x 9 (fractional ratios) and 8 x 6 (64 x 48: integer ratios)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import eve_amd
from eve_amd import data
from eve_amd.data import SurfaceLayout
from eve_amd.kernels import default_kernels, dt_code
import eye_warp_lens_ref as lref
import eye_warp_ref as ref
import pixel_format_ref as pref
import screen_resize_ref as rref
import surface_ref as sref
from test_gpu_eye_pose import cam_poses
from test_gpu_eye_warp import BAND, CAM, GRID_CAP, GUARD, SENTINEL, SENTINEL16, camera_clip, differing, stream_ptr
from test_gpu_stream import gpu_clip, make_model

pytestmark = pytest.mark.gpu
TYPE_NAMES = {torch.float32: 'float', torch.bfloat16: 'eve::bf16_t', torch.float16: 'eve::f16_t'}
PATCH = (24, 32)
TARGETS = ((9, 16), (6, 8))
MATRICES = np.stack([m for m, _ in ref.WARPS.values()] + [ref.NAN_WARP, ref.OFF_FRAME_WARP])
YUV420 = ('nv12', 'nv21', 'i420', 'yv12')


def layout_of(fmt, which):
    bpp = sref.BYTES_PER_PIXEL[fmt]
    if which == 'vec':
        return SurfaceLayout(fmt, 64, 48, pitch=96 * bpp, coded_height=56, x0=2, y0=4)
    return SurfaceLayout(fmt, 70, 46, pitch=100 * bpp)


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def warp_name(layout, lens, dtype):
    return ('eye_warp_surface_kernel<%s,%s,%s>' % (layout.kind, 'lens' if lens else 'plain', TYPE_NAMES[dtype])).encode()


def screen_name(fmt, vec):
    return ('screen_area_surface_kernel<%s>' % ('yuv420,' + ('true' if vec else 'false') if fmt in YUV420 else 'generic,false')).encode()


def raw_warp(k, surf, mat, N, frames, warps, lens, hw, out, dtype=torch.float32):
    if dtype == torch.float32:
        return k.lib.eve_eye_warp_surface_to_nchw(ctypes.byref(surf), mat, N, ptr(frames), ptr(warps), ptr(lens), hw[0], hw[1], ptr(out), stream_ptr())
    return k.lib.eve_eye_warp_surface_to_stem(dt_code(dtype), ctypes.byref(surf), mat, N, ptr(frames), ptr(warps), ptr(lens), hw[0], hw[1], ptr(out),
                                              stream_ptr())


def raw_screen(k, surf, mat, N, frames, hw, out):
    return k.lib.eve_screen_area_surface_to_nchw(ctypes.byref(surf), mat, N, ptr(frames), hw[0], hw[1], ptr(out), stream_ptr())


def linear_warp(k, lin, fmt, warps, hw, matrix='bt601', lens=None, dtype=torch.float32):
    """The existing entry points on the linearised frames (a GPU tensor of LINEAR_FORMAT fmt) -> the float or the packed form."""
    if fmt != 'rgb':
        if dtype == torch.float32:
            return k.eye_warp_fmt_to_nchw(lin, warps, hw, fmt, matrix=matrix, lens=lens)
        return k.eye_warp_fmt_to_stem(lin, warps, hw, fmt, matrix=matrix, lens=lens, dtype=dtype)
    if dtype == torch.float32:
        return k.eye_warp_u8_to_nchw(lin, warps, hw) if lens is None else k.eye_warp_lens_u8_to_nchw(lin, warps, lens, hw)
    return k.eye_warp_u8_to_stem(lin, warps, hw, dtype=dtype) if lens is None else k.eye_warp_lens_u8_to_stem(lin, warps, lens, hw, dtype=dtype)


def linear_screen(k, lin, fmt, hw, matrix='bt601'):
    return k.screen_u8_area_to_nchw(lin, hw) if fmt == 'rgb' else k.screen_area_fmt_to_nchw(lin, hw, fmt, matrix=matrix)


def rgb_of(lin, fmt, matrix='bt601'):
    return np.asarray(lin) if fmt == 'rgb' else pref.to_rgb(lin, fmt, matrix)


@functools.lru_cache(maxsize=None)
def case(fmt, which):
    """One surface case, computed once and never modified -> (layout, buf uint8 [7, frame_bytes] of random bytes, its linear frames,
    their format, the numpy patches of MATRICES, the numpy screens of TARGETS)."""
    L = layout_of(fmt, which)
    buf, lin = sref.random_surface(L, len(MATRICES), seed=len(fmt) + len(which))
    lin_fmt = sref.LINEAR_FORMAT[fmt]
    rgb = rgb_of(lin, lin_fmt)
    patches = ref.eye_warp(rgb, MATRICES, PATCH)[0]
    screens = tuple(rref.area_resize(rgb, hw) for hw in TARGETS)
    return L, buf, lin, lin_fmt, patches, screens


def equal_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    view = torch.int32 if got.dtype == torch.float32 else torch.int16
    g, w = got.contiguous().view(view).reshape(-1).cpu(), want.contiguous().view(view).reshape(-1).cpu()
    assert torch.equal(g, w), (what, differing(g, w))


# ------------------------------------------------------------------------------------------------ identity, every format, both forms
@pytest.mark.parametrize('which', ['vec', 'byte'])
@pytest.mark.parametrize('fmt', sref.FORMATS)
def test_the_warp_equals_the_format_call_on_the_linearised_frame(fmt, which):
    """Float and both packed forms, raw calls into guarded buffers: == the existing entry point on linear(buf), == numpy; the
    kernel's documented name; then the tensor-level wrapper and data.warp_eye_patches."""
    k = default_kernels()
    L, buf, lin, lin_fmt, patches, _ = case(fmt, which)
    N = len(MATRICES)
    frames, lin_gpu, warps = torch.from_numpy(buf).cuda(), torch.from_numpy(lin).cuda(), torch.from_numpy(MATRICES).cuda()
    surf = L.as_ctypes()
    want = torch.from_numpy(patches)
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        wp = want if dtype == torch.float32 else ref.pack_stem(want, dtype)
        n_out = wp.numel()
        store = torch.float32 if dtype == torch.float32 else torch.int16
        out = torch.full((n_out + GUARD,), SENTINEL if dtype == torch.float32 else SENTINEL16, dtype=store, device='cuda')
        assert raw_warp(k, surf, 0, N, frames, warps, None, PATCH, out, dtype) == 0, k.lib.eve_last_error()
        assert k.lib.eve_last_kernel() == warp_name(L, False, dtype)
        assert (out[n_out:] == (SENTINEL if dtype == torch.float32 else SENTINEL16)).all(), 'guard overwritten'
        got = out[:n_out].view(dtype).view(wp.shape)
        equal_bits(got, wp.cuda(), ('numpy', fmt, which, dtype))
        equal_bits(got, linear_warp(k, lin_gpu, lin_fmt, warps, PATCH, dtype=dtype), ('linear', fmt, which, dtype))
    assert (want[-2:] == -1.0).all() and not (want[:5] == -1.0).all()                  # the NaN and the off-frame matrix; the rest sees the frame
    via = k.eye_warp_surface_to_nchw(frames, warps, PATCH, L)
    equal_bits(via, want.cuda(), 'wrapper')
    equal_bits(k.eye_warp_surface_to_stem(frames, warps, PATCH, L, dtype=torch.float16), ref.pack_stem(want, torch.float16).cuda(), 'wrapper, packed')
    rows = frames.view(1, N, L.frame_bytes // L.pitch, L.pitch) if L.frame_bytes % L.pitch == 0 else frames.view(1, N, -1)
    equal_bits(data.warp_eye_patches(rows, warps[None], size=PATCH, layout=L)[0], want.cuda(), 'data.warp_eye_patches')


@pytest.mark.parametrize('which', ['vec', 'byte'])
@pytest.mark.parametrize('fmt', sref.FORMATS)
def test_the_screen_resize_equals_the_format_call_on_the_linearised_frame(fmt, which):
    k = default_kernels()
    L, buf, lin, lin_fmt, _, screens = case(fmt, which)
    N = len(MATRICES)
    frames, lin_gpu = torch.from_numpy(buf).cuda(), torch.from_numpy(lin).cuda()
    surf = L.as_ctypes()
    for hw, want in zip(TARGETS, screens):
        want = torch.from_numpy(want)
        n_out = want.numel()
        out = torch.full((n_out + GUARD,), SENTINEL, dtype=torch.float32, device='cuda')
        assert raw_screen(k, surf, 0, N, frames, hw, out) == 0, k.lib.eve_last_error()
        assert k.lib.eve_last_kernel() == screen_name(fmt, which == 'vec')
        assert (out[n_out:] == SENTINEL).all(), 'guard overwritten'
        got = out[:n_out].view(want.shape)
        equal_bits(got, want.cuda(), ('numpy', fmt, which, hw))
        equal_bits(got, linear_screen(k, lin_gpu, lin_fmt, hw), ('linear', fmt, which, hw))
        equal_bits(k.screen_area_surface_to_nchw(frames, hw, L), want.cuda(), 'wrapper')
    equal_bits(data.preprocess_screen_frames(frames.view(1, N, -1), size=TARGETS[0], layout=L)[0], torch.from_numpy(screens[0]).cuda(), 'data')


@pytest.mark.parametrize('fmt', ['nv21', 'yv12', 'uyvy', 'p010'])
def test_the_other_matrices(fmt):
    k = default_kernels()
    L, buf, lin, lin_fmt, patches, screens = case(fmt, 'vec')
    frames, lin_gpu, warps = torch.from_numpy(buf).cuda(), torch.from_numpy(lin).cuda(), torch.from_numpy(MATRICES).cuda()
    for matrix in ('bt709', 'jfif'):
        got = k.eye_warp_surface_to_nchw(frames, warps, PATCH, L, matrix=matrix)
        equal_bits(got, linear_warp(k, lin_gpu, lin_fmt, warps, PATCH, matrix=matrix), (fmt, matrix))
        assert not torch.equal(got.cpu(), torch.from_numpy(patches))
        scr = k.screen_area_surface_to_nchw(frames, TARGETS[0], L, matrix=matrix)
        equal_bits(scr, linear_screen(k, lin_gpu, lin_fmt, TARGETS[0], matrix=matrix), (fmt, matrix))
        equal_bits(scr, torch.from_numpy(rref.area_resize(rgb_of(lin, lin_fmt, matrix), TARGETS[0])).cuda(), (fmt, matrix, 'numpy'))
        assert not torch.equal(scr.cpu(), torch.from_numpy(screens[0]))


# ------------------------------------------------------------------------------------------------ padding, forms
@pytest.mark.parametrize('which', ['vec', 'byte'])
@pytest.mark.parametrize('fmt', sref.FORMATS)
def test_padding_is_never_read_into_a_result(fmt, which):
    """The same visible content embedded in random bytes and in their complement: every byte that is not a visible sample differs
    between the two buffers (row padding, coded rows, the pixels around the crop, an alpha channel, P010's low bytes), no output does."""
    k = default_kernels()
    L, buf, lin, _, patches, screens = case(fmt, which)
    fill = np.random.default_rng(5).integers(0, 256, size=buf.shape, dtype=np.uint8)
    a, b = sref.embed(lin, L, fill), sref.embed(lin, L, 255 - fill)
    assert int((a != b).sum()) == buf.size - lin.size and np.array_equal(sref.linear(b, L), lin)
    warps = torch.from_numpy(MATRICES).cuda()
    outs = []
    for v in (a, b):
        frames = torch.from_numpy(v).cuda()
        outs.append((k.eye_warp_surface_to_nchw(frames, warps, PATCH, L), k.eye_warp_surface_to_stem(frames, warps, PATCH, L),
                     k.screen_area_surface_to_nchw(frames, TARGETS[0], L), k.screen_area_surface_to_nchw(frames, TARGETS[1], L)))
    for x, y in zip(*outs):
        equal_bits(x, y, (fmt, which))
    equal_bits(outs[0][0], torch.from_numpy(patches).cuda(), 'numpy')
    equal_bits(outs[0][2], torch.from_numpy(screens[0]).cuda(), 'numpy')


def test_the_right_form_ran():
    """NV12 / I420: the vector form for pitches of a multiple of 8 with an 8-byte aligned base (uncropped: whole groups; cropped at
    x0 = 2: a skew, partial first and last groups), the byte form for a pitch of 100 and for a base pointer moved by one byte; the
    same content gives the same bits in both forms."""
    k = default_kernels()
    for fmt in ('nv12', 'i420'):
        tight, crop, odd = SurfaceLayout(fmt, 64, 48, pitch=96, coded_height=56), layout_of(fmt, 'vec'), SurfaceLayout(fmt, 64, 48, pitch=100, coded_height=56)
        lin = sref.random_surface(crop, 3, seed=8)[1]
        want = torch.from_numpy(rref.area_resize(pref.to_rgb(lin, fmt), TARGETS[0])).cuda()
        for L, name in ((tight, True), (crop, True), (odd, False)):
            frames = torch.from_numpy(sref.embed(lin, L, 0x5A)).cuda()
            assert frames.data_ptr() % 16 == 0
            equal_bits(k.screen_area_surface_to_nchw(frames, TARGETS[0], L), want, (fmt, L))
            assert k.lib.eve_last_kernel() == screen_name(fmt, name), (fmt, L)
        for L in (tight, crop):                                                # the base pointer moved by one byte
            v = sref.embed(lin, L, 0x5A)
            room = torch.zeros((v.size + 16,), dtype=torch.uint8, device='cuda')
            frames = room[1:1 + v.size].view(v.shape)
            frames.copy_(torch.from_numpy(v))
            assert frames.data_ptr() % 8 == 1 and frames.is_contiguous()
            equal_bits(k.screen_area_surface_to_nchw(frames, TARGETS[0], L), want, (fmt, L, 'offset'))
            assert k.lib.eve_last_kernel() == screen_name(fmt, False)
            patches = k.eye_warp_surface_to_nchw(frames, torch.from_numpy(MATRICES[:3]).cuda(), PATCH, L)       # (the taps are byte loads anyway)
            equal_bits(patches, torch.from_numpy(ref.eye_warp(pref.to_rgb(lin, fmt), MATRICES[:3], PATCH)[0]).cuda(), (fmt, 'warp, offset'))


# ------------------------------------------------------------------------------------------------ lens, eye_pose, the grid, 64 bits
def test_a_lens_through_the_surface_warp():
    k = default_kernels()
    L = SurfaceLayout('p010', 200, 160, pitch=512, coded_height=176, x0=8, y0=6)
    buf, lin = sref.random_surface(L, 2, seed=12)
    m = np.stack([ref.WARPS['rotated-perspective'][0], ref.WARPS['fractional-shift'][0]])
    rows = np.stack([lref.LENSES['barrel5'], lref.LENSES['rational8']])
    want = torch.from_numpy(lref.eye_warp(pref.to_rgb(lin, 'nv12'), m, rows, (128, 128))[0])
    frames, warps, lens = torch.from_numpy(buf).cuda(), torch.from_numpy(m).cuda(), torch.from_numpy(rows).cuda()
    got = k.eye_warp_surface_to_nchw(frames, warps, (128, 128), L, lens=lens)
    assert k.lib.eve_last_kernel() == warp_name(L, True, torch.float32)
    equal_bits(got, want.cuda(), 'numpy')
    equal_bits(got, k.eye_warp_fmt_to_nchw(torch.from_numpy(lin).cuda(), warps, (128, 128), 'nv12', lens=lens), 'linear')
    pk = k.eye_warp_surface_to_stem(frames, warps, (128, 128), L, lens=lens, dtype=torch.float16)
    assert k.lib.eve_last_kernel() == warp_name(L, True, torch.float16)
    equal_bits(pk, ref.pack_stem(want, torch.float16).cuda(), 'packed')
    assert not torch.equal(got, k.eye_warp_surface_to_nchw(frames, warps, (128, 128), L))


def camera_surface_of(B, T, seed):
    """-> (the layout, camera_surface uint8 [B, T, frame_bytes] and camera_frame_nv12 [B, T, 405, 480] of the same content, on the
    GPU): CAM-sized NV12 at crop (16, 8) inside rows of 512 bytes and 288 coded rows, padding random."""
    L = SurfaceLayout('nv12', CAM[1], CAM[0], pitch=512, coded_height=288, x0=16, y0=8)
    lin = pref.random_yuv_frames('nv12', B * T, CAM[0], CAM[1], seed)
    fill = np.random.default_rng(seed + 1).integers(0, 256, size=(B * T, L.frame_bytes), dtype=np.uint8)
    buf = sref.embed(lin, L, fill)
    return L, torch.from_numpy(buf).view(B, T, -1).cuda(), torch.from_numpy(lin).view((B, T) + lin.shape[1:]).cuda()


def screen_surface_of(B, T, seed):
    """-> (the layout, screen_surface uint8 [B, T, 144, 1088] and screen_frame_bgr [B, T, 144, 256, 3] of the same content, on the
    GPU): a 256 x 144 BGRA capture inside rows of 1088 bytes, padding and alpha random."""
    L = SurfaceLayout('bgra', 256, 144, pitch=1088)
    buf, lin = sref.random_surface(L, B * T, seed)
    return L, torch.from_numpy(buf).view(B, T, 144, 1088).cuda(), torch.from_numpy(lin).view((B, T) + lin.shape[1:]).cuda()


def tensors(v):
    return v if isinstance(v, tuple) else (v,)


def same(got, want, where=None):
    assert set(got) == set(want)
    for key in want:
        if torch.is_tensor(want[key]) or isinstance(want[key], tuple):
            for a, b in zip(tensors(got[key]), tensors(want[key])):
                assert torch.equal(a, b), (where, key)


def test_eye_pose_rows_through_the_surface_warp():
    """camera_surface + eye_pose through EyeNet.forward_sequence (bf16: the packed form) equals camera_frame_nv12 + eye_pose."""
    model, _ = make_model(dtype=torch.bfloat16)
    _, d, _ = gpu_clip(2, 3, seed=5)
    derived = ('left_eye_patch', 'right_eye_patch', 'left_h', 'right_h', 'left_o', 'right_o', 'left_R', 'right_R', 'head_R')
    rest = dict({k_: v for k_, v in d.items() if k_ not in derived}, eye_pose=cam_poses(2, 3, seed=7).cuda())
    L, surf, lin = camera_surface_of(2, 3, seed=21)
    model.eye_net.camera_layout = L
    with torch.no_grad():
        got = model.eye_net.forward_sequence(dict(rest, camera_surface=surf))
        want = model.eye_net.forward_sequence(dict(rest, camera_frame_nv12=lin))
    assert torch.isfinite(got['left_g_initial']).all()
    same(got, want)


@pytest.mark.parametrize('fmt', ['nv12', 'uyvy'])
def test_more_items_than_the_grid(fmt):
    """N = 520 patches of 4 x 4 from 12 x 8 surfaces, each with its own quarter-pixel shift: 1 040 bands in the float form and 2 600
    in the packed one against a grid of 1 024 workgroups; and 520 * 4 = 2 080 screen rows (a grid of 4 096 takes them at once)."""
    N, hw = 520, (4, 4)
    assert N * (hw[0] // BAND) > GRID_CAP and N * ((hw[0] + 6) // BAND) > GRID_CAP
    k = default_kernels()
    bpp = sref.BYTES_PER_PIXEL[fmt]
    L = SurfaceLayout(fmt, 12, 8, pitch=16 * bpp, coded_height=10, x0=2, y0=2)
    buf, lin = sref.random_surface(L, N, seed=70)
    g = np.random.default_rng(70)
    m = np.stack([ref.shift(float(g.integers(0, 32)) / 4, float(g.integers(0, 16)) / 4) for _ in range(N)])
    lin_fmt = sref.LINEAR_FORMAT[fmt]
    want = torch.from_numpy(ref.eye_warp(pref.to_rgb(lin, lin_fmt), m, hw)[0])
    frames, warps = torch.from_numpy(buf).cuda(), torch.from_numpy(m).cuda()
    equal_bits(k.eye_warp_surface_to_nchw(frames, warps, hw, L), want.cuda(), 'float')
    for dtype in (torch.bfloat16, torch.float16):
        equal_bits(k.eye_warp_surface_to_stem(frames, warps, hw, L, dtype=dtype), ref.pack_stem(want, dtype).cuda(), dtype)
    equal_bits(k.screen_area_surface_to_nchw(frames, (4, 6), L), torch.from_numpy(rref.area_resize(pref.to_rgb(lin, lin_fmt), (4, 6))).cuda(), 'screen')


def test_frame_strides_beyond_31_bits():
    """N = 2 with frame_stride = 2^31 + 4096 in an uninitialised allocation, only the two small frames written: frame 1's result is
    that of the frame alone, for the warp and for all three screen forms."""
    k = default_kernels()
    stride = 2 ** 31 + 4096
    for fmt in ('nv12', 'yuyv'):
        for which in ('vec', 'byte'):
            L, buf, _, _, patches, screens = case(fmt, which)
            room = torch.empty((stride + L.frame_bytes,), dtype=torch.uint8, device='cuda')
            room[:L.frame_bytes].copy_(torch.from_numpy(buf[0]))
            room[stride:].copy_(torch.from_numpy(buf[1]))
            surf = L.as_ctypes()
            surf.frame_stride = stride
            warps = torch.from_numpy(MATRICES[:2]).cuda()
            out = torch.full((2 * 3 * PATCH[0] * PATCH[1],), SENTINEL, device='cuda')
            assert raw_warp(k, surf, 0, 2, room, warps, None, PATCH, out) == 0, k.lib.eve_last_error()
            equal_bits(out.view((2, 3) + PATCH), torch.from_numpy(patches[:2]).cuda(), (fmt, which, 'warp'))
            alone = k.eye_warp_surface_to_nchw(room[stride:].view(1, -1), warps[1:], PATCH, L)
            equal_bits(out.view((2, 3) + PATCH)[1:], alone, (fmt, which, 'frame 1 alone'))
            scr = torch.full((2 * 3 * 9 * 16,), SENTINEL, device='cuda')
            assert raw_screen(k, surf, 0, 2, room, TARGETS[0], scr) == 0, k.lib.eve_last_error()
            assert k.lib.eve_last_kernel() == screen_name(fmt, which == 'vec')
            equal_bits(scr.view(2, 3, 9, 16), torch.from_numpy(screens[0][:2]).cuda(), (fmt, which, 'screen'))
            equal_bits(scr.view(2, 3, 9, 16)[1:], k.screen_area_surface_to_nchw(room[stride:].view(1, -1), TARGETS[0], L), (fmt, which, 'frame 1 alone'))
            del room


# ------------------------------------------------------------------------------------------------ refusals
def test_refused_requests_launch_nothing():
    k = default_kernels()
    L = layout_of('nv12', 'vec')
    frames = torch.zeros((2, L.frame_bytes), dtype=torch.uint8, device='cuda')
    warps = torch.from_numpy(np.stack([ref.shift(0, 0)] * 2)).cuda()
    k.stream_state_rows(torch.zeros((2, 8), device='cuda'), torch.zeros((2, 8), device='cuda'))     # the last named launch
    before = k.lib.eve_last_kernel()
    assert b'surface' not in before
    hw = (8, 12)
    out = torch.full((2 * 3 * 48 * 64 + GUARD,), SENTINEL, dtype=torch.float32, device='cuda')
    out16 = torch.full((2 * (hw[0] + 6) * (hw[1] + 8) * 4 + GUARD,), SENTINEL16, dtype=torch.int16, device='cuda')

    def made(**changes):
        s = L.as_ctypes()
        for name, v in changes.items():
            if isinstance(v, tuple):
                getattr(s, name)[v[0]] = v[1]
            else:
                setattr(s, name, v)
        return s

    rgb_shift = SurfaceLayout('bgra', 32, 16, pitch=128).as_ctypes()
    rgb_shift.xshift = 1
    last = lambda c: L.offset[c] + ((47 >> (1 if c else 0)) * L.pitches[c]) + ((63 >> (1 if c else 0)) * L.step[c])
    # (what is wrong with the descriptor, the matrix, N) -> a word of the message
    cases = {'struct_bytes': (made(struct_bytes=84), 0, 2, 'struct_bytes'), 'struct_bytes zero': (made(struct_bytes=0), 0, 2, 'struct_bytes'),
             'kind': (made(kind=2), 0, 2, 'unknown kind'), 'negative kind': (made(kind=-1), 0, 2, 'unknown kind'),
             'matrix': (made(), 3, 2, 'unknown matrix'), 'negative matrix': (made(), -1, 2, 'unknown matrix'),
             'xshift 2': (made(xshift=2), 0, 2, 'xshift'), 'yshift -1': (made(yshift=-1), 0, 2, 'yshift'), 'rgb with a shift': (rgb_shift, 0, 1, 'EVE_SURF_RGB'),
             'pitch 0': (made(pitch=(1, 0)), 0, 2, 'pitch'), 'negative pitch': (made(pitch=(0, -96)), 0, 2, 'pitch'), 'step 0': (made(step=(2, 0)), 0, 2, 'step'),
             'negative offset': (made(offset=(0, -1)), 0, 2, 'offset'),
             'luma beyond the frame': (made(frame_bytes=last(0)), 0, 1, 'frame_bytes'), 'U beyond the frame': (made(frame_bytes=last(1)), 0, 1, 'frame_bytes'),
             'V beyond the frame': (made(frame_bytes=last(2)), 0, 1, 'frame_bytes'), 'a pitch that leaves the frame': (made(pitch=(2, 200)), 0, 2, 'frame_bytes'),
             'a width that leaves the frame': (made(width=4096), 0, 2, 'frame_bytes'), 'a height that leaves the frame': (made(height=120), 0, 2, 'frame_bytes'),
             'frame_bytes beyond the stride': (made(frame_stride=L.frame_bytes - 1), 0, 2, 'frame_stride'),
             'no width': (made(width=0), 0, 2, 'bad arguments'), 'no frames': (made(), 0, 0, 'bad arguments')}
    assert last(2) == max(last(c) for c in range(3)) and last(2) < L.frame_bytes
    entries = (('eye_warp_surface_to_nchw:', lambda s, mat, N, h=hw, a=frames, b=warps, c=out: raw_warp(k, s, mat, N, a, b, None, h, c)),
               ('eye_warp_surface_to_stem:', lambda s, mat, N, h=hw, a=frames, b=warps, c=out16: raw_warp(k, s, mat, N, a, b, None, h, c, torch.bfloat16)),
               ('screen_area_surface_to_nchw:', lambda s, mat, N, h=hw, a=frames, b=None, c=out: raw_screen(k, s, mat, N, a, h, c)))
    for prefix, fn in entries:
        for name, (s, mat, N, word) in cases.items():
            assert fn(s, mat, N) != 0, (prefix, name)
            msg = k.lib.eve_last_error().decode()
            assert msg.startswith(prefix) and word in msg, (prefix, name, msg)
            assert k.lib.eve_last_kernel() == before, (prefix, name)
        assert fn(made(frame_bytes=last(2) + 1), 0, 1) == 0, k.lib.eve_last_error()     # one byte more: the tightest frame there is
        assert b'surface' in k.lib.eve_last_kernel()
        k.stream_state_rows(torch.zeros((2, 8), device='cuda'), torch.zeros((2, 8), device='cuda'))
        assert k.lib.eve_last_kernel() == before
        torch.cuda.synchronize()
        out.fill_(SENTINEL)
        out16.fill_(SENTINEL16)
        for nulls in (dict(a=None), dict(c=None)) + ((dict(b=None),) if 'eye_warp' in prefix else ()):
            assert fn(made(), 0, 2, **nulls) != 0
            assert k.lib.eve_last_error().decode().startswith(prefix) and k.lib.eve_last_kernel() == before
    # a null descriptor
    assert k.lib.eve_eye_warp_surface_to_nchw(None, 0, 2, ptr(frames), ptr(warps), None, hw[0], hw[1], ptr(out), stream_ptr()) != 0
    assert k.lib.eve_last_error().decode().startswith('eye_warp_surface_to_nchw:')
    assert k.lib.eve_screen_area_surface_to_nchw(None, 0, 2, ptr(frames), hw[0], hw[1], ptr(out), stream_ptr()) != 0
    assert k.lib.eve_last_error().decode().startswith('screen_area_surface_to_nchw:')
    # what the existing pairs refuse: sizes, upscaling, N limits, the packed form's dtype
    big = made(width=16386, pitch=(0, 16386), frame_bytes=2 ** 40, frame_stride=2 ** 40, offset=(1, 2 ** 30))
    big.pitch[1] = big.pitch[2] = 16386
    big.offset[2] = 2 ** 30 + 1
    for prefix, fn in entries[:2]:
        for s, N, h, word in ((big, 1, hw, 'frame too large'), (made(), 2, (4097, 12), 'patch too large'), (made(), 2, (8, 4097), 'patch too large'),
                              (made(frame_stride=L.frame_bytes), 2 ** 31 // (hw[0] + 6) + 1, hw, '31 bits')):
            assert fn(s, 0, N, h=h) != 0
            msg = k.lib.eve_last_error().decode()
            assert msg.startswith(prefix) and word in msg, (prefix, msg)
    assert k.lib.eve_eye_warp_surface_to_stem(dt_code(torch.float32), ctypes.byref(made()), 0, 2, ptr(frames), ptr(warps), None, hw[0], hw[1], ptr(out16),
                                              stream_ptr()) != 0
    msg = k.lib.eve_last_error().decode()
    assert msg.startswith('eye_warp_surface_to_stem:') and 'dtype' in msg
    prefix, fn = entries[2]
    wide = SurfaceLayout('nv12', 16384, 2).as_ctypes()
    huge = made(width=8192, height=4096, frame_bytes=2 ** 40, frame_stride=2 ** 40, offset=(1, 2 ** 30))
    huge.pitch[0] = huge.pitch[1] = huge.pitch[2] = 8192
    huge.offset[2] = 2 ** 30 + 1
    for s, N, h, word in ((made(), 2, (49, 12), 'upscaling'), (made(), 2, (8, 65), 'upscaling'), (made(), 2, (0, 12), 'bad arguments'),
                          (wide, 1, (1, 8), 'row too wide'), (huge, 1, hw, 'frame too large'), (made(), 2 ** 31 // hw[0] + 1, hw, '31 bits')):
        assert fn(s, 0, N, h=h) != 0
        msg = k.lib.eve_last_error().decode()
        assert msg.startswith(prefix) and word in msg, msg
    assert k.lib.eve_last_kernel() == before
    torch.cuda.synchronize()
    assert (out.cpu() == SENTINEL).all() and (out16.cpu() == SENTINEL16).all()
    # the tensor-level wrappers: the tensor must hold (N - 1) * frame_stride + frame_bytes bytes, a stride per frame
    with pytest.raises(ValueError, match='stride'):
        k.eye_warp_surface_to_nchw(frames[:, :-1].contiguous(), warps, hw, L)
    with pytest.raises(ValueError, match='stride'):
        k.screen_area_surface_to_nchw(torch.zeros((2, L.frame_bytes + 8), dtype=torch.uint8, device='cuda'), hw, L)
    with pytest.raises(TypeError):
        k.screen_area_surface_to_nchw(frames, hw, L.descriptor())
    with pytest.raises(RuntimeError):
        k.eye_warp_surface_to_nchw(frames, warps.cpu(), hw, L)
    assert k.lib.eve_last_kernel() == before


# ------------------------------------------------------------------------------------------------ EVEStream under graph replay
def surface_chunks(d, T, seed):
    """d: a dict of [B, T, ...] GPU tensors -> (the layouts, d with camera_surface + screen_surface, d with camera_frame_nv12 +
    screen_frame_bgr of the same content), patch keys and screen_frame removed, with camera_clip's warps."""
    _, lw, rw, _, _ = camera_clip(seed)
    B = lw.shape[0]
    cl, cam, cam_lin = camera_surface_of(B, T, seed)
    sl, scr, scr_lin = screen_surface_of(B, T, seed + 2)
    rest = {k_: v for k_, v in d.items() if k_ not in ('left_eye_patch', 'right_eye_patch', 'screen_frame')}
    rest = dict(rest, left_eye_warp=lw[:, :T].contiguous().cuda(), right_eye_warp=rw[:, :T].contiguous().cuda())
    return (cl, sl), dict(rest, camera_surface=cam, screen_surface=scr), dict(rest, camera_frame_nv12=cam_lin, screen_frame_bgr=scr_lin)


def test_stream_replays_a_graph_over_both_surfaces():
    """B = 2, Tc = 2: the capture and two replays with different contents each equal the camera_frame_nv12 + screen_frame_bgr graph
    stream on the linearised chunk bit for bit, and differ from each other; the input buffers hold the surfaces whole; another
    layout is another graph."""
    model, _ = make_model()
    _, d, _ = gpu_clip(2, 6, seed=5)
    (cl, sl), surf, lin = surface_chunks(d, 6, 33)
    model.eye_net.camera_layout, model.refine_net.screen_layout = cl, sl
    ch = lambda src, i: {k_: v[:, 2 * i:2 * i + 2].contiguous() for k_, v in src.items()}
    g, c, e = eve_amd.EVEStream(model, 2), eve_amd.EVEStream(model, 2), eve_amd.EVEStream(model, 2, use_graph=False)
    outs = []
    for i in range(3):
        og = {k_: v.clone() for k_, v in g.step(ch(surf, i), return_heatmaps=True).items()}
        same(og, c.step(ch(lin, i), return_heatmaps=True), i)
        same(og, e.step(ch(surf, i), return_heatmaps=True), i)
        outs.append(og)
    assert len(g._graphs) == 1 and len(c._graphs) == 1 and 'heatmap_final' in outs[0]
    assert not torch.equal(outs[1]['g_initial'], outs[2]['g_initial']) and not torch.equal(outs[1]['heatmap_final'], outs[2]['heatmap_final'])
    inputs = g._graphs[next(iter(g._graphs))]['inputs']
    assert tuple(inputs['camera_surface'].shape) == (2, 2, cl.frame_bytes) and tuple(inputs['screen_surface'].shape) == (2, 2, 144, 1088)
    with pytest.raises(ValueError, match='screen_surface'):
        g.step(ch(surf, 0), render=eve_amd.OverlaySpec())
    with pytest.raises(ValueError, match='one camera frame key'):
        g.step(dict(ch(surf, 0), camera_frame_nv12=ch(lin, 0)['camera_frame_nv12']))
    model.eye_net.camera_layout = SurfaceLayout('nv21', cl.width, cl.height, pitch=cl.pitch, coded_height=cl.coded_height, x0=cl.x0, y0=cl.y0)
    g.reset()
    swapped = g.step(ch(surf, 0), return_heatmaps=True)
    assert len(g._graphs) == 2 and not torch.equal(swapped['g_initial'], outs[0]['g_initial'])
    model.eye_net.camera_layout = None
    with pytest.raises(ValueError, match='camera_layout'):
        g.step(ch(surf, 0))


def test_stream_surfaces_with_lengths_and_an_eye_mask():
    model, _ = make_model()
    _, d, _ = gpu_clip(2, 4, seed=5)
    (cl, sl), surf, lin = surface_chunks(d, 4, 35)
    model.eye_net.camera_layout, model.refine_net.screen_layout = cl, sl
    mask = torch.tensor([[[1, 1], [0, 1], [1, 0], [1, 1]], [[1, 1], [1, 1], [0, 0], [1, 1]]], dtype=torch.bool)
    lengths = ([2, 1], [2, 2])
    ch = lambda src, i: {k_: v[:, 2 * i:2 * i + 2].contiguous() for k_, v in src.items()}
    g, c = eve_amd.EVEStream(model, 2), eve_amd.EVEStream(model, 2)
    for i in range(2):
        m_ = mask[:, 2 * i:2 * i + 2]
        got = {k_: v.clone() for k_, v in g.step(ch(surf, i), eye_mask=m_, lengths=lengths[i], return_heatmaps=True).items()}
        want = c.step(ch(lin, i), eye_mask=m_, lengths=lengths[i], return_heatmaps=True)
        assert set(got) == set(want) and 'eye_valid' in got and torch.equal(got['eye_valid'], want['eye_valid']) and torch.equal(got['valid'], want['valid'])
        valid, eye_valid = got['valid'], got['eye_valid']
        assert valid.any() and not valid.all()
        for key in want:
            a, b = got[key], want[key]
            if key.startswith(('left_', 'right_')) and key not in ('left_R',):
                sel = eye_valid[..., 0 if key.startswith('left_') else 1]
            else:
                sel = valid
            if a.shape[:2] == sel.shape and a.dtype.is_floating_point:
                assert torch.equal(a[sel], b[sel]), (i, key)
    assert len(g._graphs) == 1
    sa, sb = g.get_state(), c.get_state()
    for key in sb:
        for x, y in zip(tensors(sa[key]), tensors(sb[key])):
            assert torch.equal(x, y), key
