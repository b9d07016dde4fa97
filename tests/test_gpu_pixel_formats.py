"""GPU: eve_eye_warp_fmt_to_nchw / eve_eye_warp_fmt_to_stem (csrc/eye_warp.hip) bit for bit against their contract -- the existing
numpy contracts on the frame converted by tests/pixel_format_ref.to_rgb -- for BGR(A), NV12, I420 and YUYV frames, plain and with
a lens; the keys camera_frame_bgr / _nv12 / _i420 / _yuyv through EyeNet.forward_sequence, EVE.forward and EVEStream, eager and
under graph replay, against camera_frame on the converted frame; and eve_screen_u8_area_bgr_to_nchw / screen_frame_bgr against
the channel-reversed capture."""
import ctypes

import numpy as np
import pytest
import torch

import eve_amd
from eve_amd import data
from eve_amd.kernels import PIXEL_FORMATS, YUV_MATRICES, default_kernels, dt_code
import eye_warp_lens_ref as lref
import eye_warp_ref as ref
import pixel_format_ref as pref
from test_gpu_eye_pose import cam_lens, cam_poses
from test_gpu_eye_warp import BAND, CAM, FRAME, GRID_CAP, GUARD, HW, SENTINEL, SENTINEL16, camera_clip, differing, stream_ptr
from test_gpu_stream import gpu_clip, make_model

pytestmark = pytest.mark.gpu
TYPE_NAMES = {torch.float32: 'float', torch.bfloat16: 'eve::bf16_t', torch.float16: 'eve::f16_t'}


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def kernel_name(code_name, lens, dtype):
    return ('eye_warp_fmt_kernel<%s,%s,%s>' % (code_name, 'lens' if lens else 'plain', TYPE_NAMES[dtype])).encode()


def code_of(fmt, buf_shape):
    """The EVE_PIX_* name and code of a buffer: 'bgr' with four channels is EVE_PIX_BGRA."""
    name = 'bgra' if fmt == 'bgr' and buf_shape[-1] == 4 else fmt
    return name, PIXEL_FORMATS[name]


def raw_nchw(k, code, matrix, N, IH, IW, frames, warps, lens, hw, out):
    return k.lib.eve_eye_warp_fmt_to_nchw(code, matrix, N, IH, IW, ptr(frames), ptr(warps), ptr(lens), hw[0], hw[1], ptr(out), stream_ptr())


def raw_stem(k, dtype, code, matrix, N, IH, IW, frames, warps, lens, hw, out):
    return k.lib.eve_eye_warp_fmt_to_stem(dt_code(dtype), code, matrix, N, IH, IW, ptr(frames), ptr(warps), ptr(lens), hw[0], hw[1], ptr(out),
                                          stream_ptr())


def check(k, buf, fmt, m, hw, kind, matrix='bt601', L=None, packed=True, frames=None):
    """Both exports of one format, two launches each into a guarded buffer, == the RGB contract (the lens contract with L) on
    to_rgb(buf) with no tolerance on the integer view; the guard untouched; the kernel's documented name; the reference's outside
    share what the case claims; the pad ring and the fourth channel zero in the packed forms.  -> (frames, warps, lens on the GPU,
    want)."""
    N = buf.shape[0]
    IH, IW = pref.frame_hw(buf.shape, fmt)
    rgb = pref.to_rgb(buf, fmt, matrix)
    want, outside = ref.eye_warp(rgb, m, hw) if L is None else lref.eye_warp(rgb, m, L, hw)
    assert ref.outside_share_ok(kind, float(outside.mean())), (kind, float(outside.mean()))
    want = torch.from_numpy(want)
    n_out = want.numel()
    frames = torch.from_numpy(buf).cuda() if frames is None else frames
    warps = torch.from_numpy(m).cuda()
    lens = None if L is None else torch.from_numpy(L).cuda()
    name, code = code_of(fmt, buf.shape)
    mat = YUV_MATRICES[matrix]
    for _ in range(2):
        out = torch.full((n_out + GUARD,), SENTINEL, dtype=torch.float32, device='cuda')
        assert raw_nchw(k, code, mat, N, IH, IW, frames, warps, lens, hw, out) == 0, k.lib.eve_last_error()
        assert k.lib.eve_last_kernel() == kernel_name(name, L is not None, torch.float32)
        got = out.cpu()
        assert torch.equal(got[n_out:], torch.full((GUARD,), SENTINEL)), 'guard overwritten'
        gi, wi = got[:n_out].view(torch.int32), want.reshape(-1).view(torch.int32)
        assert torch.equal(gi, wi), differing(gi, wi)
    if not packed:
        return frames, warps, lens, want
    for dtype in (torch.bfloat16, torch.float16):
        wp = ref.pack_stem(want, dtype)
        n_pk = wp.numel()
        for _ in range(2):
            out = torch.full((n_pk + GUARD,), SENTINEL16, dtype=torch.int16, device='cuda')
            assert raw_stem(k, dtype, code, mat, N, IH, IW, frames, warps, lens, hw, out) == 0, k.lib.eve_last_error()
            assert k.lib.eve_last_kernel() == kernel_name(name, L is not None, dtype)
            got = out.cpu()
            assert (got[n_pk:] == SENTINEL16).all(), 'guard overwritten'
            gi, wi = got[:n_pk], wp.reshape(-1).view(torch.int16)
            assert torch.equal(gi, wi), differing(gi, wi)
            img = got[:n_pk].view(N, hw[0] + 6, hw[1] + 8, 4)
            ring = img.clone()
            ring[:, 3:hw[0] + 3, 4:hw[1] + 4] = 0
            assert not ring.any() and not img[..., 3].any()                  # the pad ring and the fourth channel
    return frames, warps, lens, want


# ------------------------------------------------------------------------------------------------ the kernel against its contract
@pytest.mark.parametrize('name', list(ref.WARPS))
@pytest.mark.parametrize('fmt', pref.FORMATS)
def test_every_format_equals_the_contract(fmt, name):
    """The five shared warps, plain and behind barrel5, on random bytes and on the chroma checkerboard; the outside shares are the
    RGB cases' (the coordinates do not depend on the format)."""
    m = np.stack([ref.WARPS[name][0]] * 2)
    L = np.stack([lref.LENSES['barrel5']] * 2)
    k = default_kernels()
    rnd = pref.random_yuv_frames(fmt, 2, FRAME[0], FRAME[1], seed=len(name) + len(fmt))
    board = pref.chroma_checkerboard(fmt, 2, FRAME[0], FRAME[1])
    for lens, kind in ((None, ref.WARPS[name][1]), (L, lref.outside_kind('barrel5', name))):
        frames, warps, lens_gpu, want = check(k, rnd, fmt, m, HW, kind, L=lens)
        check(k, board, fmt, m, HW, kind, L=lens)
        via = k.eye_warp_fmt_to_nchw(frames, warps, HW, fmt, lens=lens_gpu)                   # the tensor-level wrappers
        assert via.dtype == torch.float32 and tuple(via.shape) == (2, 3) + HW and torch.equal(via.cpu(), want)
        pk = k.eye_warp_fmt_to_stem(frames, warps, HW, fmt, lens=lens_gpu, dtype=torch.float16)
        assert pk.dtype == torch.float16 and torch.equal(pk.cpu().view(torch.int16), ref.pack_stem(want, torch.float16).view(torch.int16))
    lead = lambda t: t.view((1,) + tuple(t.shape))
    assert torch.equal(data.warp_eye_patches(lead(frames), lead(warps), size=HW, lens=lead(lens_gpu), format=fmt).cpu()[0], want)
    # ... and the RGB launch on the converted frame, on the device
    rgb = torch.from_numpy(pref.to_rgb(rnd, fmt)).cuda()
    assert torch.equal(k.eye_warp_lens_u8_to_nchw(rgb, warps, lens_gpu, HW).cpu(), want)
    if fmt != 'bgr':                                                   # the checkerboard's chroma is seen: not a grey patch
        grey = check(k, board, fmt, m, HW, ref.WARPS[name][1])[3]
        inside = grey[:, 0] != -1.0
        assert (grey[:, 0][inside] != grey[:, 2][inside]).any()


@pytest.mark.parametrize('fmt', ['nv12', 'i420', 'yuyv'])
def test_all_three_matrices(fmt):
    k = default_kernels()
    m, kind = ref.WARPS['rotated-perspective']
    buf = pref.random_yuv_frames(fmt, 2, FRAME[0], FRAME[1], seed=9)
    wants = [check(k, buf, fmt, np.stack([m, m]), HW, kind, matrix=matrix)[3] for matrix in ('bt601', 'bt709', 'jfif')]
    assert not torch.equal(wants[0], wants[1]) and not torch.equal(wants[0], wants[2]) and not torch.equal(wants[1], wants[2])


def test_bgra_ignores_alpha_and_the_matrix():
    k = default_kernels()
    buf = pref.random_yuv_frames('bgr', 2, FRAME[0], FRAME[1], seed=4, C=4)
    assert (buf[..., 3] == 255).all()
    m = np.stack([ref.WARPS['rotated-perspective'][0], ref.WARPS['fractional-shift'][0]])
    frames, warps, _, want = check(k, buf, 'bgr', m, HW, 'few')
    check(k, buf, 'bgr', m, HW, 'few', matrix='jfif')
    out = torch.empty((2, 3) + HW, device='cuda')
    assert raw_nchw(k, PIXEL_FORMATS['bgra'], 77, 2, FRAME[0], FRAME[1], frames, warps, None, HW, out) == 0      # ignored for BGR(A)
    assert torch.equal(out.cpu(), want)
    bgr3 = torch.from_numpy(np.ascontiguousarray(buf[..., :3])).cuda()
    assert torch.equal(k.eye_warp_fmt_to_nchw(bgr3, warps, HW, 'bgr').cpu(), want)


@pytest.mark.parametrize('fmt', pref.FORMATS)
@pytest.mark.parametrize('name', ['nan', 'off-frame'])
def test_a_nan_matrix_and_an_off_frame_one_give_minus_one(name, fmt):
    m = {'nan': ref.NAN_WARP, 'off-frame': ref.OFF_FRAME_WARP}[name]
    k = default_kernels()
    buf = pref.random_yuv_frames(fmt, 1, FRAME[0], FRAME[1], seed=2)
    frames, warps, _, want = check(k, buf, fmt, m[None], HW, 'all')
    assert (want == -1.0).all()
    pk = k.eye_warp_fmt_to_stem(frames, warps, HW, fmt).cpu().float()
    assert (pk[:, 3:-3, 4:-4, :3] == -1.0).all() and (pk[:, 3:-3, 4:-4, 3] == 0.0).all()


@pytest.mark.parametrize('fmt', ['nv12', 'i420', 'yuyv'])
def test_limited_range_black_is_minus_one_inside_the_frame(fmt):
    """Y = 16, U = V = 128 is RGB (0, 0, 0) in limited range: -1.0 at every pixel inside the frame, as outside it."""
    k = default_kernels()
    buf = pref.constant_frames(fmt, 2, FRAME[0], FRAME[1], 16, 128, 128)
    m = np.stack([ref.WARPS['fractional-shift'][0], ref.WARPS['integer-shift'][0]])
    for matrix in ('bt601', 'bt709'):
        want = check(k, buf, fmt, m, HW, 'none', matrix=matrix)[3]
        assert (want == -1.0).all()
    want = check(k, buf, fmt, m, HW, 'none', matrix='jfif')[3]        # full range: 16 stays 16
    assert (want == np.float32(16.0) * np.float32(2.0 / 255.0) + np.float32(-1.0)).all()


@pytest.mark.parametrize('fmt', ['nv12', 'yuyv'])
def test_more_items_than_the_grid(fmt):
    """N = 520 patches of 4 x 4 from 8 x 12 frames, each with its own quarter-pixel shift: 520 * 2 = 1 040 bands in the float form
    and 520 * 5 = 2 600 in the packed one, against a grid of 1 024 workgroups."""
    N, hw = 520, (4, 4)
    assert N * (hw[0] // BAND) > GRID_CAP and N * ((hw[0] + 6) // BAND) > GRID_CAP
    k = default_kernels()
    g = np.random.default_rng(70)
    m = np.stack([ref.shift(float(g.integers(0, 32)) / 4, float(g.integers(0, 16)) / 4) for _ in range(N)])
    check(k, pref.random_yuv_frames(fmt, N, 8, 12, seed=70), fmt, m, hw, 'none')
    check(k, pref.chroma_checkerboard(fmt, N, 8, 12), fmt, m, hw, 'none')


@pytest.mark.parametrize('fmt', ['nv12', 'i420', 'yuyv', 'bgr'])
def test_a_frame_pointer_offset_by_one_byte(fmt):
    k = default_kernels()
    v = pref.random_yuv_frames(fmt, 2, FRAME[0], FRAME[1], seed=3)
    buf = torch.zeros((v.size + 16,), dtype=torch.uint8, device='cuda')
    frames = buf[1:1 + v.size].view(v.shape)
    frames.copy_(torch.from_numpy(v))
    assert frames.data_ptr() % 16 == 1 and frames.is_contiguous()
    m, kind = ref.WARPS['rotated-perspective']
    check(k, v, fmt, np.stack([m, m]), HW, kind, frames=frames)


def test_full_hd_nv12():
    """N = 2 frames of 1080 x 1920 NV12, the plain full-HD test's warps (scale 1.4, +-10 degrees, a perspective row): all inside."""
    k = default_kernels()
    v = pref.random_yuv_frames('nv12', 2, 1080, 1920, seed=5)
    m = np.stack([ref.similarity(1.4, 10.0, 800.0, 400.0, persp=(1e-4, -2e-4)), ref.similarity(1.4, -10.0, 1000.0, 500.0, persp=(-1e-4, 2e-4))])
    check(k, v, 'nv12', m, HW, 'none')


def test_refused_requests_launch_nothing():
    k = default_kernels()
    frames = torch.zeros((1, 90 * 160 * 4), dtype=torch.uint8, device='cuda')            # room for every format at 90 x 160
    warps = torch.from_numpy(ref.shift(0, 0)[None]).cuda()
    lens = torch.from_numpy(lref.lens_row(150, 150, 80, 45, k1=-0.2)[None]).cuda()
    hw = (36, 60)
    k.stream_state_rows(torch.zeros((2, 8), device='cuda'), torch.zeros((2, 8), device='cuda'))     # the last named launch
    before = k.lib.eve_last_kernel()
    assert b'eye_warp' not in before
    n_out, n_pk = 3 * hw[0] * hw[1], (hw[0] + 6) * (hw[1] + 8) * 4
    out = torch.full((n_out + GUARD,), SENTINEL, dtype=torch.float32, device='cuda')
    out16 = torch.full((n_pk + GUARD,), SENTINEL16, dtype=torch.int16, device='cuda')
    F, M = PIXEL_FORMATS, YUV_MATRICES
    bf16 = torch.bfloat16
    nchw = lambda fmt, mat, N, IH, IW, OH, OW, a=frames, b=warps, c=out, d=None: raw_nchw(k, fmt, mat, N, IH, IW, a, b, d, (OH, OW), c)
    stem = lambda fmt, mat, N, IH, IW, OH, OW, a=frames, b=warps, c=out16, d=None, dt=bf16: raw_stem(k, dt, fmt, mat, N, IH, IW, a, b, d, (OH, OW), c)
    cases = {'unknown format': ((5, 0, 1, 90, 160) + hw, 'unknown format'), 'negative format': ((-1, 0, 1, 90, 160) + hw, 'unknown format'),
             'unknown matrix': ((F['nv12'], 3, 1, 90, 160) + hw, 'unknown matrix'), 'negative matrix': ((F['yuyv'], -1, 1, 90, 160) + hw, 'unknown matrix'),
             'nv12 odd rows': ((F['nv12'], 0, 1, 91, 160) + hw, 'even'), 'nv12 odd columns': ((F['nv12'], 0, 1, 90, 161) + hw, 'even'),
             'i420 odd rows': ((F['i420'], 0, 1, 91, 160) + hw, 'even'), 'i420 odd columns': ((F['i420'], 0, 1, 90, 161) + hw, 'even'),
             'yuyv odd columns': ((F['yuyv'], 0, 1, 90, 161) + hw, 'even'), 'no frames': ((F['nv12'], 0, 0, 90, 160) + hw, 'bad arguments'),
             'frame too wide': ((F['bgr'], 0, 1, 90, 16386) + hw, 'frame too large'), 'frame too high': ((F['i420'], 0, 1, 16386, 160) + hw, 'frame too large'),
             'patch too high': ((F['yuyv'], 0, 1, 90, 160, 4097, 60), 'patch too large'), 'patch too wide': ((F['bgra'], 0, 1, 90, 160, 36, 4097), 'patch too large')}
    for fn, prefix in ((nchw, 'eye_warp_fmt_to_nchw:'), (stem, 'eye_warp_fmt_to_stem:')):
        for name, (args, word) in cases.items():
            assert fn(*args) != 0, name
            msg = k.lib.eve_last_error().decode()
            assert msg.startswith(prefix) and word in msg, (name, msg)
            assert k.lib.eve_last_kernel() == before, name
        for nulls in (dict(a=None), dict(b=None), dict(c=None)):
            assert fn(F['nv12'], 0, 1, 90, 160, *hw, **nulls) != 0
            assert k.lib.eve_last_error().decode().startswith(prefix) and k.lib.eve_last_kernel() == before
    assert stem(F['nv12'], 0, 1, 90, 160, *hw, dt=torch.float32) != 0                   # the packed form is 16-bit only
    msg = k.lib.eve_last_error().decode()
    assert msg.startswith('eye_warp_fmt_to_stem:') and 'dtype' in msg and k.lib.eve_last_kernel() == before
    torch.cuda.synchronize()
    assert (out.cpu() == SENTINEL).all() and (out16.cpu() == SENTINEL16).all()
    nv12 = frames[:, :135 * 160].view(1, 135, 160)
    with pytest.raises(ValueError):
        k.eye_warp_fmt_to_nchw(nv12, warps, hw, 'nv21')
    with pytest.raises(ValueError):
        k.eye_warp_fmt_to_nchw(nv12, warps, hw, 'nv12', matrix='nonsense')
    with pytest.raises(ValueError):
        k.eye_warp_fmt_to_nchw(frames[:, :135 * 161].view(1, 135, 161), warps, hw, 'i420')
    with pytest.raises(ValueError):
        k.eye_warp_fmt_to_stem(frames[:, :136 * 160].view(1, 136, 160), warps, hw, 'nv12')
    with pytest.raises(ValueError):
        k.eye_warp_fmt_to_nchw(frames[:, :90 * 161 * 2].view(1, 90, 161, 2), warps, hw, 'yuyv')
    with pytest.raises(TypeError):
        k.eye_warp_fmt_to_nchw(nv12, warps, hw, 'yuyv')
    with pytest.raises(TypeError):
        k.eye_warp_fmt_to_nchw(nv12.float(), warps, hw, 'nv12')
    with pytest.raises(TypeError):
        k.eye_warp_fmt_to_nchw(nv12, warps.double(), hw, 'nv12')
    with pytest.raises(TypeError, match='lens'):
        k.eye_warp_fmt_to_nchw(nv12, warps, hw, 'nv12', lens=lens[:, :5].contiguous())
    with pytest.raises(TypeError):
        k.eye_warp_fmt_to_stem(nv12, warps, hw, 'nv12', out=torch.empty((1, hw[0] + 6, hw[1] + 8, 4), device='cuda'))
    with pytest.raises(RuntimeError):
        k.eye_warp_fmt_to_nchw(nv12, warps, hw, 'nv12', lens=lens.cpu())
    assert k.lib.eve_last_kernel() == before
    for code in (F['nv12'], F['i420'], F['yuyv']):                                      # sound arguments are taken: a zero frame, bt601
        assert nchw(code, 0, 1, 90, 160, *hw, d=lens) == 0 and stem(code, 0, 1, 90, 160, *hw) == 0
        want = pref.yuv_to_rgb(np.uint8(0), np.uint8(0), np.uint8(0), 'bt601').astype(np.float32) * np.float32(2.0 / 255.0) + np.float32(-1.0)
        got = out[:n_out].view(3, -1).cpu()
        inside = got[1] != -1.0                                                          # (Y = U = V = 0 is a green, not black)
        assert inside.any() and all((got[c][inside] == float(want[c])).all() for c in range(3))
        assert (out[n_out:] == SENTINEL).all() and (out16[n_pk:] == SENTINEL16).all() and not (out16[:n_pk] == SENTINEL16).any()


# ------------------------------------------------------------------------------------------------ EyeNet / EVE / EVEStream
def both_forms(d, fmt, seed, T, matrix='bt601'):
    """d: a dict of [B, T, ...] GPU tensors -> (d with camera_frame_<fmt> and the warps, d with camera_frame = to_rgb of the same
    bytes and the warps), patch keys removed.  The warps are camera_clip's: every (stream, frame, eye) has its own."""
    _, lw, rw, _, _ = camera_clip(seed)
    B = lw.shape[0]
    buf = pref.random_yuv_frames(fmt, B * 6, CAM[0], CAM[1], seed)
    rgb = torch.from_numpy(pref.to_rgb(buf, fmt, matrix)).view((B, 6) + CAM + (3,))[:, :T].contiguous().cuda()
    raw = torch.from_numpy(buf).view((B, 6) + buf.shape[1:])[:, :T].contiguous().cuda()
    rest = {k_: v for k_, v in d.items() if k_ not in ('left_eye_patch', 'right_eye_patch')}
    warps = dict(left_eye_warp=lw[:, :T].contiguous().cuda(), right_eye_warp=rw[:, :T].contiguous().cuda())
    return dict(rest, **warps, **{'camera_frame_' + fmt: raw}), dict(rest, camera_frame=rgb, **warps)


def tensors(v):
    return v if isinstance(v, tuple) else (v,)


def same(got, want, where=None):
    assert set(got) == set(want)
    for key in want:
        if torch.is_tensor(want[key]) or isinstance(want[key], tuple):
            for a, b in zip(tensors(got[key]), tensors(want[key])):
                assert torch.equal(a, b), (where, key)


@pytest.mark.parametrize('fmt', ['nv12', 'yuyv'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_eyenet_takes_the_frame_as_the_camera_delivers_it(dtype, fmt):
    model, _ = make_model(dtype=dtype)
    _, d, _ = gpu_clip(2, 3, seed=5)
    raw, rgb = both_forms(d, fmt, 31, 3)
    with torch.no_grad():
        got = model.eye_net.forward_sequence(raw)
        want = model.eye_net.forward_sequence(rgb)
    assert tuple(got['left_g_initial'].shape) == (2, 3, 2) and torch.isfinite(got['left_g_initial']).all()
    same(got, want)
    model.eye_net.yuv_matrix = 'jfif'
    with torch.no_grad():
        other = model.eye_net.forward_sequence(raw)
        same(other, model.eye_net.forward_sequence(both_forms(d, fmt, 31, 3, matrix='jfif')[1]))
    assert not torch.equal(other['left_g_initial'], got['left_g_initial'])
    model.eye_net.yuv_matrix = 'nonsense'
    with pytest.raises(ValueError, match='yuv_matrix'):
        model.eye_net.forward_sequence(raw)
    with pytest.raises(ValueError, match='one camera frame key'):
        model.eye_net.forward_sequence(dict(raw, camera_frame=rgb['camera_frame']))


@pytest.mark.parametrize('fmt', ['nv12', 'yuyv'])
def test_eve_eval_takes_the_frame_as_the_camera_delivers_it(fmt):
    model, _ = make_model()
    _, _, full = gpu_clip(2, 3, seed=5)
    raw, rgb = both_forms(full, fmt, 31, 3)
    with torch.no_grad():
        got, want = model(raw), model(rgb)
    assert 'PoG_px_final' in got
    same(got, want)


@pytest.mark.parametrize('fmt', ['nv12', 'yuyv'])
def test_stream_replays_a_graph_over_the_frame_as_delivered(fmt):
    """B = 2, Tc = 2, refine_net config: two replays of one graph with different bytes equal the camera_frame graph stream on the
    converted frames bit for bit, and differ from each other; another matrix captures a graph of its own."""
    model, _ = make_model()
    _, d, _ = gpu_clip(2, 6, seed=5)
    raw, rgb = both_forms(d, fmt, 33, 6)
    ch = lambda src, i: {k_: v[:, 2 * i:2 * i + 2].contiguous() for k_, v in src.items()}
    g, c, e = eve_amd.EVEStream(model, 2), eve_amd.EVEStream(model, 2), eve_amd.EVEStream(model, 2, use_graph=False)
    outs = []
    for i in range(3):
        og = {k_: v.clone() for k_, v in g.step(ch(raw, i), return_heatmaps=True).items()}
        same(og, c.step(ch(rgb, i), return_heatmaps=True), i)
        same(og, e.step(ch(raw, i), return_heatmaps=True), i)
        outs.append(og)
    assert len(g._graphs) == 1 and len(c._graphs) == 1 and 'heatmap_final' in outs[0]
    assert not torch.equal(outs[0]['g_initial'], outs[1]['g_initial'])
    assert g._graphs[next(iter(g._graphs))]['inputs']['camera_frame_' + fmt].numel() * 3 <= rgb['camera_frame'][:, :2].numel() * 2
    model.eye_net.yuv_matrix = 'bt709'
    g.reset()
    hd = g.step(ch(raw, 0), return_heatmaps=True)
    assert len(g._graphs) == 2 and not torch.equal(hd['g_initial'], outs[0]['g_initial'])
    e2 = eve_amd.EVEStream(model, 2, use_graph=False)
    same(hd, e2.step(ch(both_forms(d, fmt, 33, 6, matrix='bt709')[1], 0), return_heatmaps=True))


def test_i420_with_pose_rows_a_lens_and_an_eye_mask():
    """camera_frame_i420 + eye_pose + camera_lens + eye_mask under graph replay equals camera_frame on the converted frames."""
    model, _ = make_model()
    _, d, _ = gpu_clip(2, 4, seed=5)
    rest = {k_: v for k_, v in d.items() if k_ not in ('left_eye_patch', 'right_eye_patch', 'left_h', 'right_h', 'left_o', 'right_o',
                                                      'left_R', 'right_R', 'head_R')}
    buf = pref.random_yuv_frames('i420', 8, CAM[0], CAM[1], seed=6)
    raw = torch.from_numpy(buf).view((2, 4) + buf.shape[1:]).cuda()
    rgb = torch.from_numpy(pref.to_rgb(buf, 'i420')).view((2, 4) + CAM + (3,)).cuda()
    common = dict(rest, eye_pose=cam_poses(2, 4, seed=7).cuda(), camera_lens=cam_lens(2, 4).cuda())
    mask = torch.tensor([[[1, 1], [0, 1], [1, 0], [1, 1]], [[1, 1], [1, 1], [0, 0], [1, 1]]], dtype=torch.bool)
    ch = lambda src, i: {k_: v[:, 2 * i:2 * i + 2].contiguous() for k_, v in src.items()}
    g, c = eve_amd.EVEStream(model, 2), eve_amd.EVEStream(model, 2)
    for i in range(2):
        m_ = mask[:, 2 * i:2 * i + 2]
        got = {k_: v.clone() for k_, v in g.step(ch(dict(common, camera_frame_i420=raw), i), eye_mask=m_).items()}
        want = c.step(ch(dict(common, camera_frame=rgb), i), eye_mask=m_)
        assert 'eye_valid' in got and 'pose_valid' in got and torch.equal(got['eye_valid'].cpu(), m_)
        valid, eye_valid = got['valid'], got['eye_valid']
        for key in want:
            a, b = got[key], want[key]
            if key.startswith(('left_', 'right_')) and key not in ('left_R',):
                sel = eye_valid[..., 0 if key.startswith('left_') else 1]
            else:
                sel = valid
            if a.shape[:2] == sel.shape and a.dtype.is_floating_point:
                assert torch.equal(a[sel], b[sel]), (i, key)
    assert len(g._graphs) == 1


# ------------------------------------------------------------------------------------------------ the screen
@pytest.mark.parametrize('shape,vec', [((1080, 1920, 4), True), ((768, 1366, 3), False)], ids=['1080p-bgra', '1366x768-bgr'])
def test_the_bgr_area_resize_equals_the_rgb_one_on_the_reversed_capture(shape, vec):
    k = default_kernels()
    SCREEN = (72, 128)
    cap = torch.from_numpy(np.random.default_rng(shape[0]).integers(0, 256, size=(2,) + shape, dtype=np.uint8)).cuda()
    rev = cap.clone()
    rev[..., 0], rev[..., 2] = cap[..., 2], cap[..., 0]
    n_out = 2 * 3 * SCREEN[0] * SCREEN[1]
    want = k.screen_u8_area_to_nchw(rev, SCREEN)
    assert k.lib.eve_last_kernel() == (b'screen_u8_area_kernel<true>' if vec else b'screen_u8_area_kernel<false>')
    for _ in range(2):
        out = torch.full((n_out + GUARD,), SENTINEL, dtype=torch.float32, device='cuda')
        assert k.lib.eve_screen_u8_area_bgr_to_nchw(2, shape[0], shape[1], shape[2], ptr(cap), SCREEN[0], SCREEN[1], ptr(out), stream_ptr()) == 0
        assert k.lib.eve_last_kernel() == (b'screen_u8_area_bgr_kernel<true>' if vec else b'screen_u8_area_bgr_kernel<false>')
        assert (out[n_out:] == SENTINEL).all() and torch.equal(out[:n_out].view(torch.int32), want.reshape(-1).view(torch.int32))
    assert not torch.equal(k.screen_u8_area_to_nchw(cap, SCREEN), want)
    assert torch.equal(k.screen_u8_area_bgr_to_nchw(cap, SCREEN), want)
    assert torch.equal(data.preprocess_screen_frames(cap.view((1, 2) + shape), size=SCREEN, bgr=True)[0], want)
    sentinel = torch.full((8,), SENTINEL, device='cuda')
    assert k.lib.eve_screen_u8_area_bgr_to_nchw(2, shape[0], shape[1], 2, ptr(cap), SCREEN[0], SCREEN[1], ptr(sentinel), stream_ptr()) != 0
    assert k.lib.eve_last_error().decode().startswith('screen_u8_area_bgr_to_nchw:') and (sentinel == SENTINEL).all()


def test_stream_takes_screen_frame_bgr_under_graph_replay():
    model, _ = make_model()
    _, d, _ = gpu_clip(2, 4, seed=5)
    rest = {k_: v for k_, v in d.items() if k_ != 'screen_frame'}
    cap = torch.from_numpy(np.random.default_rng(8).integers(0, 256, size=(2, 4, 144, 256, 4), dtype=np.uint8)).cuda()
    rev = cap[..., [2, 1, 0]].contiguous()
    ch = lambda src, i: {k_: v[:, 2 * i:2 * i + 2].contiguous() for k_, v in src.items()}
    g, c = eve_amd.EVEStream(model, 2), eve_amd.EVEStream(model, 2)
    for i in range(2):
        got = g.step(ch(dict(rest, screen_frame_bgr=cap), i), return_heatmaps=True)
        same(got, c.step(ch(dict(rest, screen_frame=rev), i), return_heatmaps=True), i)
    assert len(g._graphs) == 1
    with pytest.raises(ValueError, match='not both'):
        g.step(ch(dict(d, screen_frame_bgr=cap), 0))
