"""GPU: eve_eye_warp_u8_to_nchw / eve_eye_warp_u8_to_stem (csrc/eye_warp.hip) bit for bit against their contract in numpy
(tests/eye_warp_ref.py), and whole camera frames plus per-eye homographies through EyeNet.forward_sequence, EVE.forward and
EVEStream, eager and under graph replay."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import eve_amd
from eve_amd import data
from eve_amd.kernels import default_kernels, dt_code
import eye_warp_ref as ref
from test_gpu_stream import gpu_clip, make_model

pytestmark = pytest.mark.gpu
GUARD = 1024                  # elements behind the output that no launch may touch
SENTINEL = -7.0
SENTINEL16 = 0x5A5A
HW = (128, 128)
FRAME = (160, 200)            # (IH, IW) of the kernel cases unless stated
GRID_CAP, BAND = 1024, 2      # csrc/eye_warp.hip EW_MAX_BLOCKS / EW_BAND
NAMES = {torch.float32: b'eye_warp_u8_kernel<float>', torch.bfloat16: b'eye_warp_u8_kernel<eve::bf16_t>',
         torch.float16: b'eye_warp_u8_kernel<eve::f16_t>'}


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def raw_nchw(k, frames, warps, hw, out):
    N, IH, IW, C = frames.shape
    return k.lib.eve_eye_warp_u8_to_nchw(N, IH, IW, C, ctypes.c_void_p(frames.data_ptr()), ctypes.c_void_p(warps.data_ptr()), hw[0], hw[1],
                                         ctypes.c_void_p(out.data_ptr()), stream_ptr())


def raw_stem(k, dtype, frames, warps, hw, out):
    N, IH, IW, C = frames.shape
    return k.lib.eve_eye_warp_u8_to_stem(dt_code(dtype), N, IH, IW, C, ctypes.c_void_p(frames.data_ptr()), ctypes.c_void_p(warps.data_ptr()),
                                         hw[0], hw[1], ctypes.c_void_p(out.data_ptr()), stream_ptr())


def differing(got, want):
    bad = got != want
    return '%d of %d elements differ, first at flat index %d: got %r want %r' % (
        int(bad.sum()), got.numel(), int(bad.flatten().nonzero()[0]), int(got[bad][0]), int(want[bad][0]))


def check(k, v, m, hw, kind, packed=True, frames=None):
    """Both exports, two launches each into a guarded buffer, == the numpy contract with no tolerance on the integer view; the
    guard untouched; the kernel's name; the reference's outside share what the case claims.  -> (frames, warps on the GPU, want)."""
    N = v.shape[0]
    want, outside = ref.eye_warp(v, m, hw)
    assert ref.outside_share_ok(kind, float(outside.mean())), (kind, float(outside.mean()))
    want = torch.from_numpy(want)
    n_out = want.numel()
    frames = torch.from_numpy(v).cuda() if frames is None else frames
    warps = torch.from_numpy(m).cuda()
    for _ in range(2):
        out = torch.full((n_out + GUARD,), SENTINEL, dtype=torch.float32, device='cuda')
        assert raw_nchw(k, frames, warps, hw, out) == 0, k.lib.eve_last_error()
        assert k.lib.eve_last_kernel() == NAMES[torch.float32]
        got = out.cpu()
        assert torch.equal(got[n_out:], torch.full((GUARD,), SENTINEL)), 'guard overwritten'
        gi, wi = got[:n_out].view(torch.int32), want.reshape(-1).view(torch.int32)
        assert torch.equal(gi, wi), differing(gi, wi)
    if not packed:
        return frames, warps, want
    for dtype in (torch.bfloat16, torch.float16):
        wp = ref.pack_stem(want, dtype)
        n_pk = wp.numel()
        for _ in range(2):
            out = torch.full((n_pk + GUARD,), SENTINEL16, dtype=torch.int16, device='cuda')
            assert raw_stem(k, dtype, frames, warps, hw, out) == 0, k.lib.eve_last_error()
            assert k.lib.eve_last_kernel() == NAMES[dtype]
            got = out.cpu()
            assert (got[n_pk:] == SENTINEL16).all(), 'guard overwritten'
            gi, wi = got[:n_pk], wp.reshape(-1).view(torch.int16)
            assert torch.equal(gi, wi), differing(gi, wi)
            img = got[:n_pk].view(N, hw[0] + 6, hw[1] + 8, 4)
            ring = img.clone()
            ring[:, 3:hw[0] + 3, 4:hw[1] + 4] = 0
            assert not ring.any() and not img[..., 3].any()                  # the pad ring and the fourth channel
    return frames, warps, want


# ------------------------------------------------------------------------------------------------ the kernel against its contract
@pytest.mark.parametrize('name', list(ref.WARPS))
def test_kernel_equals_the_contract(name):
    m, kind = ref.WARPS[name]
    m = np.stack([m, m])
    k = default_kernels()
    v = ref.random_frames(2, FRAME[0], FRAME[1], 3, seed=len(name))
    frames, warps, want = check(k, v, m, HW, kind)
    check(k, ref.checkerboard_frames(2, FRAME[0], FRAME[1], 3), m, HW, kind)
    via = k.eye_warp_u8_to_nchw(frames, warps, HW)                     # the tensor-level wrappers
    assert via.dtype == torch.float32 and tuple(via.shape) == (2, 3) + HW and torch.equal(via.cpu(), want)
    pk = k.eye_warp_u8_to_stem(frames, warps, HW, dtype=torch.float16)
    assert pk.dtype == torch.float16 and torch.equal(pk.cpu().view(torch.int16), ref.pack_stem(want, torch.float16).view(torch.int16))
    if name == 'integer-shift':                                        # the bits of the plain normalisation on the crop
        tx, ty = int(m[0, 0, 2]), int(m[0, 1, 2])
        crop = frames[:, ty:ty + HW[0], tx:tx + HW[1]].contiguous()
        assert torch.equal(via, k.frames_u8_to_nchw(crop, 2.0 / 255.0, -1.0))
        for dtype in (torch.bfloat16, torch.float16):
            a = k.eye_warp_u8_to_stem(frames, warps, HW, dtype=dtype)
            b = k.frames_u8_to_stem(crop, 2.0 / 255.0, -1.0, dtype=dtype)
            assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize('name', ['nan', 'off-frame'])
def test_a_nan_matrix_and_an_off_frame_one_give_minus_one(name):
    m = {'nan': ref.NAN_WARP, 'off-frame': ref.OFF_FRAME_WARP}[name]
    k = default_kernels()
    v = ref.random_frames(1, FRAME[0], FRAME[1], 3, seed=2)
    frames, warps, want = check(k, v, m[None], HW, 'all')
    assert (want == -1.0).all()
    pk = k.eye_warp_u8_to_stem(frames, warps, HW).cpu().float()
    assert (pk[:, 3:-3, 4:-4, :3] == -1.0).all() and (pk[:, 3:-3, 4:-4, 3] == 0.0).all()


def test_a_fourth_channel_leaves_no_trace():
    k = default_kernels()
    v = ref.random_frames(2, FRAME[0], FRAME[1], 4, seed=4)
    assert (v[..., 3] == 255).all()
    m = np.stack([ref.WARPS['rotated-perspective'][0], ref.WARPS['fractional-shift'][0]])
    _, warps, want = check(k, v, m, HW, 'few')
    rgb = torch.from_numpy(np.ascontiguousarray(v[..., :3])).cuda()
    assert torch.equal(k.eye_warp_u8_to_nchw(rgb, warps, HW).cpu(), want)


def test_full_hd_frames():
    """N = 2 frames of 1080 x 1920, scale 1.4, rotated by 10 degrees, with a perspective row: all inside."""
    k = default_kernels()
    v = ref.random_frames(2, 1080, 1920, 3, seed=5)
    m = np.stack([ref.similarity(1.4, 10.0, 800.0, 400.0, persp=(1e-4, -2e-4)), ref.similarity(1.4, -10.0, 1000.0, 500.0, persp=(-1e-4, 2e-4))])
    check(k, v, m, HW, 'none')


@pytest.mark.parametrize('hw,m', [((36, 60), ref.shift(72.5, 100.25)), ((256, 256), ref.similarity(0.5, 0.0, 10.0, 5.0))], ids=['36x60', '256x256'])
def test_other_patch_sizes_through_the_float_form(hw, m):
    k = default_kernels()
    v = ref.random_frames(2, FRAME[0], FRAME[1], 3, seed=hw[0])
    frames, warps, want = check(k, v, np.stack([m, m]), hw, 'none', packed=False)
    check(k, ref.checkerboard_frames(2, FRAME[0], FRAME[1], 3), np.stack([m, m]), hw, 'none', packed=False)
    assert torch.equal(data.warp_eye_patches(frames.view((1, 2) + tuple(frames.shape[1:])), warps.view(1, 2, 3, 3), size=hw).cpu()[0], want)


def test_more_items_than_the_grid():
    """N = 70 patches of 32 x 128 from 64 x 160 frames, each with its own shift (whole and fractional): 70 * 16 = 1 120 bands in the
    float form and 70 * 19 = 1 330 in the packed one, against a grid of 1 024 workgroups."""
    N, hw = 70, (32, 128)
    assert N * (hw[0] // BAND) > GRID_CAP and N * ((hw[0] + 6) // BAND) > GRID_CAP
    k = default_kernels()
    g = np.random.default_rng(70)
    m = np.stack([ref.shift(float(g.integers(0, 128)) / 4, float(g.integers(0, 128)) / 4) for _ in range(N)])
    check(k, ref.random_frames(N, 64, 160, 3, seed=70), m, hw, 'none')
    check(k, ref.checkerboard_frames(N, 64, 160, 3), m, hw, 'none')


def test_an_unaligned_frame_pointer():
    k = default_kernels()
    v = ref.random_frames(2, FRAME[0], FRAME[1], 3, seed=3)
    buf = torch.zeros((v.size + 16,), dtype=torch.uint8, device='cuda')
    frames = buf[4:4 + v.size].view(v.shape)
    frames.copy_(torch.from_numpy(v))
    assert frames.data_ptr() % 16 == 4 and frames.is_contiguous()
    m, kind = ref.WARPS['rotated-perspective']
    check(k, v, np.stack([m, m]), HW, kind, frames=frames)


def test_refused_requests_launch_nothing():
    k = default_kernels()
    frames = torch.zeros((1, 90, 160, 3), dtype=torch.uint8, device='cuda')
    warps = torch.from_numpy(ref.shift(0, 0)[None]).cuda()
    hw = (36, 60)
    k.stream_state_rows(torch.zeros((2, 8), device='cuda'), torch.zeros((2, 8), device='cuda'))     # the last named launch
    before = k.lib.eve_last_kernel()
    assert b'eye_warp' not in before
    n_out, n_pk = 3 * hw[0] * hw[1], (hw[0] + 6) * (hw[1] + 8) * 4
    out = torch.full((n_out + GUARD,), SENTINEL, dtype=torch.float32, device='cuda')
    out16 = torch.full((n_pk + GUARD,), SENTINEL16, dtype=torch.int16, device='cuda')
    p, w, s = ctypes.c_void_p(frames.data_ptr()), ctypes.c_void_p(warps.data_ptr()), stream_ptr()
    o, o16 = ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(out16.data_ptr())
    bf16 = dt_code(torch.bfloat16)
    nchw = lambda N, IH, IW, C, OH, OW, a=p, b=w, c=o: k.lib.eve_eye_warp_u8_to_nchw(N, IH, IW, C, a, b, OH, OW, c, s)
    stem = lambda N, IH, IW, C, OH, OW, a=p, b=w, c=o16, dt=bf16: k.lib.eve_eye_warp_u8_to_stem(dt, N, IH, IW, C, a, b, OH, OW, c, s)
    cases = {'two channels': ((1, 90, 160, 2) + hw, 'C must be'), 'no frames': ((0, 90, 160, 3) + hw, 'bad arguments'),
             'frame too wide': ((1, 90, 16385, 3) + hw, 'frame too large'), 'frame too high': ((1, 16385, 160, 3) + hw, 'frame too large'),
             'patch too high': ((1, 90, 160, 3, 4097, 60), 'patch too large'), 'patch too wide': ((1, 90, 160, 3, 36, 4097), 'patch too large')}
    for fn, prefix in ((nchw, 'eye_warp_u8_to_nchw:'), (stem, 'eye_warp_u8_to_stem:')):
        for name, (args, word) in cases.items():
            assert fn(*args) != 0, name
            msg = k.lib.eve_last_error().decode()
            assert msg.startswith(prefix) and word in msg, (name, msg)
            assert k.lib.eve_last_kernel() == before, name
        for nulls in (dict(a=None), dict(b=None), dict(c=None)):
            assert fn(1, 90, 160, 3, *hw, **nulls) != 0
            assert k.lib.eve_last_error().decode().startswith(prefix) and k.lib.eve_last_kernel() == before
    assert stem(1, 90, 160, 3, *hw, dt=dt_code(torch.float32)) != 0                     # the packed form is 16-bit only
    msg = k.lib.eve_last_error().decode()
    assert msg.startswith('eye_warp_u8_to_stem:') and 'dtype' in msg and k.lib.eve_last_kernel() == before
    torch.cuda.synchronize()
    assert (out.cpu() == SENTINEL).all() and (out16.cpu() == SENTINEL16).all()
    with pytest.raises(RuntimeError, match='frame too large'):
        k.eye_warp_u8_to_nchw(torch.zeros((1, 1, 1, 3), dtype=torch.uint8, device='cuda').expand(1, 1, 16385, 3).contiguous(), warps, hw)
    with pytest.raises(TypeError):
        k.eye_warp_u8_to_nchw(frames, warps.double(), hw)
    with pytest.raises(TypeError):
        k.eye_warp_u8_to_stem(frames, warps, hw, out=torch.empty((1, hw[0] + 6, hw[1] + 8, 4), device='cuda'))
    assert nchw(1, 90, 160, 3, *hw) == 0 and stem(1, 90, 160, 3, *hw) == 0             # the same calls with sound arguments are taken
    assert (out[:n_out] == -1.0).all() and (out[n_out:] == SENTINEL).all()             # (a black frame)
    assert (out16[n_pk:] == SENTINEL16).all() and not (out16[:n_pk] == SENTINEL16).any()


# ------------------------------------------------------------------------------------------------ EyeNet / EVE / EVEStream
CAM = (270, 480)


@functools.lru_cache(maxsize=None)
def camera_clip(seed, B=2, T=6, integer=False):
    """-> (camera_frame uint8 [B, T, 270, 480, 3], left and right warps [B, T, 3, 3], the contract's float patches of both eyes), on
    the CPU.  Every (stream, frame, eye) has its own warp; the patches stay inside the frame."""
    g = np.random.default_rng(seed)
    frames = ref.random_frames(B * T, CAM[0], CAM[1], 3, seed)
    sides = []
    for _ in range(2):
        if integer:
            m = np.stack([ref.shift(int(g.integers(0, CAM[1] - 128)), int(g.integers(0, CAM[0] - 128))) for _ in range(B * T)])
        else:
            m = np.stack([ref.similarity(float(g.uniform(0.8, 1.0)), float(g.uniform(-8, 8)), float(g.uniform(60, 300)), float(g.uniform(30, 100)),
                                         persp=(float(g.uniform(-1e-4, 1e-4)), float(g.uniform(-1e-4, 1e-4)))) for _ in range(B * T)])
        vals, outside = ref.eye_warp(frames, m, HW)
        assert not outside.any()
        sides.append((torch.from_numpy(m).view(B, T, 3, 3), torch.from_numpy(vals).view((B, T, 3) + HW)))
    return torch.from_numpy(frames).view((B, T) + CAM + (3,)), sides[0][0], sides[1][0], sides[0][1], sides[1][1]


def both_forms(d, seed, T, integer=False):
    """d: a dict of [B, T, ...] GPU tensors -> (d with the camera keys, d with the contract's float patches), patch keys replaced."""
    frames, lw, rw, lp, rp = (t[:, :T].contiguous().cuda() for t in camera_clip(seed, integer=integer))
    rest = {k_: v for k_, v in d.items() if k_ not in ('left_eye_patch', 'right_eye_patch')}
    return dict(rest, camera_frame=frames, left_eye_warp=lw, right_eye_warp=rw), dict(rest, left_eye_patch=lp, right_eye_patch=rp)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_eyenet_takes_camera_frames(dtype):
    model, _ = make_model(dtype=dtype)
    k = default_kernels()
    _, d, _ = gpu_clip(2, 3, seed=5)
    for integer in (False, True):
        cam, pat = both_forms(d, 31, 3, integer=integer)
        with torch.no_grad():
            got = model.eye_net.forward_sequence(cam)
            want = model.eye_net.forward_sequence(pat)
        assert set(got) == set(want) and tuple(got['left_g_initial'].shape) == (2, 3, 2)
        for key in want:
            for a, b in zip(got[key] if isinstance(got[key], tuple) else (got[key],), want[key] if isinstance(want[key], tuple) else (want[key],)):
                assert torch.isfinite(a).all() and torch.equal(a, b), (integer, key)
        if integer:                                                     # ... and the run fed the uint8 crops
            def crops(w):
                f, w = cam['camera_frame'], w.cpu()
                rows = [f[b, t, int(w[b, t, 1, 2]):int(w[b, t, 1, 2]) + 128, int(w[b, t, 0, 2]):int(w[b, t, 0, 2]) + 128] for b in range(2) for t in range(3)]
                return torch.stack(rows).view(2, 3, 128, 128, 3).contiguous()
            with torch.no_grad():
                u8 = model.eye_net.forward_sequence(dict(pat, left_eye_patch=crops(cam['left_eye_warp']), right_eye_patch=crops(cam['right_eye_warp'])))
            for key in want:
                for a, b in zip(got[key] if isinstance(got[key], tuple) else (got[key],), u8[key] if isinstance(u8[key], tuple) else (u8[key],)):
                    assert torch.equal(a, b), key


def test_eve_eval_takes_camera_frames():
    model, _ = make_model()
    _, _, full = gpu_clip(2, 3, seed=5)
    cam, pat = both_forms(full, 31, 3)
    with torch.no_grad():
        got, want = model(cam), model(pat)
    assert set(got) == set(want) and 'PoG_px_final' in got
    for key in want:
        if torch.is_tensor(want[key]):
            assert torch.equal(got[key], want[key]), key


def test_stream_replays_a_graph_over_camera_frames():
    """B = 2, Tc = 2, refine_net config.  Three steps, the third ragged: the graph's outputs are the eager step's bit for bit, and
    two graphs are captured; the second step replays the first one's graph with other frames and other warps, and gives their
    result, not the first warps' (the graph reads its input buffers).  The camera form's chunks equal the float-patch form's chunks
    bit for bit, and -- to the bounds tests/test_gpu_stream.py::test_stream_float32_matches_the_whole_clip states for chunks against a
    whole clip -- one eval pass of the whole clip."""
    model, _ = make_model()
    _, d, full = gpu_clip(2, 6, seed=5)
    cam, pat = both_forms(d, 33, 6)
    ch = lambda src, i: {k_: v[:, 2 * i:2 * i + 2].contiguous() for k_, v in src.items()}
    g, e = eve_amd.EVEStream(model, 2), eve_amd.EVEStream(model, 2, use_graph=False)
    outs = []
    for i, lengths in enumerate((None, None, [1, 2])):
        og = {k_: v.clone() for k_, v in g.step(ch(cam, i), return_heatmaps=True, lengths=lengths).items()}
        oe = e.step(ch(cam, i), return_heatmaps=True, lengths=lengths)
        assert set(og) == set(oe) and 'heatmap_final' in og
        for k_ in og:
            assert torch.equal(og[k_], oe[k_]), (i, k_)
        outs.append(og)
    assert len(g._graphs) == 2                                       # one uniform graph replayed twice, one ragged
    e2 = eve_amd.EVEStream(model, 2, use_graph=False)
    e2.step(ch(cam, 0))
    first_warps = {k_: ch(cam, 0)[k_] for k_ in ('left_eye_warp', 'right_eye_warp')}
    other = e2.step(dict(ch(cam, 1), **first_warps))
    assert not torch.equal(other['g_initial'], outs[1]['g_initial'])
    # uniform chunks of the whole clip: the same graph stream from zero state, the float-patch form beside it
    g.reset()
    p = eve_amd.EVEStream(model, 2)
    whole_cam, whole_pat = [], []
    for i in range(3):
        whole_cam.append({k_: v.clone() for k_, v in g.step(ch(cam, i)).items()})
        whole_pat.append({k_: v.clone() for k_, v in p.step(ch(pat, i)).items()})
    assert len(g._graphs) == 3                                       # (without heat-maps: one more key)
    cat = {k_: torch.cat([o[k_] for o in whole_cam], dim=1) for k_ in whole_cam[0]}
    for k_ in cat:
        assert torch.equal(cat[k_], torch.cat([o[k_] for o in whole_pat], dim=1)), k_
    with torch.no_grad():
        whole = model(both_forms(full, 33, 6)[0])
    for k_, v in cat.items():
        if k_ in whole:
            amp = 5.0 if k_.endswith('_final') else 1.0
            err = float((v.float() - whole[k_].float()).abs().max())
            assert err <= amp * (1e-2 if 'px' in k_ else (1e-3 if 'cm' in k_ else 1e-5)), (k_, err)
