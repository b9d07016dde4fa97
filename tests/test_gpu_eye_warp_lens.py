"""GPU: eve_eye_warp_lens_u8_to_nchw / eve_eye_warp_lens_u8_to_stem (csrc/eye_warp.hip) bit for bit against their contract in numpy
(tests/eye_warp_lens_ref.py), and RAW camera frames plus per-eye homographies plus the camera's lens rows through
EyeNet.forward_sequence, EVE.forward and EVEStream, eager and under graph replay."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import eve_amd
from eve_amd import data
from eve_amd.kernels import default_kernels, dt_code
import eye_warp_lens_ref as lref
import eye_warp_ref as ref
from test_gpu_eye_warp import BAND, CAM, FRAME, GRID_CAP, GUARD, HW, SENTINEL, SENTINEL16, differing, stream_ptr
from test_gpu_eye_warp import NAMES as PLAIN_NAMES
from test_gpu_stream import gpu_clip, make_model

pytestmark = pytest.mark.gpu
NAMES = {torch.float32: b'eye_warp_lens_u8_kernel<float>', torch.bfloat16: b'eye_warp_lens_u8_kernel<eve::bf16_t>',
         torch.float16: b'eye_warp_lens_u8_kernel<eve::f16_t>'}


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def raw_lens_nchw(k, frames, warps, lens, hw, out):
    N, IH, IW, C = frames.shape
    return k.lib.eve_eye_warp_lens_u8_to_nchw(N, IH, IW, C, ptr(frames), ptr(warps), ptr(lens), hw[0], hw[1], ptr(out), stream_ptr())


def raw_lens_stem(k, dtype, frames, warps, lens, hw, out):
    N, IH, IW, C = frames.shape
    return k.lib.eve_eye_warp_lens_u8_to_stem(dt_code(dtype), N, IH, IW, C, ptr(frames), ptr(warps), ptr(lens), hw[0], hw[1], ptr(out), stream_ptr())


def check(k, v, m, L, hw, kind, packed=True, frames=None):
    """Both lens exports, two launches each into a guarded buffer, == the numpy contract with no tolerance on the integer view; the
    guard untouched; the kernel's name; the reference's outside share what the case claims; the pad ring and the fourth channel
    zero in the packed forms.  -> (frames, warps, lens on the GPU, want)."""
    N = v.shape[0]
    want, outside = lref.eye_warp(v, m, L, hw)
    assert ref.outside_share_ok(kind, float(outside.mean())), (kind, float(outside.mean()))
    want = torch.from_numpy(want)
    n_out = want.numel()
    frames = torch.from_numpy(v).cuda() if frames is None else frames
    warps, lens = torch.from_numpy(m).cuda(), torch.from_numpy(L).cuda()
    for _ in range(2):
        out = torch.full((n_out + GUARD,), SENTINEL, dtype=torch.float32, device='cuda')
        assert raw_lens_nchw(k, frames, warps, lens, hw, out) == 0, k.lib.eve_last_error()
        assert k.lib.eve_last_kernel() == NAMES[torch.float32]
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
            assert raw_lens_stem(k, dtype, frames, warps, lens, hw, out) == 0, k.lib.eve_last_error()
            assert k.lib.eve_last_kernel() == NAMES[dtype]
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
def test_kernel_equals_the_contract_with_barrel5(name):
    m = np.stack([ref.WARPS[name][0]] * 2)
    L = np.stack([lref.LENSES['barrel5']] * 2)
    kind = lref.outside_kind('barrel5', name)
    k = default_kernels()
    v = ref.random_frames(2, FRAME[0], FRAME[1], 3, seed=len(name))
    frames, warps, lens, want = check(k, v, m, L, HW, kind)
    check(k, ref.checkerboard_frames(2, FRAME[0], FRAME[1], 3), m, L, HW, kind)
    via = k.eye_warp_lens_u8_to_nchw(frames, warps, lens, HW)              # the tensor-level wrappers
    assert via.dtype == torch.float32 and tuple(via.shape) == (2, 3) + HW and torch.equal(via.cpu(), want)
    pk = k.eye_warp_lens_u8_to_stem(frames, warps, lens, HW, dtype=torch.float16)
    assert pk.dtype == torch.float16 and torch.equal(pk.cpu().view(torch.int16), ref.pack_stem(want, torch.float16).view(torch.int16))
    assert not torch.equal(via, k.eye_warp_u8_to_nchw(frames, warps, HW))  # (the lens moves the patch)
    assert k.lib.eve_last_kernel() == PLAIN_NAMES[torch.float32]           # ... and the plain export keeps its kernel
    assert torch.equal(data.warp_eye_patches(frames.view((1, 2) + tuple(frames.shape[1:])), warps.view(1, 2, 3, 3), size=HW,
                                             lens=lens.view(1, 2, 12)).cpu()[0], want)


@pytest.mark.parametrize('name', ['integer-shift', 'fractional-shift'])
@pytest.mark.parametrize('lens_name', ['rational8', 'tangential', 'pole'])
def test_rational_tangential_and_pole_lenses(lens_name, name):
    m = np.stack([ref.WARPS[name][0]] * 2)
    L = np.stack([lref.LENSES[lens_name]] * 2)
    kind = lref.outside_kind(lens_name, name)
    k = default_kernels()
    check(k, ref.random_frames(2, FRAME[0], FRAME[1], 3, seed=len(lens_name)), m, L, HW, kind)
    check(k, ref.checkerboard_frames(2, FRAME[0], FRAME[1], 3), m, L, HW, kind)


def test_a_mixed_batch_in_one_launch():
    """N = 70 patches of 32 x 128 from 64 x 160 frames, each with its own fractional shift: 70 * 16 = 1 120 bands in the float form and
    70 * 19 = 1 330 in the packed one, against a grid of 1 024 workgroups, so a workgroup takes a lens patch right after a plain one.
    Rows alternate among barrel5 with its intrinsics rescaled to the frame, a zero-coefficient row with intrinsics of its own,
    and a NaN row (24 of 70 patches black: 'some').  The zero rows' patches are the plain export's, the NaN rows' -1.0."""
    N, hw = 70, (32, 128)
    assert N * (hw[0] // BAND) > GRID_CAP and N * ((hw[0] + 6) // BAND) > GRID_CAP
    k = default_kernels()
    g = np.random.default_rng(70)
    m = np.stack([ref.shift(float(g.integers(0, 128)) / 4, float(g.integers(0, 128)) / 4) for _ in range(N)])
    b5 = lref.LENSES['barrel5'].copy()
    b5[:4] = (144, 144, 80, 32)                  # 0.8 * 180, the principal point at the frame's centre
    kinds = [b5, lref.lens_row(3, -7, 1e6, 0, k2=-0.0), np.full((12,), np.nan, dtype=np.float32)]
    L = np.stack([kinds[(n + n // 3) % 3] for n in range(N)])           # (not a fixed period of three against the grid stride)
    which = np.array([(n + n // 3) % 3 for n in range(N)])
    assert [int((which == i).sum()) for i in range(3)] == [23, 23, 24]
    for v in (ref.random_frames(N, 64, 160, 3, seed=70), ref.checkerboard_frames(N, 64, 160, 3)):
        frames, warps, lens, want = check(k, v, m, L, hw, 'some')
        plain = k.eye_warp_u8_to_nchw(frames, warps, hw)
        assert k.lib.eve_last_kernel() == PLAIN_NAMES[torch.float32]
        got = k.eye_warp_lens_u8_to_nchw(frames, warps, lens, hw)
        zero, nan, lensed = (torch.from_numpy(np.flatnonzero(which == i)).cuda() for i in (1, 2, 0))
        assert torch.equal(got[zero].view(torch.int32), plain[zero].view(torch.int32))
        assert (got[nan] == -1.0).all()
        assert not torch.equal(got[lensed], plain[lensed])
        for dtype in (torch.bfloat16, torch.float16):
            a = k.eye_warp_lens_u8_to_stem(frames, warps, lens, hw, dtype=dtype)
            b = k.eye_warp_u8_to_stem(frames, warps, hw, dtype=dtype)
            assert torch.equal(a[zero].view(torch.int16), b[zero].view(torch.int16))
            assert (a[nan][:, 3:-3, 4:-4, :3].float() == -1.0).all()


def test_a_fourth_channel_leaves_no_trace():
    k = default_kernels()
    v = ref.random_frames(2, FRAME[0], FRAME[1], 4, seed=4)
    assert (v[..., 3] == 255).all()
    m = np.stack([ref.WARPS['rotated-perspective'][0], ref.WARPS['fractional-shift'][0]])
    L = np.stack([lref.LENSES['barrel5'], lref.LENSES['rational8']])
    _, warps, lens, want = check(k, v, m, L, HW, 'few')
    rgb = torch.from_numpy(np.ascontiguousarray(v[..., :3])).cuda()
    assert torch.equal(k.eye_warp_lens_u8_to_nchw(rgb, warps, lens, HW).cpu(), want)


def test_an_unaligned_frame_pointer():
    k = default_kernels()
    v = ref.random_frames(2, FRAME[0], FRAME[1], 3, seed=3)
    buf = torch.zeros((v.size + 16,), dtype=torch.uint8, device='cuda')
    frames = buf[4:4 + v.size].view(v.shape)
    frames.copy_(torch.from_numpy(v))
    assert frames.data_ptr() % 16 == 4 and frames.is_contiguous()
    m = ref.WARPS['rotated-perspective'][0]
    check(k, v, np.stack([m, m]), np.stack([lref.LENSES['barrel5']] * 2), HW, lref.outside_kind('barrel5', 'rotated-perspective'), frames=frames)


def test_full_hd_frames():
    """N = 2 frames of 1080 x 1920 behind fx = fy = 1400, cx = 960, cy = 540, k1 = -0.12, k2 = 0.03; the plain full-HD test's warps
    (scale 1.4, +-10 degrees, a perspective row): all inside."""
    k = default_kernels()
    v = ref.random_frames(2, 1080, 1920, 3, seed=5)
    m = np.stack([ref.similarity(1.4, 10.0, 800.0, 400.0, persp=(1e-4, -2e-4)), ref.similarity(1.4, -10.0, 1000.0, 500.0, persp=(-1e-4, 2e-4))])
    L = np.stack([lref.lens_row(1400, 1400, 960, 540, k1=-0.12, k2=0.03)] * 2)
    check(k, v, m, L, HW, 'none')


def test_refused_requests_launch_nothing():
    k = default_kernels()
    frames = torch.zeros((1, 90, 160, 3), dtype=torch.uint8, device='cuda')
    warps = torch.from_numpy(ref.shift(0, 0)[None]).cuda()
    lens = torch.from_numpy(lref.lens_row(150, 150, 80, 45, k1=-0.2)[None]).cuda()
    hw = (36, 60)
    k.stream_state_rows(torch.zeros((2, 8), device='cuda'), torch.zeros((2, 8), device='cuda'))     # the last named launch
    before = k.lib.eve_last_kernel()
    assert b'eye_warp' not in before
    n_out, n_pk = 3 * hw[0] * hw[1], (hw[0] + 6) * (hw[1] + 8) * 4
    out = torch.full((n_out + GUARD,), SENTINEL, dtype=torch.float32, device='cuda')
    out16 = torch.full((n_pk + GUARD,), SENTINEL16, dtype=torch.int16, device='cuda')
    p, w, l_, s = ptr(frames), ptr(warps), ptr(lens), stream_ptr()
    o, o16 = ptr(out), ptr(out16)
    bf16 = dt_code(torch.bfloat16)
    nchw = lambda N, IH, IW, C, OH, OW, a=p, b=w, c=o, d=l_: k.lib.eve_eye_warp_lens_u8_to_nchw(N, IH, IW, C, a, b, d, OH, OW, c, s)
    stem = lambda N, IH, IW, C, OH, OW, a=p, b=w, c=o16, d=l_, dt=bf16: k.lib.eve_eye_warp_lens_u8_to_stem(dt, N, IH, IW, C, a, b, d, OH, OW, c, s)
    cases = {'two channels': ((1, 90, 160, 2) + hw, 'C must be'), 'no frames': ((0, 90, 160, 3) + hw, 'bad arguments'),
             'frame too wide': ((1, 90, 16385, 3) + hw, 'frame too large'), 'frame too high': ((1, 16385, 160, 3) + hw, 'frame too large'),
             'patch too high': ((1, 90, 160, 3, 4097, 60), 'patch too large'), 'patch too wide': ((1, 90, 160, 3, 36, 4097), 'patch too large')}
    for fn, prefix in ((nchw, 'eye_warp_lens_u8_to_nchw:'), (stem, 'eye_warp_lens_u8_to_stem:')):
        for name, (args, word) in cases.items():
            assert fn(*args) != 0, name
            msg = k.lib.eve_last_error().decode()
            assert msg.startswith(prefix) and word in msg, (name, msg)
            assert k.lib.eve_last_kernel() == before, name
        for nulls in (dict(d=None), dict(a=None), dict(b=None), dict(c=None)):               # a NULL lens first
            assert fn(1, 90, 160, 3, *hw, **nulls) != 0
            assert k.lib.eve_last_error().decode().startswith(prefix) and k.lib.eve_last_kernel() == before
    assert stem(1, 90, 160, 3, *hw, dt=dt_code(torch.float32)) != 0                     # the packed form is 16-bit only
    msg = k.lib.eve_last_error().decode()
    assert msg.startswith('eye_warp_lens_u8_to_stem:') and 'dtype' in msg and k.lib.eve_last_kernel() == before
    torch.cuda.synchronize()
    assert (out.cpu() == SENTINEL).all() and (out16.cpu() == SENTINEL16).all()
    with pytest.raises(TypeError, match='lens'):
        k.eye_warp_lens_u8_to_nchw(frames, warps, lens.double(), hw)
    with pytest.raises(TypeError, match='lens'):
        k.eye_warp_lens_u8_to_nchw(frames, warps, lens[:, :5].contiguous(), hw)
    with pytest.raises(TypeError, match='lens'):
        k.eye_warp_lens_u8_to_stem(frames, warps, lens.double(), hw)
    with pytest.raises(TypeError, match='lens'):
        k.eye_warp_lens_u8_to_stem(frames, warps, torch.zeros((1, 5), device='cuda'), hw)
    with pytest.raises(TypeError):
        k.eye_warp_lens_u8_to_nchw(frames, warps.double(), lens, hw)
    with pytest.raises(TypeError):
        k.eye_warp_lens_u8_to_stem(frames, warps, lens, hw, out=torch.empty((1, hw[0] + 6, hw[1] + 8, 4), device='cuda'))
    with pytest.raises(RuntimeError):
        k.eye_warp_lens_u8_to_nchw(frames, warps, lens.cpu(), hw)
    assert k.lib.eve_last_kernel() == before
    assert nchw(1, 90, 160, 3, *hw) == 0 and stem(1, 90, 160, 3, *hw) == 0             # the same calls with sound arguments are taken
    assert (out[:n_out] == -1.0).all() and (out[n_out:] == SENTINEL).all()             # (a black frame)
    assert (out16[n_pk:] == SENTINEL16).all() and not (out16[:n_pk] == SENTINEL16).any()


# ------------------------------------------------------------------------------------------------ EyeNet / EVE / EVEStream
def cam_lens(g, k1=-0.25):
    """A barrel5-like camera for CAM-sized frames, its centre and focal lengths jittered."""
    return lref.lens_row(430 + g.uniform(-10, 10), 430 + g.uniform(-10, 10), CAM[1] / 2 + g.uniform(-5, 5), CAM[0] / 2 + g.uniform(-5, 5),
                         k1=k1 + g.uniform(-0.02, 0.02), k2=0.08, p1=1e-3, p2=-5e-4, k3=-0.01)


@functools.lru_cache(maxsize=None)
def lens_clip(seed, B=2, T=6, k1=-0.25):
    """-> (camera_frame uint8 [B, T, 270, 480, 3], left and right warps [B, T, 3, 3], camera_lens [B, T, 12], the lens contract's float
    patches of both eyes), on the CPU.  Every (stream, frame, eye) has its own warp and every (stream, frame) its own camera; at most
    a sliver of a patch leaves the frame."""
    g = np.random.default_rng(seed)
    frames = ref.random_frames(B * T, CAM[0], CAM[1], 3, seed)
    L = np.stack([cam_lens(g, k1) for _ in range(B * T)])
    sides = []
    for _ in range(2):
        m = np.stack([ref.similarity(float(g.uniform(0.8, 1.0)), float(g.uniform(-8, 8)), float(g.uniform(60, 300)), float(g.uniform(30, 100)),
                                     persp=(float(g.uniform(-1e-4, 1e-4)), float(g.uniform(-1e-4, 1e-4)))) for _ in range(B * T)])
        vals, outside = lref.eye_warp(frames, m, L, HW)
        assert outside.mean() < 0.05
        assert not np.array_equal(vals, ref.eye_warp(frames, m, HW)[0])
        sides.append((torch.from_numpy(m).view(B, T, 3, 3), torch.from_numpy(vals).view((B, T, 3) + HW)))
    return (torch.from_numpy(frames).view((B, T) + CAM + (3,)), sides[0][0], sides[1][0], torch.from_numpy(L).view(B, T, 12),
            sides[0][1], sides[1][1])


def both_forms(d, seed, T, k1=-0.25):
    """d: a dict of [B, T, ...] GPU tensors -> (d with the camera keys and camera_lens, d with the lens contract's float patches)."""
    frames, lw, rw, lens, lp, rp = (t[:, :T].contiguous().cuda() for t in lens_clip(seed, k1=k1))
    rest = {k_: v for k_, v in d.items() if k_ not in ('left_eye_patch', 'right_eye_patch')}
    return (dict(rest, camera_frame=frames, left_eye_warp=lw, right_eye_warp=rw, camera_lens=lens),
            dict(rest, left_eye_patch=lp, right_eye_patch=rp))


def tensors(v):
    return v if isinstance(v, tuple) else (v,)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_eyenet_takes_raw_frames_and_a_lens(dtype):
    model, _ = make_model(dtype=dtype)
    _, d, _ = gpu_clip(2, 3, seed=5)
    cam, pat = both_forms(d, 31, 3)
    with torch.no_grad():
        got = model.eye_net.forward_sequence(cam)
        want = model.eye_net.forward_sequence(pat)
        plain = model.eye_net.forward_sequence({k_: v for k_, v in cam.items() if k_ != 'camera_lens'})
    assert set(got) == set(want) and tuple(got['left_g_initial'].shape) == (2, 3, 2)
    for key in want:
        for a, b in zip(tensors(got[key]), tensors(want[key])):
            assert torch.isfinite(a).all() and torch.equal(a, b), key
    assert not torch.equal(got['left_g_initial'], plain['left_g_initial'])
    with pytest.raises(TypeError, match='camera_lens'):
        model.eye_net.forward_sequence(dict(cam, camera_lens=cam['camera_lens'].double()))
    with pytest.raises(ValueError, match='camera_lens'):
        model.eye_net.forward_sequence(dict(pat, camera_lens=cam['camera_lens']))


def test_eve_eval_takes_raw_frames_and_a_lens():
    model, _ = make_model()
    _, _, full = gpu_clip(2, 3, seed=5)
    cam, pat = both_forms(full, 31, 3)
    with torch.no_grad():
        got, want = model(cam), model(pat)
    assert set(got) == set(want) and 'PoG_px_final' in got
    for key in want:
        if torch.is_tensor(want[key]):
            assert torch.equal(got[key], want[key]), key


def test_stream_replays_a_graph_over_raw_frames_and_lenses():
    """B = 2, Tc = 2, refine_net config.  Three steps, the third ragged: the graph's outputs are the eager step's bit for bit, and two
    graphs are captured; the second step replays the first one's graph with other frames, other warps and ANOTHER LENS, and gives
    that lens's result, not the first lens's (the graph reads its input buffers).  The chunks equal the float-patch form's chunks
    bit for bit.  A chunk without camera_lens captures a graph of its own and gives the plain warp's result."""
    model, _ = make_model()
    _, d, _ = gpu_clip(2, 6, seed=5)
    cam, pat = both_forms(d, 33, 6)
    ch = lambda src, i: {k_: v[:, 2 * i:2 * i + 2].contiguous() for k_, v in src.items()}
    assert not torch.equal(ch(cam, 0)['camera_lens'], ch(cam, 1)['camera_lens'])
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
    other = e2.step(dict(ch(cam, 1), camera_lens=ch(cam, 0)['camera_lens']))    # the second chunk under the first chunk's lens
    assert not torch.equal(other['g_initial'], outs[1]['g_initial'])
    # uniform chunks of the whole clip: the same graph stream from zero state, the float-patch form beside it
    g.reset()
    p = eve_amd.EVEStream(model, 2)
    whole_cam, whole_pat = [], []
    for i in range(3):
        whole_cam.append({k_: v.clone() for k_, v in g.step(ch(cam, i)).items()})
        whole_pat.append({k_: v.clone() for k_, v in p.step(ch(pat, i)).items()})
    assert len(g._graphs) == 3                                       # (without heat-maps: one more key)
    for a, b in zip(whole_cam, whole_pat):
        for k_ in a:
            assert torch.equal(a[k_], b[k_]), k_
    # without the key: a graph of its own, and the plain warp's patches
    g.reset()
    no_lens = {k_: v for k_, v in ch(cam, 0).items() if k_ != 'camera_lens'}
    plain = {k_: v.clone() for k_, v in g.step(no_lens).items()}
    assert len(g._graphs) == 4
    e3 = eve_amd.EVEStream(model, 2, use_graph=False)
    plain_eager = e3.step(no_lens)
    for k_ in plain:
        assert torch.equal(plain[k_], plain_eager[k_]), k_
    assert not torch.equal(plain['g_initial'], whole_cam[0]['g_initial'])
