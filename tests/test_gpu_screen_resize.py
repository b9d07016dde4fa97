"""GPU: eve_screen_u8_area_to_nchw (csrc/screen_resize.hip) bit for bit against its contract in numpy (tests/screen_resize_ref.py),
and the full-resolution uint8 screen through RefineNet.forward_sequence and EVEStream, eager and under graph replay."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import eve_amd
from eve_amd.kernels import default_kernels
import screen_resize_ref as ref
from test_gpu_stream import gpu_clip, make_model

pytestmark = pytest.mark.gpu
SCREEN = (72, 128)
GUARD = 1024                  # floats behind the output that no launch may touch
SENTINEL = -7.0

# (N, IH, IW, C, OH, OW, the kernel that takes it): <true> reads 16-byte vectors, <false> single bytes (a row pitch that is no
# multiple of 16).  The grid is capped at 4 096 (frame, output row) items; the N = 60 cases go round the grid-stride loop.
CASES = [
    (2, 1080, 1920, 3, 72, 128, True),         # the workload's ratio, 15 x 15
    (1, 144, 256, 3, 72, 128, True),           # ratio 2, the smallest integer ratio
    (5, 144, 256, 3, 72, 128, True),
    (1, 73, 129, 3, 72, 128, False),           # barely above 1: every output straddles two sources with extreme weights
    (5, 73, 129, 3, 72, 128, False),
    (2, 100, 171, 3, 72, 128, False),          # fractional, pitch 513
    (1, 768, 1366, 3, 72, 128, False),         # a laptop panel, fractional both ways, pitch 4 098
    (2, 90, 160, 4, 72, 128, True),            # BGRA
    (3, 100, 171, 4, 72, 128, False),          # BGRA with a pitch of 684 = 16 * 42 + 12
    (1, 1080, 1920, 3, 36, 64, True),          # targets other than the default
    (3, 45, 77, 3, 5, 7, False),
    (2, 72, 128, 3, 72, 128, True),            # already at the target size
    (60, 144, 256, 3, 72, 128, True),          # 4 320 items > the grid
    (60, 73, 129, 3, 72, 128, False),
]
IDS = ['%dx%dx%dx%d-%dx%d' % c[:6] for c in CASES]


def random_frames(N, IH, IW, C, seed):
    v = np.random.default_rng(seed).integers(0, 256, size=(N, IH, IW, C), dtype=np.uint8)
    if C == 4:
        v[..., 3] = 255                        # the alpha plane: must leave no trace
    return v


def alternating_frames(N, IH, IW, C):
    """Rows and columns alternate 0 / 255 (frame n starts at phase n): a weight off by one source pixel changes every output."""
    y = np.arange(IH)[None, :, None, None]
    x = np.arange(IW)[None, None, :, None]
    n = np.arange(N)[:, None, None, None]
    v = (((y + n) % 2 == 0) & ((x + n // 2) % 2 == 0)).astype(np.uint8) * 255
    v = np.broadcast_to(v, (N, IH, IW, C)).copy()
    if C == 4:
        v[..., 3] = 255
    return v


def raw_call(k, frames, out_hw, out_flat):
    N, IH, IW, C = frames.shape
    return k.lib.eve_screen_u8_area_to_nchw(N, IH, IW, C, ctypes.c_void_p(frames.data_ptr()), out_hw[0], out_hw[1],
                                            ctypes.c_void_p(out_flat.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def check(k, v, out_hw, vec):
    """Two launches into a guarded buffer, each == the numpy contract with no tolerance; the guard untouched; the kernel's name."""
    N = v.shape[0]
    want = torch.from_numpy(ref.area_resize(v, out_hw))
    n_out = want.numel()
    frames = torch.from_numpy(v).cuda()
    for _ in range(2):
        out = torch.full((n_out + GUARD,), SENTINEL, dtype=torch.float32, device='cuda')
        assert raw_call(k, frames, out_hw, out) == 0, k.lib.eve_last_error()
        assert k.lib.eve_last_kernel() == (b'screen_u8_area_kernel<true>' if vec else b'screen_u8_area_kernel<false>')
        got = out.cpu()
        assert torch.equal(got[n_out:], torch.full((GUARD,), SENTINEL)), 'guard overwritten'
        got = got[:n_out].view(N, 3, out_hw[0], out_hw[1])
        bad = (got.view(torch.int32) != want.view(torch.int32))
        assert not bad.any(), ('%d of %d outputs differ, first at %s: got %r want %r' % (
            int(bad.sum()), n_out, tuple(bad.nonzero()[0].tolist()), float(got[bad][0]), float(want[bad][0])))
    return frames, want


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_kernel_equals_the_contract(case):
    N, IH, IW, C, OH, OW, vec = case
    k = default_kernels()
    frames, want = check(k, random_frames(N, IH, IW, C, seed=IH + IW + N), (OH, OW), vec)
    check(k, alternating_frames(N, IH, IW, C), (OH, OW), vec)
    via = k.screen_u8_area_to_nchw(frames, (OH, OW))                  # the tensor-level wrapper
    assert via.dtype == torch.float32 and tuple(via.shape) == (N, 3, OH, OW) and torch.equal(via.cpu(), want)
    if (IH, IW, C) == (OH, OW, 3):                                    # the same bits as the plain normalisation
        assert torch.equal(via, k.frames_u8_to_nchw(frames, 1.0 / 255.0, None))


def test_largest_sum_fits():
    """One 2160 x 3840 frame of all 255: S = 255 * 8 294 400 = 2 115 072 000 per output needs 31 bits, the column sums 20; a
    signed or 24-bit accumulator shows here.  Every output is exactly 1.0."""
    k = default_kernels()
    v = np.full((1, 2160, 3840, 3), 255, dtype=np.uint8)
    _, want = check(k, v, SCREEN, True)
    assert (want == 1.0).all()


def test_unaligned_base_takes_the_byte_path():
    """A frame pitch that is a multiple of 16 behind a base that is not 16-byte aligned must not be read as vectors."""
    k = default_kernels()
    v = random_frames(2, 90, 160, 3, seed=3)
    want = torch.from_numpy(ref.area_resize(v, SCREEN))
    buf = torch.zeros((v.size + 16,), dtype=torch.uint8, device='cuda')
    frames = buf[4:4 + v.size].view(v.shape)
    frames.copy_(torch.from_numpy(v))
    assert frames.data_ptr() % 16 == 4 and frames.is_contiguous()
    got = k.screen_u8_area_to_nchw(frames, SCREEN)
    assert k.lib.eve_last_kernel() == b'screen_u8_area_kernel<false>'
    assert torch.equal(got.cpu(), want)


def test_refused_requests_launch_nothing():
    k = default_kernels()
    frames = torch.zeros((1, 90, 160, 3), dtype=torch.uint8, device='cuda')
    k.frames_u8_to_nchw(frames, 1.0 / 255.0, None)
    k.stream_state_rows(torch.zeros((2, 8), device='cuda'), torch.zeros((2, 8), device='cuda'))     # the last named launch
    before = k.lib.eve_last_kernel()
    assert b'screen_u8_area' not in before
    out = torch.full((3 * 72 * 128 + GUARD,), SENTINEL, dtype=torch.float32, device='cuda')
    p, s = ctypes.c_void_p(frames.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    o = ctypes.c_void_p(out.data_ptr())
    call = lambda N, IH, IW, C, OH, OW, a=p, b=o: k.lib.eve_screen_u8_area_to_nchw(N, IH, IW, C, a, OH, OW, b, s)
    cases = {'rows upscaled': ((1, 60, 160, 3, 72, 128), 'upscaling'), 'columns upscaled': ((1, 90, 100, 3, 72, 128), 'upscaling'),
             'oversize': ((1, 4105, 4104, 3, 72, 128), 'too large'), 'two channels': ((1, 90, 160, 2, 72, 128), 'C must be'),
             'no frames': ((0, 90, 160, 3, 72, 128), 'bad arguments'), 'row too wide': ((1, 72, 13654, 3, 72, 128), 'too wide')}
    for name, (args, word) in cases.items():
        assert call(*args) != 0, name
        msg = k.lib.eve_last_error().decode()
        assert msg.startswith('screen_u8_area_to_nchw:') and word in msg, (name, msg)
        assert k.lib.eve_last_kernel() == before, name
    assert call(1, 90, 160, 3, 72, 128, None, o) != 0 and call(1, 90, 160, 3, 72, 128, p, None) != 0
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.full((out.numel(),), SENTINEL))
    with pytest.raises(RuntimeError, match='upscaling'):
        k.screen_u8_area_to_nchw(frames, (91, 128))
    assert call(1, 90, 160, 3, 72, 128) == 0                          # the same call with sound arguments is taken
    assert (out[:3 * 72 * 128] == 0).all() and (out[3 * 72 * 128:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ RefineNet / EVEStream
@functools.lru_cache(maxsize=None)
def capture(seed, B=2, T=3):
    """A 1080p capture: uint8 [B, T, 1080, 1920, 3] on the CPU."""
    return torch.from_numpy(random_frames(B * T, 1080, 1920, 3, seed=seed)).view(B, T, 1080, 1920, 3)


@functools.lru_cache(maxsize=None)
def capture_resized(seed):
    """The float [B, T, 3, 72, 128] the contract gives for capture(seed)."""
    v = capture(seed)
    return torch.from_numpy(ref.area_resize(v.numpy().reshape((-1,) + tuple(v.shape[2:])), SCREEN)).view(tuple(v.shape[:2]) + (3,) + SCREEN)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_refinenet_takes_the_full_resolution_screen(dtype):
    model, _ = make_model(dtype=dtype)
    cap, pre = capture(21), capture_resized(21)
    heat = torch.rand((2, 3, 1) + SCREEN, generator=torch.Generator().manual_seed(2)).cuda()
    with torch.no_grad():
        got, gst = model.refine_net.forward_sequence(heat, cap.cuda())
        want, wst = model.refine_net.forward_sequence(heat, pre.cuda())
    assert tuple(got.shape) == (2, 3, 1) + SCREEN and torch.isfinite(got).all()
    assert torch.equal(got, want)
    flat = lambda sts: [t for s_ in sts for t in (s_ if isinstance(s_, tuple) else (s_,))]
    for a, b in zip(flat(gst), flat(wst)):
        assert torch.equal(a, b)


def test_stream_replays_a_graph_over_the_capture():
    """B = 2, Tc = 2.  The graph's outputs are the eager step's, bit for bit; a replay with another screen gives that screen's
    result (the graph reads its input buffer, not a pointer baked in at capture); one ragged step goes the same way."""
    model, _ = make_model()
    _, d, _ = gpu_clip(2, 6, seed=5)
    screens = [capture(21)[:, :2].cuda(), capture(22)[:, :2].cuda(), capture(22)[:, 1:3].cuda()]
    ch = lambda i: dict({k_: v[:, 2 * i:2 * i + 2].contiguous() for k_, v in d.items()}, screen_frame=screens[i])
    g, e = eve_amd.EVEStream(model, 2), eve_amd.EVEStream(model, 2, use_graph=False)
    outs = []
    for i, lengths in enumerate((None, None, [1, 2])):
        og = {k_: v.clone() for k_, v in g.step(ch(i), return_heatmaps=True, lengths=lengths).items()}
        oe = e.step(ch(i), return_heatmaps=True, lengths=lengths)
        assert set(og) == set(oe) and 'heatmap_final' in og
        for k_ in og:
            assert torch.equal(og[k_], oe[k_]), (i, k_)
        outs.append(og)
    assert len(g._graphs) == 2                                       # one uniform graph replayed twice, one ragged
    # the second replay saw the second screen: the same chunk with the FIRST screen gives another heat-map
    e2 = eve_amd.EVEStream(model, 2, use_graph=False)
    e2.step(ch(0), return_heatmaps=True)
    other = e2.step(dict(ch(1), screen_frame=screens[0]), return_heatmaps=True)
    assert not torch.equal(other['heatmap_final'], outs[1]['heatmap_final'])
