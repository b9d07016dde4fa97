"""CPU: full-resolution uint8 screen captures -- the contract of eve_screen_u8_area_to_nchw (tests/screen_resize_ref.py) against its
two restatements, and the host path from data.preprocess_screen_frames(size=...) through RefineNet, EVE and EVEStream on the
torch-CPU stand-in kernels.  tests/test_gpu_screen_resize.py checks the HIP kernel and the graph mode."""
import numpy as np
import pytest
import torch

import eve_amd
from eve_amd import data, kernels
import screen_resize_ref as ref
from test_stream_host import chunk_of, clip
from test_stream_ragged_host import CONFIGS, LoggingFakes, RaggedFakes, make_model

SCREEN = (72, 128)            # configs/refine_net.json screen_size, as (H, W)


class ScreenFakes(RaggedFakes):
    screen_u8_area_to_nchw = ref.screen_u8_area_to_nchw


class LoggingScreenFakes(LoggingFakes):
    screen_u8_area_to_nchw = ref.screen_u8_area_to_nchw


@pytest.fixture()
def fake():
    k = ScreenFakes()
    kernels.set_default_kernels(k)
    yield k
    kernels.set_default_kernels(None)
    eve_amd.reset_standalone_config()


def frames_u8(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the contract
# (IH, IW, C) -> (OH, OW): fractional both ways, coprime, integer ratios (3 x 2 and 2 x 2), the same size, barely larger, four
# channels
SMALL = [((24, 40, 3), (9, 16)), ((13, 17, 3), (5, 7)), ((18, 32, 3), (9, 16)), ((10, 14, 3), (5, 7)), ((9, 16, 3), (9, 16)),
         ((10, 17, 3), (9, 16)), ((24, 40, 4), (9, 16)), ((10, 14, 4), (5, 7))]


@pytest.mark.parametrize('shape,out_hw', SMALL, ids=['%dx%dx%d-%dx%d' % (s + o) for s, o in SMALL])
def test_restatements_agree_bit_for_bit(shape, out_hw):
    v = frames_u8((3,) + shape, seed=sum(shape))
    v[2, ::2, 1::2] = 255                     # one frame whose rows and columns alternate 0 / 255
    v[2, 1::2, :] = 0
    v[2, ::2, ::2] = 0
    S = ref.area_sums(v, out_hw)
    assert S.dtype == np.int64 and S.shape == (3, 3) + out_hw
    assert np.array_equal(S, ref.area_sums_by_replication(v, out_hw))
    assert S.max() <= 255 * shape[0] * shape[1]
    got = ref.area_resize(v, out_hw)
    assert got.dtype == np.float32 and got.min() >= 0.0 and got.max() <= 1.0
    if shape[0] % out_hw[0] == 0 and shape[1] % out_hw[1] == 0:
        assert np.array_equal(bits(got), bits(ref.area_resize_avg_pool(v, out_hw)))
    if shape[:2] == out_hw:                   # already at the target size: the values of frames_u8_to_nchw
        want = v[..., :3].transpose(0, 3, 1, 2).astype(np.float32) * np.float32(1.0 / 255.0)
        assert np.array_equal(bits(got), bits(want))
    if shape[2] == 4:                         # the fourth channel leaves no trace
        w = v.copy()
        w[..., 3] = 255 - w[..., 3]
        assert np.array_equal(bits(got), bits(ref.area_resize(w, out_hw)))


@pytest.mark.parametrize('shape,out_hw', [((13, 17, 3), (5, 7)), ((24, 40, 3), (9, 16)), ((18, 32, 4), (9, 16))])
def test_a_constant_frame_keeps_its_value_exactly(shape, out_hw):
    v = np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None, None, None], (256,) + shape)
    got = ref.area_resize(v, out_hw)
    want = np.arange(256, dtype=np.float32) * np.float32(1.0 / 255.0)
    assert np.array_equal(bits(got), bits(np.broadcast_to(want[:, None, None, None], got.shape)))


@pytest.mark.parametrize('I,O', [(24, 9), (40, 16), (13, 5), (17, 7), (1080, 72), (1920, 128), (768, 72), (1366, 128), (73, 72), (9, 9)])
def test_weights_of_every_output_sum_to_the_source_extent(I, O):
    w = ref.axis_weights(I, O)
    assert w.shape == (O, I) and w.min() >= 0
    assert (w.sum(axis=1) == I).all()         # an output pixel's footprint is I units of 1/O source pixels
    assert (w.sum(axis=0) == O).all()         # and every source pixel is handed out whole
    for o in range(O):                        # the support is the rows the kernel walks, and no more than ceil(I / O) + 1 of them
        nz = np.nonzero(w[o])[0]
        assert nz[0] == o * I // O and nz[-1] + 1 == ((o + 1) * I + O - 1) // O
        assert len(nz) <= -(-I // O) + 1


def test_upscaling_and_oversize_frames_raise(fake):
    small = torch.zeros((1, 2, 60, 128, 3), dtype=torch.uint8)
    with pytest.raises((ValueError, RuntimeError)):
        data.preprocess_screen_frames(small, size=SCREEN)                  # 60 rows -> 72
    with pytest.raises((ValueError, RuntimeError)):
        data.preprocess_screen_frames(torch.zeros((1, 80, 100, 3), dtype=torch.uint8), size=SCREEN)     # 100 columns -> 128
    huge = torch.zeros((1, 1, 1, 3), dtype=torch.uint8).expand(1, 4105, 4104, 3)         # 16 846 920 pixels, no memory behind them
    with pytest.raises((ValueError, RuntimeError)):
        fake.screen_u8_area_to_nchw(huge, SCREEN)
    ok = torch.zeros((1, 1, 1, 3), dtype=torch.uint8).expand(1, 4103, 4105, 3)           # 16 842 815: inside the limit
    ref.check_shapes(tuple(ok.shape), SCREEN)
    with pytest.raises(TypeError):
        data.preprocess_screen_frames(torch.zeros((1, 144, 256, 3)), size=SCREEN)        # float frames are not resized


# ------------------------------------------------------------------------------------------------ data.py / RefineNet
def test_preprocess_screen_frames_routes_by_size():
    k = LoggingScreenFakes()
    kernels.set_default_kernels(k)
    try:
        same = torch.from_numpy(frames_u8((2, 3) + SCREEN + (3,), 1))
        a = data.preprocess_screen_frames(same)
        b = data.preprocess_screen_frames(same, size=SCREEN)
        assert [c[0] for c in k.log] == ['frames_u8_to_nchw', 'frames_u8_to_nchw'] and torch.equal(a, b)
        del k.log[:]
        full = torch.from_numpy(frames_u8((2, 3, 100, 171, 4), 2))
        c = data.preprocess_screen_frames(full, size=SCREEN)
        assert [c_[0] for c_ in k.log] == ['screen_u8_area_to_nchw']
        assert tuple(c.shape) == (2, 3, 3) + SCREEN and c.dtype == torch.float32
        assert np.array_equal(bits(c.numpy().reshape((6, 3) + SCREEN)), bits(ref.area_resize(full.numpy().reshape(6, 100, 171, 4), SCREEN)))
    finally:
        kernels.set_default_kernels(None)


@pytest.mark.parametrize('shape', [(144, 256, 3), (100, 171, 4)], ids=['144x256x3', '100x171x4'])
def test_refinenet_takes_a_full_resolution_uint8_screen(fake, shape):
    """forward_sequence on the capture equals, bit for bit, forward_sequence on the float tensor the contract gives for it."""
    model = make_model(*CONFIGS['gru-cgru'])
    B, T = 1, 2
    g = torch.Generator().manual_seed(5)
    heat = torch.rand((B, T, 1) + SCREEN, generator=g)
    cap = torch.from_numpy(frames_u8((B, T) + shape, 7))
    want_screen = torch.from_numpy(ref.area_resize(cap.numpy().reshape((B * T,) + shape), SCREEN)).view((B, T, 3) + SCREEN)
    with torch.no_grad():
        got, gst = model.refine_net.forward_sequence(heat, cap)
        want, wst = model.refine_net.forward_sequence(heat, want_screen)
    assert tuple(got.shape) == (B, T, 1) + SCREEN
    assert torch.equal(got, want)
    for a, b in zip(gst, wst):
        assert torch.equal(a, b)


def test_a_same_size_uint8_screen_issues_the_calls_it_always_did():
    k = LoggingScreenFakes()
    kernels.set_default_kernels(k)
    try:
        model = make_model(*CONFIGS['gru-cgru'])
        batch = clip(2, 2, seed=3)
        ch = chunk_of(batch, 0, 2)
        ch['screen_frame'] = (ch['screen_frame'] * 255).round().to(torch.uint8).permute(0, 1, 3, 4, 2).contiguous()
        eve_amd.EVEStream(model, 2, use_graph=False).step(ch)
        names = [c[0] for c in k.log]
        assert 'screen_u8_area_to_nchw' not in names
        assert [c for c in k.log if c[0] == 'frames_u8_to_nchw'] == [['frames_u8_to_nchw', [[[4] + list(SCREEN) + [3], 'torch.uint8']]]]
    finally:
        kernels.set_default_kernels(None)
        eve_amd.reset_standalone_config()


def test_eve_forward_takes_the_capture(fake):
    """EVE.forward (the path Trainer takes too), eval: the capture in place of the float screen it resizes to."""
    model = make_model(*CONFIGS['gru-cgru'])
    batch = clip(1, 2, seed=3)
    cap = torch.from_numpy(frames_u8((1, 2, 100, 171, 3), 9))
    pre = torch.from_numpy(ref.area_resize(cap.numpy().reshape(2, 100, 171, 3), SCREEN)).view((1, 2, 3) + SCREEN)
    with torch.no_grad():
        got = model(dict(batch, screen_frame=cap))
        want = model(dict(batch, screen_frame=pre))
    for key in ('PoG_px_final', 'g_final', 'PoG_px_initial'):
        assert torch.equal(got[key], want[key]), key


# ------------------------------------------------------------------------------------------------ EVEStream
@pytest.mark.parametrize('lengths', [None, [2, 0], [1, 2]], ids=['uniform', 'ragged-idle', 'ragged'])
def test_stream_step_takes_the_capture(fake, lengths):
    model = make_model(*CONFIGS['gru-cgru'])
    batch = clip(2, 2, seed=3)
    ch = chunk_of(batch, 0, 2)
    cap = torch.from_numpy(frames_u8((2, 2, 100, 171, 4), 11))
    pre = torch.from_numpy(ref.area_resize(cap.numpy().reshape(4, 100, 171, 4), SCREEN)).view((2, 2, 3) + SCREEN)
    a, b = eve_amd.EVEStream(model, 2, use_graph=False), eve_amd.EVEStream(model, 2, use_graph=False)
    fake.calls.clear()
    got = a.step(dict(ch, screen_frame=cap), return_heatmaps=True, lengths=lengths)
    want = b.step(dict(ch, screen_frame=pre), return_heatmaps=True, lengths=lengths)
    assert set(got) == set(want) and 'heatmap_final' in got and ('valid' in got) == (lengths is not None)
    for key in want:
        assert torch.equal(got[key], want[key]), key
    sa, sb = a.get_state(), b.get_state()
    for key in sb:
        for x, y in zip(sa[key] if isinstance(sa[key], tuple) else (sa[key],), sb[key] if isinstance(sb[key], tuple) else (sb[key],)):
            assert torch.equal(x, y), key
