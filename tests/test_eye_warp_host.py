"""CPU: eye patches cut from whole uint8 camera frames -- the contract of eve_eye_warp_u8_to_nchw / _to_stem (tests/eye_warp_ref.py)
against the plain normalisation, a hand-computed case and its outside rules, and the host path from data.warp_eye_patches through
EyeNet, EVE and EVEStream on the torch-CPU stand-in kernels.  tests/test_gpu_eye_warp.py checks the HIP kernels and the graph mode."""
import math

import numpy as np
import pytest
import torch

import eve_amd
from eve_amd import data, kernels
from eve_amd.eye_net import eye_input
import eye_warp_ref as ref
from test_stream_host import chunk_of, clip
from test_stream_ragged_host import CONFIGS, LoggingFakes, RaggedFakes, make_model

SIZE = 64                     # the patch the CPU trunk is run on (configs: eyes_size = [64, 64])
FRAME = (96, 120)             # the camera frames of the host-path tests, (IH, IW)
SMALL_EYES = dict(eyes_size=[SIZE, SIZE])


class WarpFakes(RaggedFakes):
    eye_warp_u8_to_nchw = ref.eye_warp_u8_to_nchw
    eye_warp_u8_to_stem = ref.eye_warp_u8_to_stem


class LoggingWarpFakes(LoggingFakes):
    eye_warp_u8_to_nchw = ref.eye_warp_u8_to_nchw
    eye_warp_u8_to_stem = ref.eye_warp_u8_to_stem


@pytest.fixture()
def fake():
    k = WarpFakes()
    kernels.set_default_kernels(k)
    yield k
    kernels.set_default_kernels(None)
    eve_amd.reset_standalone_config()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def preprocess_crop(frames, x, y, hw):
    """The numpy expressions of preprocess_frames (datasources/eve_sequences.py:196-203) on frames[:, y:y+H, x:x+W, :3]."""
    crop = frames[:, y:y + hw[0], x:x + hw[1], :3].astype(np.float32)
    crop *= np.float32(2.0 / 255.0)
    crop -= np.float32(1.0)
    return np.transpose(crop, (0, 3, 1, 2))


# ------------------------------------------------------------------------------------------------ the contract
@pytest.mark.parametrize('C', [3, 4])
@pytest.mark.parametrize('tx,ty,hw', [(37, 21, (128, 128)), (0, 0, (160, 200)), (72, 124, (36, 60)), (1, 0, (5, 7))])
def test_an_integer_translation_is_preprocess_frames_on_the_crop(tx, ty, hw, C):
    v = ref.random_frames(2, 160, 200, C, seed=tx + ty + C)
    got, outside = ref.eye_warp(v, np.stack([ref.shift(tx, ty)] * 2), hw)
    assert got.dtype == np.float32 and got.shape == (2, 3) + hw and not outside.any()
    assert np.array_equal(bits(got), bits(preprocess_crop(v, tx, ty, hw)))
    if C == 4:                                # the fourth channel leaves no trace
        w = v.copy()
        w[..., 3] = 7
        assert np.array_equal(bits(got), bits(ref.eye_warp(w, np.stack([ref.shift(tx, ty)] * 2), hw)[0]))


def test_a_hand_computed_frame_pins_the_weights():
    """Frame [[10, 20], [30, 40]] (channel c adds c).  v = 0.5 throughout: ay = 128, y0 = 0.
      u = -0.5: x0 = -1, ax = 128   S = 128*128 * (0 + 10 + 0 + 30)   = 16384 * 40       the column before the frame reads 0
      u =  0.5: x0 =  0, ax = 128   S = 16384 * (10 + 20 + 30 + 40)   = 16384 * 100
      u =  1.5: x0 =  1, ax = 128   S = 16384 * (20 + 0 + 40 + 0)     = 16384 * 60       the column behind it too
    and one pixel at (u, v) = (0.25, 0.5): ax = 64: S = 192*128*10 + 64*128*20 + 192*128*30 + 64*128*40 = 1 474 560 = 22.5 * 65536."""
    f = np.array([[10, 20], [30, 40]], dtype=np.uint8)[None, :, :, None] + np.arange(3, dtype=np.uint8)
    S, outside = ref.warp_sums(f, ref.shift(-0.5, 0.5)[None], (1, 3))
    assert not outside.any()
    assert S[0, 0, 0].tolist() == [16384 * 40, 16384 * 100, 16384 * 60]
    assert S[0, 1, 0].tolist() == [16384 * 42, 16384 * 104, 16384 * 62]          # channel 1: every tap inside the frame one higher
    S, _ = ref.warp_sums(f, ref.shift(0.25, 0.5)[None], (1, 1))
    assert S[0, :, 0, 0].tolist() == [1474560, 1474560 + 65536, 1474560 + 2 * 65536]
    got = ref.values_of_sums(S)
    want = np.array([22.5, 23.5, 24.5], dtype=np.float32) * np.float32(2.0 / 255.0) + np.float32(-1.0)
    assert np.array_equal(bits(got[0, :, 0, 0]), bits(want))
    # the rounding of the coordinate: 0.5 / 256 is a tie and goes up (floor(x + 0.5)), just below it goes down
    S, _ = ref.warp_sums(f, ref.shift(0.5 / 256, 0)[None], (1, 1))
    assert S[0, 0, 0, 0] == 255 * 256 * 10 + 1 * 256 * 20
    S, _ = ref.warp_sums(f, ref.shift(0.49 / 256, 0)[None], (1, 1))
    assert S[0, 0, 0, 0] == 65536 * 10


def test_outside_pixels_are_minus_one():
    v = ref.random_frames(1, 160, 200, 3, seed=5)
    hw = (128, 128)
    for name, (m, kind) in ref.WARPS.items():
        got, outside = ref.eye_warp(v, m[None], hw)
        assert ref.outside_share_ok(kind, outside.mean()), (name, outside.mean())
        assert (got[0][:, outside[0]] == -1.0).all(), name
        assert got.min() >= -1.0 and got.max() <= 1.0
    # Wd = 1 - 0.02 * ox is <= 0 from column 51 on (float32(-0.02) is a little above -0.02, so column 50 keeps a tiny positive
    # Wd and leaves through u < IW instead)
    got, outside = ref.eye_warp(v, ref.WARPS['negative-denominator'][0][None], hw)
    assert outside[0, :, 50:].all() and not outside[0, 0, :36].any()
    for m in (ref.NAN_WARP, ref.OFF_FRAME_WARP):
        got, outside = ref.eye_warp(v, m[None], hw)
        assert outside.all() and (got == -1.0).all()
    # a NaN in one row of the matrix only: X stays finite, v is NaN, every comparison with it is false
    assert np.isnan(ref.NAN_WARP[1]).any() and not np.isnan(ref.NAN_WARP[[0, 2]]).any()


def scalar_pixel(frame, m, oy, ox):
    """The contract for one pixel in plain Python floats and ints: -> (S per channel, outside)."""
    IH, IW = frame.shape[:2]
    m = [[float(x) for x in row] for row in m]
    X = (m[0][0] * ox + m[0][1] * oy) + m[0][2]
    Y = (m[1][0] * ox + m[1][1] * oy) + m[1][2]
    Wd = (m[2][0] * ox + m[2][1] * oy) + m[2][2]
    if not Wd > 0:                               # (also a NaN; Python would raise on a division by zero)
        return [0, 0, 0], True
    u, v = X / Wd, Y / Wd
    if not (u > -1 and u < IW and v > -1 and v < IH):
        return [0, 0, 0], True
    fu, fv = math.floor(u * 256 + 0.5), math.floor(v * 256 + 0.5)
    x0, ax, y0, ay = fu >> 8, fu & 255, fv >> 8, fv & 255
    tap = lambda y, x, c: int(frame[y, x, c]) if 0 <= y < IH and 0 <= x < IW else 0
    return [(256 - ax) * (256 - ay) * tap(y0, x0, c) + ax * (256 - ay) * tap(y0, x0 + 1, c) + (256 - ax) * ay * tap(y0 + 1, x0, c) +
            ax * ay * tap(y0 + 1, x0 + 1, c) for c in range(3)], False


def test_the_vectorised_contract_equals_a_pixel_by_pixel_restatement():
    v = ref.random_frames(1, 160, 200, 3, seed=6)
    g = np.random.default_rng(0)
    for name, m in [(n_, w[0]) for n_, w in ref.WARPS.items()] + [('nan', ref.NAN_WARP), ('off-frame', ref.OFF_FRAME_WARP)]:
        S, outside = ref.warp_sums(v, m[None], (128, 128))
        edge = [(0, 0), (0, 127), (127, 0), (127, 127)]
        for oy, ox in edge + [tuple(p) for p in g.integers(0, 128, size=(300, 2))]:
            s, out = scalar_pixel(v[0], m, int(oy), int(ox))
            assert out == bool(outside[0, oy, ox]) and s == S[0, :, oy, ox].tolist(), (name, oy, ox)


def test_the_far_edge_needs_two_columns_of_padding():
    """u just below IW rounds to fu = 256 * IW: x0 = IW, ax = 0, and the taps at x0 and x0 + 1 = IW + 1 both read 0 -- the pixel is
    inside by the test and -1 by its taps."""
    v = np.full((1, 4, 6, 3), 255, dtype=np.uint8)
    got, outside = ref.eye_warp(v, ref.shift(6 - 2.0 ** -10, 4 - 2.0 ** -10)[None], (1, 1))
    assert not outside.any() and (got == -1.0).all()
    got, outside = ref.eye_warp(v, ref.shift(-1 + 2.0 ** -10, 0)[None], (1, 1))        # u*256 + 0.5 = -255.25: x0 = -1, ax = 0
    assert not outside.any() and (got == -1.0).all()
    got, outside = ref.eye_warp(v, ref.shift(-1, 0)[None], (1, 1))                      # u > -1 is strict
    assert outside.all()
    got, outside = ref.eye_warp(v, ref.shift(6, 0)[None], (1, 1))                       # and so is u < IW
    assert outside.all()


def test_oversize_and_malformed_requests_raise():
    f = np.zeros((1, 8, 8, 3), dtype=np.uint8)
    ident = ref.shift(0, 0)[None]
    for frames_shape, hw in (((1, 8, 8, 2), (4, 4)), ((1, 16385, 8, 3), (4, 4)), ((1, 8, 16385, 3), (4, 4)), ((1, 8, 8, 3), (4097, 4)),
                             ((1, 8, 8, 3), (4, 4097)), ((1, 8, 8, 3), (0, 4))):
        with pytest.raises(ValueError):
            ref.check_shapes(frames_shape, (1, 3, 3), hw)
    with pytest.raises(ValueError):
        ref.eye_warp(f, np.stack([ident[0]] * 2), (4, 4))
    ref.check_shapes((1, 16384, 16384, 4), (1, 3, 3), (4096, 4096))


# ------------------------------------------------------------------------------------------------ data.warp_eye_patches
def camera(B, T, seed, C=3):
    return torch.from_numpy(ref.random_frames(B * T, FRAME[0], FRAME[1], C, seed)).view(B, T, FRAME[0], FRAME[1], C)


def warps_for(B, T, seed, integer=False):
    """Per (stream, frame, eye) another warp that keeps a SIZE patch mostly inside a FRAME frame -> (left, right) [B, T, 3, 3]."""
    g = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        ms = []
        for _ in range(B * T):
            if integer:
                ms.append(ref.shift(int(g.integers(0, FRAME[1] - SIZE + 1)), int(g.integers(0, FRAME[0] - SIZE + 1))))
            else:
                ms.append(ref.similarity(float(g.uniform(0.8, 1.2)), float(g.uniform(-15, 15)), float(g.uniform(5, 40)), float(g.uniform(0, 20)),
                                         persp=(float(g.uniform(-2e-4, 2e-4)), float(g.uniform(-2e-4, 2e-4)))))
        out.append(torch.from_numpy(np.stack(ms)).view(B, T, 3, 3))
    return out


def contract_patches(frames, warps, hw):
    B, T = frames.shape[:2]
    v, _ = ref.eye_warp(frames.numpy().reshape((B * T,) + tuple(frames.shape[2:])), warps.numpy().reshape(B * T, 3, 3), hw)
    return torch.from_numpy(v).view((B, T, 3) + hw)


def test_warp_eye_patches_folds_leading_dimensions_and_reads_the_config(fake):
    frames, (lw, _) = camera(2, 3, seed=1, C=4), warps_for(2, 3, seed=2)
    got = data.warp_eye_patches(frames, lw, size=(36, 60))
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 3, 3, 36, 60)
    assert torch.equal(got, contract_patches(frames, lw, (36, 60)))
    assert torch.equal(data.warp_eye_patches(frames[1], lw[1], size=(36, 60)), got[1])                      # one leading dimension
    assert tuple(data.warp_eye_patches(frames, lw).shape) == (2, 3, 3, 128, 128)                           # eyes_size's default
    eve_amd.get_config().import_dict(dict(eyes_size=[60, 36]))                                             # (W, H), as screen_size
    assert data.eye_patch_hw() == (36, 60)
    assert torch.equal(data.warp_eye_patches(frames, lw), got)
    with pytest.raises(TypeError):
        data.warp_eye_patches(frames.float(), lw)
    with pytest.raises(TypeError):
        data.warp_eye_patches(frames, lw.double())
    with pytest.raises(TypeError):
        data.warp_eye_patches(frames, lw[:, :2])
    with pytest.raises(TypeError):
        data.warp_eye_patches(frames[..., :2], lw)


# ------------------------------------------------------------------------------------------------ EyeNet / EVE / EVEStream keys
def camera_batch(batch, frames, lw, rw):
    b = {k_: v for k_, v in batch.items() if k_ not in ('left_eye_patch', 'right_eye_patch')}
    return dict(b, camera_frame=frames, left_eye_warp=lw, right_eye_warp=rw)


def test_eye_input_picks_the_form_and_refuses_mixtures():
    batch = clip(2, 3, seed=3, size=SIZE)
    frames, (lw, rw) = camera(2, 3, seed=4), warps_for(2, 3, seed=5)
    cam = camera_batch(batch, frames, lw, rw)
    assert eye_input(batch) is batch['left_eye_patch'] and eye_input(cam) is frames
    assert tuple(eye_input(cam).shape[:2]) == (2, 3)
    with pytest.raises(ValueError, match='not both'):
        eye_input(dict(cam, left_eye_patch=batch['left_eye_patch'], right_eye_patch=batch['right_eye_patch']))
    with pytest.raises(ValueError, match='not both'):
        eye_input(dict(batch, left_eye_warp=lw))
    for missing in ('camera_frame', 'left_eye_warp', 'right_eye_warp'):
        with pytest.raises(ValueError, match='missing ' + missing):
            eye_input({k_: v for k_, v in cam.items() if k_ != missing})
    for key, bad in (('camera_frame', frames.float()), ('camera_frame', frames[0]), ('camera_frame', frames[..., :2]),
                     ('camera_frame', frames.permute(0, 1, 4, 2, 3)), ('left_eye_warp', lw.double()), ('right_eye_warp', rw[:, :2]),
                     ('right_eye_warp', rw[..., :2]), ('left_eye_warp', lw.numpy())):
        with pytest.raises(TypeError, match=key):
            eye_input(dict(cam, **{key: bad}))


@pytest.mark.parametrize('integer', [False, True], ids=['general', 'integer-shift'])
def test_eyenet_takes_camera_frames(fake, integer):
    """forward_sequence on (camera_frame, warps) equals, bit for bit, forward_sequence on the float patches of the contract; with
    integer shifts also the run fed the uint8 crops."""
    model = make_model(dict(CONFIGS['gru-cgru'][0], **SMALL_EYES))
    B, T = 2, 2
    batch = clip(B, T, seed=3, size=SIZE)
    frames, (lw, rw) = camera(B, T, seed=6), warps_for(B, T, seed=7, integer=integer)
    fake.calls.clear()
    with torch.no_grad():
        got = model.eye_net.forward_sequence(camera_batch(batch, frames, lw, rw))
        want = model.eye_net.forward_sequence(dict(batch, left_eye_patch=contract_patches(frames, lw, (SIZE, SIZE)),
                                                   right_eye_patch=contract_patches(frames, rw, (SIZE, SIZE))))
    assert set(got) == set(want) and tuple(got['left_g_initial'].shape) == (B, T, 2)
    for key in want:
        assert torch.equal(got[key], want[key]), key
    assert not torch.equal(got['left_g_initial'], got['right_g_initial'])
    if integer:
        def crops(w):
            rows = [frames[b, t, int(w[b, t, 1, 2]):int(w[b, t, 1, 2]) + SIZE, int(w[b, t, 0, 2]):int(w[b, t, 0, 2]) + SIZE] for b in range(B) for t in range(T)]
            return torch.stack(rows).view(B, T, SIZE, SIZE, 3).contiguous()
        with torch.no_grad():
            u8 = model.eye_net.forward_sequence(dict(batch, left_eye_patch=crops(lw), right_eye_patch=crops(rw)))
        for key in want:
            assert torch.equal(got[key], u8[key]), key
    for bad in (dict(camera_batch(batch, frames, lw, rw), left_eye_patch=batch['left_eye_patch']),):
        with pytest.raises(ValueError):
            model.eye_net.forward_sequence(bad)
    with pytest.raises(ValueError):
        model.eye_net.forward_sequence({k_: v for k_, v in camera_batch(batch, frames, lw, rw).items() if k_ != 'right_eye_warp'})
    with pytest.raises(TypeError):
        model.eye_net.forward_sequence(camera_batch(batch, frames, lw.double(), rw))
    with pytest.raises(TypeError):
        model.eye_net.forward_sequence(camera_batch(batch, frames.float(), lw, rw))


def test_the_routes_issue_the_calls_they_should():
    """Patch keys: no warp call (the path they always took).  Camera keys, float32 trunk: two eye_warp_u8_to_nchw calls on the
    folded frames.  Camera keys, 16-bit trunk on 128-wide patches: two eye_warp_u8_to_stem calls into the halves of x_padded and no
    float patch in between."""
    k = LoggingWarpFakes()
    kernels.set_default_kernels(k)
    try:
        model = make_model(dict(CONFIGS['gru-cgru'][0], **SMALL_EYES))
        batch = clip(1, 2, seed=3, size=SIZE)
        frames, (lw, rw) = camera(1, 2, seed=6, C=4), warps_for(1, 2, seed=7)
        with torch.no_grad():
            model.eye_net.forward_sequence(batch)
            assert not [c for c in k.log if c[0].startswith('eye_warp')]
            del k.log[:]
            model.eye_net.forward_sequence(camera_batch(batch, frames, lw, rw))
        warp_calls = [c for c in k.log if c[0].startswith('eye_warp')]
        assert warp_calls == [['eye_warp_u8_to_nchw', [[[2, FRAME[0], FRAME[1], 4], 'torch.uint8'], [[2, 3, 3], 'torch.float32']]]] * 2
        assert not [c for c in k.log if c[0].startswith('frames_u8')]
        # the packed route: eyes_size 128 x 32 (W x H), bf16
        eve_amd.get_config().import_dict(dict(eyes_size=[128, 32]))
        net = eve_amd.EyeNet()
        net.compute_dtype = torch.bfloat16
        net.eval()
        wide = torch.from_numpy(ref.random_frames(2, 48, 160, 3, seed=8)).view(1, 2, 48, 160, 3)
        shifts = torch.from_numpy(np.stack([ref.shift(3, 2), ref.shift(30, 16)])).view(1, 2, 3, 3)
        del k.log[:]
        with torch.no_grad():
            got = net.forward_sequence(dict(camera_frame=wide, left_eye_warp=shifts, right_eye_warp=shifts.flip(1).contiguous(),
                                            left_h=batch['left_h'], right_h=batch['right_h']))
            crop = lambda t, x, y: wide[0, t, y:y + 32, x:x + 128]
            u8 = {'left_eye_patch': torch.stack([crop(0, 3, 2), crop(1, 30, 16)])[None].contiguous(),
                  'right_eye_patch': torch.stack([crop(0, 30, 16), crop(1, 3, 2)])[None].contiguous()}
            calls = [c for c in k.log if c[0].startswith(('eye_warp', 'frames_u8', 'stem_pack'))]
            want = net.forward_sequence(dict(u8, left_h=batch['left_h'], right_h=batch['right_h']))
        stem_call = ['eye_warp_u8_to_stem', [[[2, 48, 160, 3], 'torch.uint8'], [[2, 3, 3], 'torch.float32'], [[2, 38, 136, 4], 'torch.bfloat16']]]
        assert [c for c in calls if c[0] == 'eye_warp_u8_to_stem'] == [stem_call, stem_call]
        assert not [c for c in calls if c[0] in ('eye_warp_u8_to_nchw', 'frames_u8_to_stem', 'frames_u8_to_nchw')]
        for key in want:
            assert torch.equal(got[key], want[key]), key
    finally:
        kernels.set_default_kernels(None)
        eve_amd.reset_standalone_config()


def test_eve_forward_takes_camera_frames(fake):
    """EVE.forward in eval mode: B and T come from camera_frame, and every prediction equals the float-patch run's."""
    model = make_model(dict(CONFIGS['gru-cgru'][0], **SMALL_EYES))
    B, T = 1, 2
    batch = clip(B, T, seed=3, size=SIZE)
    frames, (lw, rw) = camera(B, T, seed=9), warps_for(B, T, seed=10)
    with torch.no_grad():
        got = model(camera_batch(batch, frames, lw, rw))
        want = model(dict(batch, left_eye_patch=contract_patches(frames, lw, (SIZE, SIZE)),
                          right_eye_patch=contract_patches(frames, rw, (SIZE, SIZE))))
    assert set(got) == set(want)
    for key in ('g_initial', 'PoG_px_initial', 'PoG_cm_initial', 'g_final', 'PoG_px_final', 'PoG_cm_final', 'left_pupil_size', 'right_pupil_size',
                'full_loss'):
        assert torch.equal(got[key], want[key]), key
    with pytest.raises(ValueError):
        model(dict(camera_batch(batch, frames, lw, rw), right_eye_patch=batch['right_eye_patch']))


@pytest.mark.parametrize('lengths', [None, [2, 0], [1, 2]], ids=['uniform', 'ragged-idle', 'ragged'])
def test_stream_step_takes_camera_frames(fake, lengths):
    model = make_model(dict(CONFIGS['gru-cgru'][0], **SMALL_EYES))
    B, T = 2, 2
    ch = chunk_of(clip(B, T, seed=3, size=SIZE), 0, T)
    frames, (lw, rw) = camera(B, T, seed=11, C=4), warps_for(B, T, seed=12)
    a, b = eve_amd.EVEStream(model, B, use_graph=False), eve_amd.EVEStream(model, B, use_graph=False)
    got = a.step(camera_batch(ch, frames, lw, rw), return_heatmaps=True, lengths=lengths)
    want = b.step(dict(ch, left_eye_patch=contract_patches(frames, lw, (SIZE, SIZE)), right_eye_patch=contract_patches(frames, rw, (SIZE, SIZE))),
                  return_heatmaps=True, lengths=lengths)
    assert set(got) == set(want) and 'heatmap_final' in got and ('valid' in got) == (lengths is not None)
    assert tuple(got['g_initial'].shape[:2]) == (B, T)
    for key in want:
        assert torch.equal(got[key], want[key]), key
    sa, sb = a.get_state(), b.get_state()
    for key in sb:
        for x, y in zip(sa[key] if isinstance(sa[key], tuple) else (sa[key],), sb[key] if isinstance(sb[key], tuple) else (sb[key],)):
            assert torch.equal(x, y), key
    # the stream count and the chunk length are read from camera_frame
    with pytest.raises(ValueError, match='chunk has 1 streams'):
        a.step(camera_batch({k_: v[:1] for k_, v in ch.items()}, frames[:1], lw[:1], rw[:1]))
    with pytest.raises(ValueError, match='lengths must lie in 0..2'):
        a.step(camera_batch(ch, frames, lw, rw), lengths=[3, 0])
    with pytest.raises(ValueError, match='not both'):
        a.step(dict(camera_batch(ch, frames, lw, rw), left_eye_patch=ch['left_eye_patch'], right_eye_patch=ch['right_eye_patch']))
    with pytest.raises(ValueError, match='missing left_eye_warp'):
        a.step({k_: v for k_, v in camera_batch(ch, frames, lw, rw).items() if k_ != 'left_eye_warp'})
