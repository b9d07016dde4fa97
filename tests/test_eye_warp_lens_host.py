"""CPU: eye patches cut from RAW camera frames through the camera's lens model -- the contract of eve_eye_warp_lens_u8_to_nchw /
_to_stem (tests/eye_warp_lens_ref.py) against hand-worked values, the plain contract and its degenerate rows; data.camera_lens;
and the `camera_lens` key from data.warp_eye_patches through EyeNet, EVE and EVEStream on the torch-CPU stand-in kernels.
tests/test_gpu_eye_warp_lens.py checks the HIP kernels and the graph mode."""
import numpy as np
import pytest
import torch

import eve_amd
from eve_amd import data, kernels
from eve_amd.eye_net import eye_input
import eye_warp_lens_ref as lref
import eye_warp_ref as ref
from test_eye_warp_host import FRAME, SIZE, SMALL_EYES, bits, camera, camera_batch, contract_patches, warps_for
from test_stream_host import chunk_of, clip
from test_stream_ragged_host import CONFIGS, LoggingFakes, RaggedFakes, make_model

HW = (128, 128)
BIG = (160, 200)              # the frames of the contract cases, (IH, IW)


class LensFakes(RaggedFakes):
    eye_warp_u8_to_nchw = ref.eye_warp_u8_to_nchw
    eye_warp_u8_to_stem = ref.eye_warp_u8_to_stem
    eye_warp_lens_u8_to_nchw = lref.eye_warp_lens_u8_to_nchw
    eye_warp_lens_u8_to_stem = lref.eye_warp_lens_u8_to_stem


class LoggingLensFakes(LoggingFakes):
    eye_warp_u8_to_nchw = ref.eye_warp_u8_to_nchw
    eye_warp_u8_to_stem = ref.eye_warp_u8_to_stem
    eye_warp_lens_u8_to_nchw = lref.eye_warp_lens_u8_to_nchw
    eye_warp_lens_u8_to_stem = lref.eye_warp_lens_u8_to_stem


@pytest.fixture()
def fake():
    k = LensFakes()
    kernels.set_default_kernels(k)
    yield k
    kernels.set_default_kernels(None)
    eve_amd.reset_standalone_config()


def small_lens(B, T, seed):
    """One barrel5-like camera per (stream, frame) for FRAME-sized frames -> float32 [B, T, 12]."""
    g = np.random.default_rng(seed)
    rows = [lref.lens_row(110 + g.uniform(-5, 5), 110 + g.uniform(-5, 5), FRAME[1] / 2 + g.uniform(-3, 3), FRAME[0] / 2 + g.uniform(-3, 3),
                          k1=-0.25 + g.uniform(-0.02, 0.02), k2=0.08, p1=1e-3, p2=-5e-4, k3=-0.01) for _ in range(B * T)]
    return torch.from_numpy(np.stack(rows)).view(B, T, 12)


def lens_patches(frames, warps, lens, hw):
    B, T = frames.shape[:2]
    v, _ = lref.eye_warp(frames.numpy().reshape((B * T,) + tuple(frames.shape[2:])), warps.numpy().reshape(B * T, 3, 3),
                         lens.numpy().reshape(B * T, 12), hw)
    return torch.from_numpy(v).view((B, T, 3) + hw)


# ------------------------------------------------------------------------------------------------ the contract
def test_hand_worked_values_pin_the_convention():
    """fx = fy = 100, cx = cy = 0, (u, v) = (50, 0): x = 0.5, y = 0, r2 = 0.25.
      k1 = 0.4: rad = 1.1, ud = 100 * 0.55 = 55                    p2 = 0.1: xd = 0.5 + 0.1 * (0.25 + 0.5) = 0.575, ud = 57.5
      p1 = 0.1: yd = 0.1 * (0.25 + 0) = 0.025, vd = 2.5, ud = 50    k4 = 1.0: rad = 1 / 1.25, ud = 40
    OpenCV's 2 p1 x y + p2 (r2 + 2 x^2) in x, p1 (r2 + 2 y^2) + 2 p2 x y in y: the swapped convention would move p1 along x."""
    row = lambda **kw: [100.0, 100.0, 0.0, 0.0] + [kw.get(n_, 0.0) for n_ in ('k1', 'k2', 'p1', 'p2', 'k3', 'k4', 'k5', 'k6')]
    for kw, (wu, wv) in ((dict(k1=0.4), (55.0, 0.0)), (dict(p2=0.1), (57.5, 0.0)), (dict(p1=0.1), (50.0, 2.5)), (dict(k4=1.0), (40.0, 0.0))):
        ud, vd, den = lref.distort(50.0, 0.0, row(**kw))
        assert abs(float(ud) - wu) <= 1e-12 and abs(float(vd) - wv) <= 1e-12 and float(den) > 0, (kw, float(ud), float(vd))
    # the order of a row: k3 sits behind p2, k4..k6 last
    ud, _, den = lref.distort(50.0, 0.0, lref.lens_row(100, 100, 0, 0, k3=0.64).astype(np.float64))
    assert abs(float(ud) - 50.0 * (1 + 0.64 * 0.25 ** 3)) <= 1e-5 and float(den) == 1.0
    _, _, den = lref.distort(50.0, 0.0, lref.lens_row(100, 100, 0, 0, k6=64.0).astype(np.float64))
    assert float(den) == 2.0
    # cx, cy and distinct focal lengths
    ud, vd, _ = lref.distort(60.0, 105.0, [100.0, 50.0, 10.0, 5.0] + [0.0] * 8)
    assert (float(ud), float(vd)) == (60.0, 105.0)                 # x = 0.5, y = 2: exact without coefficients


def test_a_zero_coefficient_row_is_the_plain_warp():
    """... bit for bit and whatever the intrinsics say (negative zeros and absurd intrinsics included), also for the pixels it
    leaves outside; fx*((u - cx)/fx) + cx itself is not u."""
    v = ref.random_frames(2, BIG[0], BIG[1], 3, seed=1)
    zero = np.stack([lref.lens_row(180, 180, 100, 80), lref.lens_row(0, np.nan, -5, 1e30, k1=-0.0, p2=-0.0, k6=-0.0)])
    assert all(lref.takes_the_plain_path(r) for r in zero) and not lref.takes_the_plain_path(lref.LENSES['tangential'])
    assert not lref.takes_the_plain_path(lref.lens_row(1, 1, 0, 0, k5=np.nan))
    for name, (m, kind) in ref.WARPS.items():
        mm = np.stack([m, m])
        got, outside = lref.eye_warp(v, mm, zero, HW)
        want, want_out = ref.eye_warp(v, mm, HW)
        assert ref.outside_share_ok(kind, float(outside.mean())), name
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(outside, want_out), name
    u = np.arange(0, 200, dtype=np.float64) + 1 / 3
    x = (u - 100.0) / 180.0
    assert (180.0 * x + 100.0 != u).any()


@pytest.mark.parametrize('lens_name', list(lref.LENSES))
def test_the_shared_lenses_move_the_patch_and_keep_their_outside_shares(lens_name):
    v = ref.random_frames(1, BIG[0], BIG[1], 3, seed=2)
    L = lref.LENSES[lens_name]
    for name in (ref.WARPS if lens_name in ('barrel5', 'rational8') else ('integer-shift', 'fractional-shift')):
        m = ref.WARPS[name][0]
        got, outside = lref.eye_warp(v, m[None], L[None], HW)
        assert ref.outside_share_ok(lref.outside_kind(lens_name, name), float(outside.mean())), (name, float(outside.mean()))
        assert (got[0][:, outside[0]] == -1.0).all() and got.min() >= -1.0 and got.max() <= 1.0
        fu, fv, inside, pole = lref.coordinates(m, L, BIG, HW)
        pu, pv, plain_inside, _ = lref.coordinates(m, lref.lens_row(1, 1, 0, 0), BIG, HW)
        both = inside & plain_inside
        assert (((fu != pu) | (fv != pv))[both]).mean() > 0.98               # a build that ignores the lens cannot pass
        if lens_name == 'pole' and name == 'fractional-shift':                 # beyond the pole rad flips sign and lands inside
            assert 0.11 < pole.mean() < 0.12 and outside[0][pole].all()
        elif lens_name != 'pole':
            assert not pole.any()


def test_nan_and_zero_focal_rows_are_black():
    v = ref.random_frames(1, BIG[0], BIG[1], 3, seed=3)
    m = ref.WARPS['integer-shift'][0][None]
    b5 = lref.LENSES['barrel5']
    rows = {'all nan': np.full((12,), np.nan, dtype=np.float32), 'fx = 0': b5 * np.array([0] + [1] * 11, dtype=np.float32),
            'fy = 0': b5 * np.array([1, 0] + [1] * 10, dtype=np.float32)}
    for i in range(12):                         # a NaN anywhere in a row with coefficients
        r = b5.copy()
        r[i] = np.nan
        rows['nan at %d' % i] = r
    for name, row in rows.items():
        got, outside = lref.eye_warp(v, m, row[None], HW)
        assert outside.all() and (got == -1.0).all(), name
    mirrored = b5 * np.array([-1] + [1] * 11, dtype=np.float32)               # a negative focal length simply works
    got, outside = lref.eye_warp(v, m, mirrored[None], HW)
    assert not outside.all() and not np.array_equal(got, lref.eye_warp(v, m, b5[None], HW)[0])


def test_malformed_lens_requests_raise():
    f = np.zeros((2, 8, 8, 3), dtype=np.uint8)
    ident = np.stack([ref.shift(0, 0)] * 2)
    with pytest.raises(ValueError):
        lref.eye_warp(f, ident, np.zeros((1, 12), dtype=np.float32), (4, 4))
    with pytest.raises(ValueError):
        lref.eye_warp(f, ident, np.zeros((2, 5), dtype=np.float32), (4, 4))
    with pytest.raises(ValueError):
        lref.eye_warp(f[..., :2], ident, np.zeros((2, 12), dtype=np.float32), (4, 4))
    k = LensFakes()
    t = lambda a: torch.from_numpy(a)
    for lens in (torch.zeros((2, 12), dtype=torch.float64), torch.zeros((2, 5)), torch.zeros((1, 12))):
        with pytest.raises(TypeError):
            k.eye_warp_lens_u8_to_nchw(t(f), t(ident), lens, (4, 4))


# ------------------------------------------------------------------------------------------------ data.camera_lens
def test_camera_lens_lays_out_opencv_calibrations():
    K = np.array([[1400.0, 0, 960.5], [0, 1390.0, 540.25], [0, 0, 1]])
    d8 = np.array([0.9, 0.1, 2e-3, 1e-3, 0.01, 1.1, 0.15, 0.02])
    for n in (4, 5, 8):
        row = data.camera_lens(K, d8[:n])
        assert isinstance(row, np.ndarray) and row.dtype == np.float32 and row.shape == (12,)
        want = np.zeros(12)
        want[:4] = [1400.0, 1390.0, 960.5, 540.25]
        want[4:4 + n] = d8[:n]                 # k1, k2, p1, p2, k3, k4, k5, k6: OpenCV's own order
        assert np.array_equal(row, want.astype(np.float32)), n
    assert np.array_equal(data.camera_lens(K, d8[:5]), lref.lens_row(1400, 1390, 960.5, 540.25, k1=0.9, k2=0.1, p1=2e-3, p2=1e-3, k3=0.01))
    # torch in, torch out; leading dimensions broadcast
    Ks = torch.from_numpy(np.stack([K, K * np.array([[2.0], [2.0], [1.0]])])).view(2, 1, 3, 3)
    ds = torch.from_numpy(np.stack([d8[:5], d8[:5] * 2, d8[:5] * 3]))
    rows = data.camera_lens(Ks, ds)
    assert torch.is_tensor(rows) and rows.dtype == torch.float32 and tuple(rows.shape) == (2, 3, 12)
    assert torch.equal(rows[1, 2, :4], torch.tensor([2800.0, 2780.0, 1921.0, 1080.5]))
    assert torch.equal(rows[0, 1, 4:9], (ds[1]).float()) and not rows[..., 9:].any()
    assert tuple(data.camera_lens(Ks.numpy()[:, 0], d8).shape) == (2, 12)
    assert tuple(data.camera_lens(K.astype(np.float32), np.zeros((7, 4), dtype=np.float32)).shape) == (7, 12)
    for bad in (np.zeros(12), np.zeros(14), np.zeros(6), np.zeros(())):
        with pytest.raises(ValueError):
            data.camera_lens(K, bad)
    skew = K.copy()
    skew[0, 1] = 0.5
    with pytest.raises(ValueError, match='skew'):
        data.camera_lens(skew, d8)
    for i, val in ((0, 1e-3), (1, 1.0), (2, 2.0)):
        last = K.copy()
        last[2, i] = val
        with pytest.raises(ValueError, match='last row'):
            data.camera_lens(last, d8)
    with pytest.raises(ValueError):
        data.camera_lens(K[:2], d8)


def test_warp_eye_patches_takes_lens_rows(fake):
    frames, (lw, _) = camera(2, 3, seed=1, C=4), warps_for(2, 3, seed=2)
    lens = small_lens(2, 3, seed=3)
    got = data.warp_eye_patches(frames, lw, size=(36, 60), lens=lens)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 3, 3, 36, 60)
    assert torch.equal(got, lens_patches(frames, lw, lens, (36, 60)))
    plain = data.warp_eye_patches(frames, lw, size=(36, 60))
    assert torch.equal(plain, contract_patches(frames, lw, (36, 60))) and not torch.equal(got, plain)
    zero = lens.clone()
    zero[..., 4:] = 0
    assert torch.equal(data.warp_eye_patches(frames, lw, size=(36, 60), lens=zero), plain)
    assert torch.equal(data.warp_eye_patches(frames[1], lw[1], size=(36, 60), lens=lens[1]), got[1])
    for bad in (lens.double(), lens[:, :2], lens[..., :5], lens.numpy()):
        with pytest.raises(TypeError):
            data.warp_eye_patches(frames, lw, size=(36, 60), lens=bad)


# ------------------------------------------------------------------------------------------------ EyeNet / EVE / EVEStream keys
def test_eye_input_validates_the_lens():
    batch = clip(2, 3, seed=3, size=SIZE)
    frames, (lw, rw) = camera(2, 3, seed=4), warps_for(2, 3, seed=5)
    lens = small_lens(2, 3, seed=6)
    cam = dict(camera_batch(batch, frames, lw, rw), camera_lens=lens)
    assert eye_input(cam) is frames
    for bad in (lens.double(), lens.half(), lens[:, :2], lens[..., :5], lens.view(6, 12), lens.numpy(), lens[:, :, None].expand(2, 3, 2, 12)):
        with pytest.raises(TypeError, match='camera_lens'):
            eye_input(dict(cam, camera_lens=bad))
    with pytest.raises(ValueError, match='camera_lens'):
        eye_input(dict(batch, camera_lens=lens))                     # pre-cut patches came from an undistorted frame already
    with pytest.raises(ValueError, match='missing left_eye_warp'):
        eye_input({k_: v for k_, v in cam.items() if k_ != 'left_eye_warp'})


def test_eyenet_takes_raw_frames_and_a_lens(fake):
    """forward_sequence on (camera_frame, warps, camera_lens) equals, bit for bit, forward_sequence on the float patches of the lens
    contract -- and not the plain contract's; without the key the batch behaves as before."""
    model = make_model(dict(CONFIGS['gru-cgru'][0], **SMALL_EYES))
    B, T = 2, 2
    batch = clip(B, T, seed=3, size=SIZE)
    frames, (lw, rw) = camera(B, T, seed=6), warps_for(B, T, seed=7)
    lens = small_lens(B, T, seed=8)
    cam = camera_batch(batch, frames, lw, rw)
    with torch.no_grad():
        got = model.eye_net.forward_sequence(dict(cam, camera_lens=lens))
        want = model.eye_net.forward_sequence(dict(batch, left_eye_patch=lens_patches(frames, lw, lens, (SIZE, SIZE)),
                                                   right_eye_patch=lens_patches(frames, rw, lens, (SIZE, SIZE))))
        plain = model.eye_net.forward_sequence(cam)
        plain_want = model.eye_net.forward_sequence(dict(batch, left_eye_patch=contract_patches(frames, lw, (SIZE, SIZE)),
                                                         right_eye_patch=contract_patches(frames, rw, (SIZE, SIZE))))
    assert set(got) == set(want) and tuple(got['left_g_initial'].shape) == (B, T, 2)
    for key in want:
        assert torch.equal(got[key], want[key]), key
        assert torch.equal(plain[key], plain_want[key]), key
    assert not torch.equal(got['left_g_initial'], plain['left_g_initial'])
    with pytest.raises(TypeError, match='camera_lens'):
        model.eye_net.forward_sequence(dict(cam, camera_lens=lens.double()))
    with pytest.raises(ValueError, match='camera_lens'):
        model.eye_net.forward_sequence(dict(batch, camera_lens=lens))


def test_the_lens_routes_issue_the_lens_calls():
    """Camera keys with camera_lens, float32 trunk: two eye_warp_lens_u8_to_nchw calls, the lens rows folded to [B*T, 12]; 16-bit
    trunk on 128-wide patches: two eye_warp_lens_u8_to_stem calls into the halves of x_padded.  Never a plain warp call beside them,
    and without the key never a lens call."""
    k = LoggingLensFakes()
    kernels.set_default_kernels(k)
    try:
        model = make_model(dict(CONFIGS['gru-cgru'][0], **SMALL_EYES))
        batch = clip(1, 2, seed=3, size=SIZE)
        frames, (lw, rw) = camera(1, 2, seed=6, C=4), warps_for(1, 2, seed=7)
        lens = small_lens(1, 2, seed=8)
        with torch.no_grad():
            model.eye_net.forward_sequence(camera_batch(batch, frames, lw, rw))
            assert [c[0] for c in k.log if c[0].startswith('eye_warp')] == ['eye_warp_u8_to_nchw'] * 2
            del k.log[:]
            model.eye_net.forward_sequence(dict(camera_batch(batch, frames, lw, rw), camera_lens=lens))
        calls = [c for c in k.log if c[0].startswith('eye_warp')]
        assert calls == [['eye_warp_lens_u8_to_nchw', [[[2, FRAME[0], FRAME[1], 4], 'torch.uint8'], [[2, 3, 3], 'torch.float32'],
                                                       [[2, 12], 'torch.float32']]]] * 2
        eve_amd.get_config().import_dict(dict(eyes_size=[128, 32]))
        net = eve_amd.EyeNet()
        net.compute_dtype = torch.bfloat16
        net.eval()
        wide = torch.from_numpy(ref.random_frames(2, 48, 160, 3, seed=8)).view(1, 2, 48, 160, 3)
        shifts = torch.from_numpy(np.stack([ref.shift(3.5, 2.25), ref.shift(30, 16)])).view(1, 2, 3, 3)
        wl = torch.from_numpy(np.stack([lref.lens_row(150, 150, 80, 24, k1=-0.2, k2=0.05), lref.lens_row(150, 150, 80, 24)])).view(1, 2, 12)
        del k.log[:]
        with torch.no_grad():
            got = net.forward_sequence(dict(camera_frame=wide, left_eye_warp=shifts, right_eye_warp=shifts.flip(1).contiguous(), camera_lens=wl,
                                            left_h=batch['left_h'], right_h=batch['right_h']))
            calls = [c for c in k.log if c[0].startswith(('eye_warp', 'frames_u8', 'stem_pack'))]
            want = net.forward_sequence(dict(left_eye_patch=lens_patches(wide, shifts, wl, (32, 128)),
                                             right_eye_patch=lens_patches(wide, shifts.flip(1).contiguous(), wl, (32, 128)),
                                             left_h=batch['left_h'], right_h=batch['right_h']))
        stem_call = ['eye_warp_lens_u8_to_stem', [[[2, 48, 160, 3], 'torch.uint8'], [[2, 3, 3], 'torch.float32'], [[2, 12], 'torch.float32'],
                                                  [[2, 38, 136, 4], 'torch.bfloat16']]]
        assert [c for c in calls if c[0].startswith('eye_warp')] == [stem_call, stem_call]
        assert not [c for c in calls if c[0].startswith('frames_u8')]
        for key in want:
            assert torch.equal(got[key], want[key]), key
    finally:
        kernels.set_default_kernels(None)
        eve_amd.reset_standalone_config()


def test_eve_forward_takes_raw_frames_and_a_lens(fake):
    model = make_model(dict(CONFIGS['gru-cgru'][0], **SMALL_EYES))
    B, T = 1, 2
    batch = clip(B, T, seed=3, size=SIZE)
    frames, (lw, rw) = camera(B, T, seed=9), warps_for(B, T, seed=10)
    lens = small_lens(B, T, seed=11)
    with torch.no_grad():
        got = model(dict(camera_batch(batch, frames, lw, rw), camera_lens=lens))
        want = model(dict(batch, left_eye_patch=lens_patches(frames, lw, lens, (SIZE, SIZE)),
                          right_eye_patch=lens_patches(frames, rw, lens, (SIZE, SIZE))))
        plain = model(camera_batch(batch, frames, lw, rw))
    assert set(got) == set(want) == set(plain)
    for key in ('g_initial', 'PoG_px_initial', 'PoG_cm_initial', 'g_final', 'PoG_px_final', 'PoG_cm_final', 'left_pupil_size', 'right_pupil_size',
                'full_loss'):
        assert torch.equal(got[key], want[key]), key
    assert not torch.equal(got['g_initial'], plain['g_initial'])
    with pytest.raises(ValueError, match='camera_lens'):
        model(dict(batch, camera_lens=lens))


@pytest.mark.parametrize('lengths', [None, [1, 2]], ids=['uniform', 'ragged'])
def test_stream_step_takes_raw_frames_and_a_lens(fake, lengths):
    model = make_model(dict(CONFIGS['gru-cgru'][0], **SMALL_EYES))
    B, T = 2, 2
    ch = chunk_of(clip(B, T, seed=3, size=SIZE), 0, T)
    frames, (lw, rw) = camera(B, T, seed=11, C=4), warps_for(B, T, seed=12)
    lens = small_lens(B, T, seed=13)
    cam = camera_batch(ch, frames, lw, rw)
    a, b, c, d = (eve_amd.EVEStream(model, B, use_graph=False) for _ in range(4))
    got = a.step(dict(cam, camera_lens=lens), return_heatmaps=True, lengths=lengths)
    want = b.step(dict(ch, left_eye_patch=lens_patches(frames, lw, lens, (SIZE, SIZE)), right_eye_patch=lens_patches(frames, rw, lens, (SIZE, SIZE))),
                  return_heatmaps=True, lengths=lengths)
    assert set(got) == set(want) and 'heatmap_final' in got and ('valid' in got) == (lengths is not None)
    for key in want:
        assert torch.equal(got[key], want[key]), key
    sa, sb = a.get_state(), b.get_state()
    for key in sb:
        for x, y in zip(sa[key] if isinstance(sa[key], tuple) else (sa[key],), sb[key] if isinstance(sb[key], tuple) else (sb[key],)):
            assert torch.equal(x, y), key
    # a chunk without the key behaves as before
    plain = c.step(cam, return_heatmaps=True, lengths=lengths)
    plain_want = d.step(dict(ch, left_eye_patch=contract_patches(frames, lw, (SIZE, SIZE)), right_eye_patch=contract_patches(frames, rw, (SIZE, SIZE))),
                        return_heatmaps=True, lengths=lengths)
    for key in plain_want:
        assert torch.equal(plain[key], plain_want[key]), key
    assert not torch.equal(plain['g_initial'], got['g_initial'])
    with pytest.raises(TypeError, match='camera_lens'):
        a.step(dict(cam, camera_lens=lens[..., :5]))
    with pytest.raises(ValueError, match='camera_lens'):
        a.step(dict(ch, camera_lens=lens))
