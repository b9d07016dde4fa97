"""CPU: the contract of eve_face_pose_solve_ex / eve_undistort_points (tests/face_pose_raw_ref.py) itself -- the Newton inversion of
the lens model, the reduction to the plain solve, what the Huber loss buys on contaminated landmarks, an independent minimiser --
and face_landmarks_raw / face_huber_px through eye_input, eye_pose_batch, EVE.forward and EVEStream on the torch-CPU fakes."""
import functools

import numpy as np
import pytest
import torch
from scipy.optimize import minimize
from scipy.spatial.transform import Rotation

import eve_amd
from eve_amd import data, kernels
from eve_amd.eye_net import EYE_POSE_DERIVED, FACE_LANDMARKS_KEY, FACE_LANDMARKS_RAW_KEY, FACE_RIG_KEY, eye_input, eye_pose_batch
import eye_warp_lens_ref as lref
import face_pose_raw_ref as rr
import face_pose_ref as fr
from test_eye_warp_host import FRAME, SIZE, SMALL_EYES, camera
from test_face_pose_host import SMALL_CAMERA, FaceFakes, face_batch, face_case
from test_stream_host import chunk_of, clip
from test_stream_ragged_host import CONFIGS, make_model

HUBER = 3.0
SMALL_LENS = rr.lens_row(rr.LENS_COEFFS['barrel5'], K=SMALL_CAMERA)      # the raw camera behind the FRAME-sized frames


class RawFakes(FaceFakes):
    face_pose_solve_ex = rr.face_pose_solve_ex
    undistort_points = rr.undistort_points_fake


@pytest.fixture()
def fake():
    k = RawFakes()
    kernels.set_default_kernels(k)
    yield k
    kernels.set_default_kernels(None)
    eve_amd.reset_standalone_config()


# ------------------------------------------------------------------------------------------------ 1. the inversion
def field(n, seed, half=(0.64, 0.36)):
    """n true normalised points in +-0.64 x +-0.36 (1280 x 720 at f = 1000) -> (x, y, u, v) with (u, v) the undistorted pixels."""
    g = np.random.default_rng(seed)
    x, y = g.uniform(-half[0], half[0], n), g.uniform(-half[1], half[1], n)
    return x, y, fr.CAMERA[0] * x + fr.CAMERA[2], fr.CAMERA[1] * y + fr.CAMERA[3]


@pytest.mark.parametrize('name', sorted(rr.LENSES))
def test_newton_inverts_the_lens_model(name):
    row = rr.LENSES[name]
    x, y, u, v = field(2000, seed=7)
    ud, vd, den = lref.distort(u, v, row)
    assert (den > 0).all()
    xr, yr, ok, steps = rr.undistort(ud, vd, row)
    xt, yt = (u - fr.CAMERA[2]) / fr.CAMERA[0], (v - fr.CAMERA[3]) / fr.CAMERA[1]
    err = max(np.abs(xr - xt).max(), np.abs(yr - yt).max())
    print('%s: most Newton steps %d, largest |x - x_true| %.3g, raw pixels up to %.1f px off' % (name, steps.max(), err, np.hypot(ud - u, vd - v).max()))
    assert ok.all()
    assert steps.max() <= 8              # measured 5
    assert err <= 1e-14                  # measured 4.4e-16
    # the vectorised contract is the point-by-point one
    for i in (0, 1, 1999):
        x1, y1, ok1, s1 = rr.undistort(ud[i], vd[i], row)
        assert (x1[0], y1[0], ok1[0], s1[0]) == (xr[i], yr[i], True, steps[i])


def test_zero_rows_poles_and_nans_behave_as_specified():
    x, y, u, v = field(50, seed=8)
    zero = rr.lens_row((), K=(900.0, 910.0, 600.0, 350.0))
    xr, yr, ok, steps = rr.undistort(u, v, zero)
    assert ok.all() and not steps.any()
    assert np.array_equal(xr, (u - 600.0) / 900.0) and np.array_equal(yr, (v - 350.0) / 910.0)        # (xd, yd) exactly
    neg = zero.copy()
    neg[4:] = -0.0
    assert np.array_equal(rr.undistort(u, v, neg)[0], xr)
    # the rational model's pole: D = 1 - 3 r2 vanishes at r = 0.577.  A raw point whose only pre-images lie beyond it is unusable
    pole = rr.lens_row((0, 0, 0, 0, 0, -3.0, 0, 0))
    xb, yb = np.array([0.7]), np.array([0.1])
    gx, gy = rr.distort_normalized(xb, yb, pole)                             # the image of a point beyond the pole: rad < 0
    assert gx[0] < 0
    _, _, ok, _ = rr.undistort(fr.CAMERA[0] * gx + fr.CAMERA[2], fr.CAMERA[1] * gy + fr.CAMERA[3], pole)
    xin, yin, okin, _ = rr.undistort(np.array([700.0]), np.array([380.0]), pole)
    assert not ok[0] and okin[0] and xin[0] ** 2 + yin[0] ** 2 < 1.0 / 3.0
    # through the entry's contract: a NaN row, fx = 0, a NaN point
    pts = np.stack([u, v], axis=-1).astype(np.float32)
    for bad in (np.where(np.arange(12) == 5, np.nan, rr.LENSES['barrel5']), np.where(np.arange(12) == 0, 0.0, rr.LENSES['barrel5'])):
        xy, ok = rr.undistort_points(pts, bad.astype(np.float32)[None])
        assert not ok.any() and not xy.any()
    pts[3, 1] = np.nan
    xy, ok = rr.undistort_points(pts, rr.LENSES['barrel5'][None])
    assert ok.sum() == 49 and not ok[3] and not xy[3].any() and np.isfinite(xy).all()
    # ... and in the solve: a lens row that is not usable makes the frame invalid, an unusable point is dropped
    raw, rig, lens, _ = rr.raw_sequences(1, 2, 6, seed=4)
    lens = lens.copy()
    lens[0, 1, 7] = np.inf
    res = rr.solve(raw, rig, lens)
    assert res['valid'].tolist() == [[1, 0]] and res['inliers'].tolist() == [[6, 0]]


def test_data_undistort_points_equals_the_contract(fake):
    x, y, u, v = field(40, seed=9)
    row = rr.LENSES['rational8']
    ud, vd, _ = lref.distort(u, v, row)
    pts = torch.from_numpy(np.stack([ud, vd], axis=-1).astype(np.float32)).view(4, 10, 2)
    want_xy, want_ok = rr.undistort_points(pts.view(-1, 2).numpy(), row[None])
    got, ok = data.undistort_points(pts, torch.from_numpy(row))
    assert got.dtype == torch.float64 and tuple(got.shape) == (4, 10, 2) and ok.dtype == torch.bool and ok.all() and want_ok.all()
    assert np.array_equal(got.view(-1, 2).numpy(), np.stack([1000.0 * want_xy[:, 0] + 640.0, 1000.0 * want_xy[:, 1] + 360.0], axis=-1))
    assert np.abs(got.view(-1, 2).numpy() - np.stack([u, v], axis=-1)).max() < 1e-4            # float32 raw pixels: 6e-5 px at 1000
    per = torch.from_numpy(np.stack([row, rr.LENSES['barrel5']] * 20)).view(4, 10, 12)
    got2, ok2 = data.undistort_points(pts, per)
    assert torch.equal(got2.view(-1, 2)[0::2], got.view(-1, 2)[0::2]) and not torch.equal(got2, got) and ok2.all()
    for bad_p, bad_l in ((pts.double(), per), (pts[..., :1], per), (pts, per[:, :5]), (pts, per.double()), (pts.numpy(), per)):
        with pytest.raises(TypeError):
            data.undistort_points(bad_p, bad_l)


# ------------------------------------------------------------------------------------------------ 2. the reduction
@pytest.mark.parametrize('L', [6, 68])
@pytest.mark.parametrize('weights', [False, True])
def test_no_lens_and_no_loss_is_the_plain_solve_bit_for_bit(L, weights):
    lm, rig = fr.sequences(3, 3, L, seed=40 + L, weights=weights)
    lengths, reset = np.array([3, 2, 3]), np.array([0, 0, 1])
    carried = np.zeros((3, 13))
    fr.solve(lm[:, :1], rig, state=carried)
    for kw in (dict(), dict(lengths=lengths, reset=reset)):
        sa, sb = carried.copy(), carried.copy()
        a, b = fr.solve(lm, rig, state=sa, **kw), rr.solve(lm, rig, state=sb, **kw)
        for key in ('head_R', 'head_t', 'reproj_rms', 'valid', 'accepted'):
            assert np.array_equal(a[key].view(np.uint8), b[key].view(np.uint8)), key
        assert np.array_equal(sa.view(np.uint64), sb.view(np.uint64))
        used = (lm[..., 2] > 0).sum(-1) if weights else np.full((3, 3), L)
        assert np.array_equal(b['inliers'], np.where(b['valid'] != 0, used, 0))
    # a zero-coefficient lens row with the rig's intrinsics: the same bits again
    zero = np.broadcast_to(rr.lens_row(()), (3, 3, 12)).copy()
    c = rr.solve(lm, rig, zero)
    a = fr.solve(lm, rig)
    for key in ('head_R', 'head_t', 'reproj_rms', 'valid'):
        assert np.array_equal(a[key].view(np.uint8), c[key].view(np.uint8)), key


# ------------------------------------------------------------------------------------------------ 3. robustness
@functools.lru_cache(maxsize=None)
def robust_runs(L, nout):
    rows = []
    for seed in range(40):
        model, clean, lm, R, t, idx = rr.contaminated_case(L, nout, seed)
        rig = fr.rig_row(model)
        plain, ref, hub = fr.solve_frame(lm, rig), fr.solve_frame(clean, rig), rr.solve_frame(lm, rig, None, HUBER)
        rows.append(dict(plain=rr.angle_deg(plain['R'], R) if plain['valid'] else None, clean=rr.angle_deg(ref['R'], R), valid=hub['valid'],
                         huber=rr.angle_deg(hub['R'], R), accepted=hub['accepted'], inliers=hub['inliers'], sol=hub, lm=lm, rig=rig))
    return rows


@pytest.mark.parametrize('nout', [7, 14])
def test_huber_loss_holds_the_pose_against_outliers(nout):
    """The issue's recipe, L = 68, k = 3 px, seeds 0..39.  Measured with this association: 7 outliers: Huber 0.349 deg median / 1.167
    max, 10 accepted steps, inliers 58..61, plain 3.058 / 10.44; 14 outliers: 0.389 / 1.054, 12 steps, inliers 51..54, plain 4.021 /
    10.75; clean landmarks, plain solve: 0.554 max -- so 2.11 x and 1.90 x the clean maximum, medians 8.76 x and 10.3 x apart."""
    L = 68
    rows = robust_runs(L, nout)
    assert all(r['valid'] for r in rows)
    huber, plain, clean = [r['huber'] for r in rows], [r['plain'] for r in rows if r['plain'] is not None], [r['clean'] for r in rows]
    inl = [r['inliers'] for r in rows]
    print('L = %d, %d outliers: Huber median %.3f max %.3f deg, plain median %.3f max %.3f (%d valid), clean max %.3f; most accepted %d; inliers %d..%d'
          % (L, nout, np.median(huber), max(huber), np.median(plain), max(plain), len(plain), max(clean), max(r['accepted'] for r in rows),
             min(inl), max(inl)))
    assert max(r['accepted'] for r in rows) <= 20
    assert max(huber) <= 2.5 * max(clean)
    assert np.median(plain) >= 5.0 * np.median(huber)
    assert L - nout - 6 <= min(inl) and max(inl) <= L - nout


# ------------------------------------------------------------------------------------------------ 4. an independent minimiser
def huber_cost(v, X, x, y, fx, fy, k):
    """The written Huber cost in pixels^2 of the pose (rotation vector, t), unit weights."""
    P = X @ Rotation.from_rotvec(v[:3]).as_matrix().T + v[3:]
    ex, ey = P[:, 0] / P[:, 2] - x, P[:, 1] / P[:, 2] - y
    p2 = (fx * ex) ** 2 + (fy * ey) ** 2
    r = np.sqrt(p2)
    return float(np.where(r > k, k * (2.0 * r - k), p2).sum())


def test_huber_solution_is_a_minimum_of_the_written_cost():
    """scipy.optimize.minimize (BFGS, central differences) on the Huber cost over (rotation vector, t), started at the contract's
    solution, on the first 8 contaminated cases of both recipes: it must stay where it is.  What the comparison can resolve is
    set by scipy, not by the solve: a cost around 1e3 px^2 known to 1e-16 relative leaves the minimiser's position uncertain by
    about sqrt(1e-13 / curvature), 1e-7 rad here, so BFGS may stop where it starts: the test then says that the central-difference
    gradient at the contract's solution is below gtol.  Measured: max(|dR|, |dt| / |t|) = 1.12e-10, bound 10 x that; the plain
    solve agrees with least_squares, which sees the residuals and not only their squares, to 4.3e-9."""
    worst = 0.0
    for nout in (7, 14):
        for r in robust_runs(68, nout)[:8]:
            sol, rig, lm = r['sol'], r['rig'].astype(np.float64), r['lm'].astype(np.float64)
            X = rig[12:].reshape(-1, 3)
            x, y = (lm[:, 0] - rig[2]) / rig[0], (lm[:, 1] - rig[3]) / rig[1]
            scale = np.array([1e-3, 1e-3, 1e-3, 0.1, 0.1, 1.0])            # one unit of each parameter moves the landmarks by about a pixel
            v0 = np.concatenate([Rotation.from_matrix(sol['R']).as_rotvec(), sol['t']])
            f = lambda z: huber_cost(v0 + z * scale, X, x, y, rig[0], rig[1], HUBER)
            res = minimize(f, np.zeros(6), method='BFGS', jac='3-point', options=dict(gtol=1e-9))
            v = v0 + res.x * scale
            assert res.fun <= f(np.zeros(6))
            dR = np.abs(Rotation.from_rotvec(v[:3]).as_matrix() - sol['R']).max()
            dt = np.abs(v[3:] - sol['t']).max() / np.abs(sol['t']).max()
            worst = max(worst, dR, dt)
    print('independent minimiser: worst max(|dR|, |dt| / |t|) = %.3g' % worst)
    assert worst < MINIMISER_TOL


MINIMISER_TOL = 1.2e-9               # 10 x the measured 1.12e-10


# ------------------------------------------------------------------------------------------------ 5. raw landmarks end to end
def fixed_point_inverse(ud, vd, row, passes=400):
    """An inversion of the lens model that shares nothing with Newton's: OpenCV's fixed-point pass, run until it stands still."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6 = (np.float64(t) for t in row)
    xd, yd = (ud - cx) / fx, (vd - cy) / fy
    x, y = xd.copy(), yd.copy()
    for _ in range(passes):
        r2 = x * x + y * y
        rad = (1 + r2 * (k1 + r2 * (k2 + r2 * k3))) / (1 + r2 * (k4 + r2 * (k5 + r2 * k6)))
        dx, dy = 2 * p1 * x * y + p2 * (r2 + 2 * x * x), p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (xd - dx) / rad, (yd - dy) / rad
    return fx * x + cx, fy * y + cy


@pytest.mark.parametrize('name', ['barrel5', 'rational8'])
def test_raw_landmarks_give_the_pose_of_the_undistorted_ones(name):
    """The float32 RAW landmarks are the input; their exact pre-images, float64, found by another method, go through the plain
    contract (which widens what it is given): the poses agree to 1e-9.  Measured: 1.1e-13 (barrel5) and 3.0e-13 (rational8) --
    the inversions differ by 1e-15 in normalised coordinates and both solves stop at a step below 1e-10 |t|.  Against the plain
    solve on float32 UNDISTORTED landmarks the difference is the float32 rounding of the inputs, up to 6e-5 px on each of 6..68
    landmarks that carry 1 px of noise: measured 2.5e-7 and 8.7e-8, bounded by 1e-5 (6e-5 px over a 100 px face, times ten)."""
    row = rr.LENSES[name]
    worst, worst32 = 0.0, 0.0
    for L, seed in ((6, 0), (20, 1), (68, 2), (68, 3)):
        model, lm, R, t = fr.case(L, seed)
        rig = fr.rig_row(model)
        raw = rr.distort_landmarks(lm, row)                                  # float32 raw pixels: the tracker's output
        u, v = fixed_point_inverse(raw[:, 0].astype(np.float64), raw[:, 1].astype(np.float64), row)
        back = lref.distort(u, v, row)
        assert np.abs(back[0] - raw[:, 0]).max() < 1e-9 and np.abs(back[1] - raw[:, 1]).max() < 1e-9
        want = fr.solve_frame(np.stack([u, v], axis=-1), rig)
        got = rr.solve_frame(raw, rig, row)
        near = fr.solve_frame(lm, rig)
        assert got['valid'] and want['valid'] and got['inliers'] == L and 1 <= got['newton'] <= 8
        worst = max(worst, np.abs(got['R'] - want['R']).max(), np.abs(got['t'] - want['t']).max() / np.abs(want['t']).max())
        worst32 = max(worst32, np.abs(got['R'] - near['R']).max(), np.abs(got['t'] - near['t']).max() / np.abs(near['t']).max())
    print('%s: raw against exact pre-images %.3g; against float32 undistorted landmarks %.3g' % (name, worst, worst32))
    assert worst <= 1e-9
    assert worst32 <= 1e-5


def raw_case(B, T, seed, invalid=()):
    """face_case seen through SMALL_LENS -> (raw landmarks, rig, lens [B, T, 12], the undistorted landmarks) as tensors."""
    lm, rig = face_case(B, T, seed, invalid=invalid)
    raw = torch.from_numpy(rr.distort_landmarks(lm.numpy(), SMALL_LENS))
    lens = torch.from_numpy(np.broadcast_to(SMALL_LENS, (B, T, 12)).copy())
    return raw, rig, lens, lm


def raw_batch(batch, frames, raw, rig, lens):
    b = {k_: v for k_, v in batch.items() if k_ not in ('left_eye_patch', 'right_eye_patch') + EYE_POSE_DERIVED}
    return dict(b, camera_frame=frames, face_landmarks_raw=raw, face_rig=rig, camera_lens=lens)


def warp_form_of_raw(face, raw, rig, lens, huber=None, lengths=None, state=None, reset=None, key=FACE_LANDMARKS_RAW_KEY):
    """The warp form the contract derives -> (the batch, pose_valid, the solve's dict)."""
    B, T = raw.shape[:2]
    sol = rr.solve(raw.numpy(), rig.numpy(), None if lens is None else lens.numpy(), huber, lengths, state, reset)
    res = fr.normalize_rt(rig.numpy(), sol['head_R'], sol['head_t'], sol['valid'], (SIZE, SIZE))
    d = {k_: v for k_, v in face.items() if k_ not in (key, FACE_RIG_KEY)}
    d['head_R'] = torch.from_numpy(sol['head_R'])
    for e, side in enumerate(('left', 'right')):
        d.update({side + '_o': torch.from_numpy(res['o'][e]).view(B, T, 3), side + '_R': torch.from_numpy(res['R'][e]).view(B, T, 3, 3),
                  side + '_eye_warp': torch.from_numpy(res['warp'][e]).view(B, T, 3, 3), side + '_h': torch.from_numpy(res['h'][e]).view(B, T, 2)})
    valid = torch.from_numpy(res['valid']).view(2, B, T).permute(1, 2, 0) != 0
    return d, valid, {k_: torch.from_numpy(v) for k_, v in sol.items()}


def test_eye_input_takes_the_raw_key_and_refuses_mixtures():
    batch = clip(2, 3, seed=3, size=SIZE)
    frames = camera(2, 3, seed=4)
    raw, rig, lens, lm = raw_case(2, 3, seed=5)
    face = raw_batch(batch, frames, raw, rig, lens)
    assert eye_input(face) is frames and eye_input(dict(face, face_landmarks_raw=raw[..., :2].contiguous())) is frames
    with pytest.raises(ValueError, match='face_landmarks_raw.*needs camera_lens'):
        eye_input({k_: v for k_, v in face.items() if k_ != 'camera_lens'})
    with pytest.raises(ValueError, match='not both'):
        eye_input(dict(face, face_landmarks=lm))
    with pytest.raises(ValueError, match='not both'):
        eye_pose_batch(dict(face, face_landmarks=lm))
    for key in EYE_POSE_DERIVED + ('head_t', 'face_reproj_rms', 'face_inliers', 'left_eye_patch', 'right_eye_patch', 'eye_pose'):
        with pytest.raises(ValueError, match='face_landmarks_raw.*found %s' % key):
            eye_input(dict(face, **{key: torch.zeros(2, 3, 2)}))
    with pytest.raises(ValueError, match='needs face_landmarks_raw and face_rig'):
        eye_input({k_: v for k_, v in face.items() if k_ != FACE_RIG_KEY})
    with pytest.raises(ValueError, match='face_landmarks_raw goes with camera_frame'):
        eye_input({k_: v for k_, v in face.items() if k_ != 'camera_frame'})
    for bad in (raw.double(), raw[:, :2], raw[..., :1], raw.numpy(), torch.zeros(2, 3, 69, 2)):
        with pytest.raises(TypeError, match='face_landmarks_raw'):
            eye_input(dict(face, face_landmarks_raw=bad))
    with pytest.raises(TypeError, match='camera_lens'):
        eye_input(dict(face, camera_lens=lens[:, :2]))
    # face_landmarks + camera_lens keeps its meaning: accepted, the landmarks are the undistorted image's
    assert eye_input(dict({k_: v for k_, v in face.items() if k_ != FACE_LANDMARKS_RAW_KEY}, face_landmarks=lm)) is frames


def test_eye_pose_batch_picks_the_entry(fake):
    eve_amd.get_config().import_dict(SMALL_EYES)
    batch = clip(2, 3, seed=3, size=SIZE)
    raw, rig, lens, lm = raw_case(2, 3, seed=6, invalid=[(1, 1)])
    face = raw_batch(batch, camera(2, 3, seed=4), raw, rig, lens)
    calls = []
    for name in ('face_pose_solve', 'face_pose_solve_ex'):
        setattr(fake, name, (lambda n, f: lambda *a, **k_: calls.append(n) or f(*a, **k_))(name, getattr(fake, name)))
    keys = set(face)
    got = eye_pose_batch(face)
    assert calls == ['face_pose_solve_ex'] and set(face) == keys
    assert set(got) == (keys - {FACE_LANDMARKS_RAW_KEY, FACE_RIG_KEY}) | set(EYE_POSE_DERIVED) | {'head_t', 'face_reproj_rms', 'face_inliers'}
    want, valid, sol = warp_form_of_raw(face, raw, rig, lens)
    for key in EYE_POSE_DERIVED[:-1]:
        assert torch.equal(got[key], want[key]), key
    assert torch.equal(got['head_t'], sol['head_t']) and torch.equal(got['face_reproj_rms'], sol['reproj_rms'])
    assert got['face_inliers'].dtype == torch.uint8 and torch.equal(got['face_inliers'], sol['inliers'])
    assert got['face_inliers'].tolist() == [[7, 7, 7], [7, 0, 7]] and torch.equal(got['pose_valid'], valid) and not valid[1, 1].any()
    assert 'camera_lens' in got and eye_input(got) is face['camera_frame']
    # the plain key: today's entry without the attribute, the new one with it; the loss changes the pose only slightly on clean landmarks
    plain = {k_: v for k_, v in face_batch(batch, face['camera_frame'], lm, rig).items()}
    del calls[:]
    a = eye_pose_batch(plain)
    b = eye_pose_batch(plain, huber_px=HUBER)
    assert calls == ['face_pose_solve', 'face_pose_solve_ex'] and 'face_inliers' not in a and 'face_inliers' in b
    assert torch.equal(b['head_t'], warp_form_of_raw(plain, lm, rig, None, HUBER, key=FACE_LANDMARKS_KEY)[2]['head_t'])
    for bad in (0, -1.0, float('nan'), float('inf'), 'three', True, torch.tensor(3.0)):
        with pytest.raises(ValueError, match='huber_px'):
            eye_pose_batch(plain, huber_px=bad)
    # the stand-alone entry
    s0 = data.solve_head_pose(lm, rig)
    s1 = data.solve_head_pose(raw, rig, lens=lens, huber_px=HUBER)
    want = rr.solve(raw.numpy(), rig.numpy(), lens.numpy(), HUBER)
    assert 'inliers' not in s0 and set(s1) == set(s0) | {'inliers'} and s1['valid'].dtype == torch.bool
    for key in ('head_R', 'head_t', 'reproj_rms', 'inliers'):
        assert np.array_equal(s1[key].numpy(), want[key]), key
    single = data.solve_head_pose(raw[0], rig[0], lens=lens[0])
    assert torch.equal(single['head_t'], got['head_t'][0]) and tuple(single['inliers'].shape) == (3,)
    with pytest.raises(TypeError, match='lens'):
        data.solve_head_pose(raw, rig, lens=lens[:, :2])
    with pytest.raises(ValueError, match='huber_px'):
        data.solve_head_pose(raw, rig, huber_px=0)


def test_eve_forward_takes_the_raw_key_and_the_loss(fake):
    model = make_model(dict(CONFIGS['gru-cgru'][0], **SMALL_EYES))
    B, T = 1, 2
    batch = clip(B, T, seed=3, size=SIZE)
    raw, rig, lens, lm = raw_case(B, T, seed=10)
    face = raw_batch(batch, camera(B, T, seed=9), raw, rig, lens)
    model.eye_net.face_huber_px = HUBER
    try:
        warp_form, valid, sol = warp_form_of_raw(face, raw, rig, lens, HUBER)
        with torch.no_grad():
            got = model(dict(face))
            want = model(dict(warp_form))
        assert set(got) == set(want) | {'pose_valid', 'head_t', 'face_reproj_rms', 'face_inliers'} and valid.all()
        assert torch.equal(got['head_t'], sol['head_t']) and torch.equal(got['face_inliers'], sol['inliers']) and (sol['inliers'] >= 4).all()
        for key in ('g_initial', 'PoG_px_initial', 'g_final', 'PoG_px_final', 'left_pupil_size', 'full_loss', 'head_R', 'left_R', 'o'):
            assert torch.equal(got[key], want[key]), key
        model.eye_net.face_huber_px = -2
        with pytest.raises(ValueError, match='huber_px'):
            model(dict(face))
    finally:
        model.eye_net.face_huber_px = None
    with torch.no_grad():
        assert 'face_inliers' in model(dict(face))                            # the raw key alone runs the new entry too


def test_stream_chunks_equal_one_pass_and_the_graph_key(fake):
    model = make_model(dict(CONFIGS['gru-cgru'][0], **SMALL_EYES))
    B, T = 2, 4
    full = chunk_of(clip(B, T, seed=3, size=SIZE), 0, T)
    raw, rig, lens, lm = raw_case(B, T, seed=12)
    face = raw_batch(full, camera(B, T, seed=11), raw, rig, lens)
    cut = lambda i: {k_: (v if k_ == FACE_RIG_KEY else v[:, 2 * i:2 * i + 2].contiguous()) for k_, v in face.items()}
    model.eye_net.face_huber_px = HUBER
    try:
        one, two, three = (eve_amd.EVEStream(model, B, use_graph=False) for _ in range(3))
        whole = one.step(face)
        assert {'pose_valid', 'head_t', 'face_reproj_rms', 'face_inliers'} <= set(whole) and whole['pose_valid'].all()
        parts = [{k_: v.clone() for k_, v in two.step(cut(i)).items()} for i in range(2)]
        for key in whole:
            assert torch.equal(torch.cat([parts[0][key], parts[1][key]], dim=1), whole[key]), key
        assert torch.equal(one._face_pose, two._face_pose)
        state = np.zeros((B, 13))
        for i in range(2):
            wf, valid, sol = warp_form_of_raw(cut(i), raw[:, 2 * i:2 * i + 2], rig, lens[:, 2 * i:2 * i + 2], HUBER, state=state)
            assert torch.equal(parts[i]['head_t'], sol['head_t']) and torch.equal(parts[i]['face_inliers'], sol['inliers'])
            assert torch.equal(parts[i]['pose_valid'], valid)
        assert np.array_equal(state, two._face_pose.numpy())
        # lengths, a reset and skip_invalid_pose combine as in the plain form
        three.step(cut(0))
        three.reset([1])
        got = three.step(cut(1), lengths=[2, 1], skip_invalid_pose=True)
        st = state_after(raw, rig, lens)
        want = rr.solve(raw[:, 2:].numpy(), rig.numpy(), lens[:, 2:].numpy(), HUBER, lengths=[2, 1], state=st, reset=[0, 1])
        assert np.array_equal(got['head_t'].numpy()[want['valid'] != 0], want['head_t'][want['valid'] != 0])
        assert got['valid'].tolist() == [[True, True], [True, False]] and np.array_equal(three._face_pose.numpy(), st)
        # the graph's key: the landmark key and face_huber_px
        stream = eve_amd.EVEStream(model, B, use_graph=False)
        captured = []
        stream._capture = lambda chunk, *a, **k_: captured.append(model.eye_net.face_huber_px) or {'n': len(captured)}
        ch = cut(0)
        first = stream._graph_for(ch, False)
        assert stream._graph_for(dict(ch), False) is first
        model.eye_net.face_huber_px = 2.0
        second = stream._graph_for(ch, False)
        model.eye_net.face_huber_px = None
        third = stream._graph_for(ch, False)
        model.eye_net.face_huber_px = HUBER
        assert stream._graph_for(ch, False) is first and second is not first and third is not second and captured == [HUBER, 2.0, None]
        plain = dict({k_: v for k_, v in ch.items() if k_ != FACE_LANDMARKS_RAW_KEY}, face_landmarks=ch[FACE_LANDMARKS_RAW_KEY])
        assert stream._graph_for(plain, False) is not first and len(stream._graphs) == 4
        model.eye_net.face_huber_px = [3.0]                                    # a value that is refused never becomes a key
        with pytest.raises(ValueError, match='huber_px'):
            stream._graph_for(ch, False)
        assert len(stream._graphs) == 4
        patches = chunk_of(clip(B, 2, seed=3, size=SIZE), 0, 2)                # a chunk without landmarks: the attribute is not in its key
        k1 = stream._graph_key(patches, False)
        model.eye_net.face_huber_px = 2.0
        assert stream._graph_key(patches, False) == k1
    finally:
        model.eye_net.face_huber_px = None


def state_after(raw, rig, lens):
    state = np.zeros((raw.shape[0], 13))
    rr.solve(raw[:, :2].numpy(), rig.numpy(), lens[:, :2].numpy(), HUBER, state=state)
    return state
