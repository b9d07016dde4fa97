"""CPU: eye normalisation derived from the head pose -- the contract of eve_eye_pose_normalize (tests/eye_pose_ref.py) against
hand-worked values that pin its conventions, independent float64 cross-checks (scipy's Rodrigues, numpy's general inverse) and its
degenerate rows; data.eye_pose; and the `eye_pose` key through EyeNet, EVE and EVEStream on the torch-CPU stand-in kernels, where
the pose form must equal the warp form fed the contract's derived tensors bit for bit.  tests/test_gpu_eye_pose.py checks the HIP
kernel and the graph mode."""
import math

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

import eve_amd
from eve_amd import data, kernels
from eve_amd.eye_net import EYE_POSE_DERIVED, eye_input, eye_pose_batch
import eye_pose_ref as pref
from test_eye_warp_host import FRAME, SIZE, SMALL_EYES, camera, camera_batch, warps_for
from test_eye_warp_lens_host import LensFakes, small_lens
from test_stream_host import chunk_of, clip
from test_stream_ragged_host import CONFIGS, make_model

HW = (16, 24)                 # (OH, OW) of the contract cases
NO_EYES = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
REL = 1e-12                   # the issue's tolerance for the float64 cross-checks


class PoseFakes(LensFakes):
    eye_pose_normalize = pref.eye_pose_normalize


@pytest.fixture()
def fake():
    k = PoseFakes()
    kernels.set_default_kernels(k)
    yield k
    kernels.set_default_kernels(None)
    eve_amd.reset_standalone_config()


def one(**kw):
    return pref.normalize(pref.pose_row(**kw)[None], HW)


def matrices(P, res, e, n):
    """K, Kn, S of eye e of row n, in float64."""
    p = P[n].astype(np.float64)
    K = np.array([[p[0], 0, p[2]], [0, p[1], p[3]], [0, 0, 1]])
    Kn = np.array([[p[16], 0, HW[1] / 2], [0, p[16], HW[0] / 2], [0, 0, 1]])
    return K, Kn, np.diag([1.0, 1.0, p[17] / res['d'][e, n]])


# ------------------------------------------------------------------------------------------------ the contract's conventions
def test_hand_worked_values_pin_the_conventions():
    """r = 0 and o on the optical axis: R = I, h = (0, 0), the patch centre (OW/2, OH/2) maps to (cx, cy) and, at d = distance_norm,
    the warp is K Kn^-1: a patch pixel is focal_norm / fx camera pixels wide.  head_R = Rx(a): h = (-a, 0); head_R = Ry(b): h = (0, b);
    R o / |o| = (0, 0, 1) for any pose."""
    r = one(eyes=NO_EYES)
    assert r['valid'].tolist() == [[1], [1]] and np.array_equal(r['head_R'][0], np.eye(3, dtype=np.float32))
    for e in range(2):
        assert np.array_equal(r['R'][e, 0], np.eye(3, dtype=np.float32)) and np.array_equal(r['h'][e, 0], np.zeros(2, dtype=np.float32))
        assert np.array_equal(r['o'][e, 0], np.array([0, 0, 600], dtype=np.float32))
        q = r['warp'][e, 0].astype(np.float64) @ np.array([HW[1] / 2, HW[0] / 2, 1.0])
        assert abs(q[0] / q[2] - 64.0) < 1e-5 and abs(q[1] / q[2] - 48.0) < 1e-5 and q[2] > 0
        g = 140.0 / 220.0
        want = np.array([[g, 0, 64 - 12 * g], [0, g, 48 - 8 * g], [0, 0, 1]])
        assert np.allclose(r['warp'][e, 0], want, rtol=0, atol=1e-5)
    a, b = 0.3, -0.2
    for e in range(2):
        assert np.allclose(one(r=(a, 0, 0), eyes=NO_EYES)['h'][e, 0], [-a, 0], rtol=0, atol=1e-7)
        assert np.allclose(one(r=(0, b, 0), eyes=NO_EYES)['h'][e, 0], [0, b], rtol=0, atol=1e-7)
        assert np.allclose(one(r=(0, 0, 0.4), eyes=NO_EYES)['h'][e, 0], [0, 0], rtol=0, atol=1e-7)        # a roll is taken out by R
    # the left eye is the first centre, the right one the second; o = head_R c + t
    r = one(r=(0, 0, math.pi / 2), t=(1, 2, 500))
    assert np.allclose(r['o'][0, 0], [1 + 35, 2 - 32, 525], atol=1e-4) and np.allclose(r['o'][1, 0], [1 + 35, 2 + 32, 525], atol=1e-4)
    P = pref.random_poses(50, seed=3)
    res = pref.normalize(P, HW)
    for e in range(2):
        o = res['o'][e].astype(np.float64)
        fw = np.einsum('nij,nj->ni', res['R64'][e], o / np.linalg.norm(o, axis=1, keepdims=True))
        assert np.abs(fw - np.array([0, 0, 1.0])).max() < 1e-15 * 10


def test_independent_float64_cross_checks():
    """On the contract's float64 values before their rounding: head_R against scipy's from_rotvec; det R = +1 and R R^T = I; W inv(W)
    = I against numpy's general inverse with W = Kn S R K^-1; the patch centre maps to the projection of o.  1e-12 relative, the
    matrices' entries being O(1) or scaled by their own magnitude.  (|W inv(W) - I| as this test evaluates it -- random_poses(2000,
    seed=1), every seventh row, a 24 x 16 patch -- is 5.7e-14.)"""
    P = pref.random_poses(2000, seed=1)
    res = pref.normalize(P, HW)
    assert res['valid'].all()
    want = Rotation.from_rotvec(P[:, 4:7].astype(np.float64)).as_matrix()
    assert np.abs(res['head_R64'] - want).max() <= REL
    assert np.abs(res['head_R'].astype(np.float64) - want).max() <= 2.0 ** -24          # ... and its float32 rounding
    p = P.astype(np.float64)
    Kt = (p[:, 0], p[:, 1], p[:, 2], p[:, 3])
    worst = 0.0
    for e in range(2):
        R64, d = res['R64'][e], res['d'][e]
        assert np.abs(np.linalg.det(R64) - 1.0).max() <= REL
        assert np.abs(np.einsum('nij,nkj->nik', R64, R64) - np.eye(3)).max() <= REL
        inv_w = pref.inverse_warp(R64, d, Kt, p[:, 16], p[:, 17], HW)
        for n in range(0, 2000, 7):
            K, Kn, S = matrices(P, res, e, n)
            W = Kn @ S @ R64[n] @ np.linalg.inv(K)
            worst = max(worst, float(np.abs(W @ inv_w[n] - np.eye(3)).max()))
            gen = np.linalg.inv(W)
            assert np.abs(gen / gen[2, 2] - inv_w[n] / inv_w[n][2, 2]).max() <= REL * np.abs(gen / gen[2, 2]).max()
            q = inv_w[n] @ np.array([HW[1] / 2, HW[0] / 2, 1.0])
            proj = K @ res['o'][e, n].astype(np.float64)
            assert abs(q[0] / q[2] - proj[0] / proj[2]) <= REL * abs(proj[0] / proj[2])
            assert abs(q[1] / q[2] - proj[1] / proj[2]) <= REL * abs(proj[1] / proj[2])
            assert q[2] > 0
    assert worst <= REL, worst
    # h against the angles of scipy's M = R head_R
    for e in range(2):
        M = np.einsum('nij,njk->nik', res['R'][e].astype(np.float64), res['head_R'].astype(np.float64))
        assert np.abs(res['h'][e][:, 0] - np.arcsin(M[:, 1, 2])).max() <= 1e-7
        assert np.abs(res['h'][e][:, 1] - np.arctan2(M[:, 0, 2], M[:, 2, 2])).max() <= 1e-7


def test_random_poses_keep_the_patch_in_the_frame():
    res = pref.normalize(pref.random_poses(2000, seed=2), HW)
    assert res['valid'].all()
    assert pref.patch_corners_inside(res, pref.FRAME, HW) == (True, True)


def degenerate_rows():
    """name -> (row, valid of (left, right), head_R is the identity)"""
    rows = {'theta = 0': (pref.pose_row(), (1, 1), True),
            'theta = 1e-8': (pref.pose_row(r=(1e-8, 0, 0)), (1, 1), False),
            'theta just below pi': (pref.pose_row(r=(0, math.pi - 1e-6, 0), eyes=((-32, -35, -25), (32, -35, -25))), (1, 1), False),
            'theta just above pi': (pref.pose_row(r=(0, 0, math.pi + 1e-6)), (1, 1), False),
            'o = 0': (pref.pose_row(t=(0, 0, 0), eyes=NO_EYES), (0, 0), True),
            'o_z < 0': (pref.pose_row(t=(0, 0, -600)), (0, 0), True),
            'left eye behind the camera': (pref.pose_row(t=(0, 0, 10), eyes=((-32, -35, -25), (32, -35, 25))), (0, 1), True),
            'focal_norm = 0': (pref.pose_row(focal_norm=0.0), (0, 0), True),
            'distance_norm < 0': (pref.pose_row(distance_norm=-600.0), (0, 0), True),
            'fx = 0': (pref.pose_row(K=(0.0, 140.0, 64.0, 48.0)), (0, 0), True),
            'fy < 0': (pref.pose_row(K=(140.0, -140.0, 64.0, 48.0)), (0, 0), True)}
    for i, name in enumerate(pref.FIELDS):
        for word, val in (('nan', np.nan), ('inf', np.inf)):
            row = pref.pose_row(r=(0.1, -0.2, 0.05))
            row[i] = val
            rows['%s in %s' % (word, name)] = (row, (0, 0), 4 <= i < 7)
    return rows


def test_degenerate_rows():
    """theta = 0, 1e-8 and next to pi stay valid and orthonormal; a NaN or an Inf in any field, o = 0, o_z < 0, a non-positive focal
    length or distance are invalid: warp = 0, R = I, o = 0, h = 0, with head_R still the rotation of a finite r."""
    for name, (row, valid, ident) in degenerate_rows().items():
        res = pref.normalize(row[None], HW)
        assert res['valid'][:, 0].tolist() == list(valid), name
        assert np.array_equal(res['head_R'][0], np.eye(3, dtype=np.float32)) == ident, name
        assert np.isfinite(res['head_R']).all() and abs(np.linalg.det(res['head_R'][0].astype(np.float64)) - 1) < 1e-6, name
        for e in range(2):
            if valid[e]:
                R = res['R'][e, 0].astype(np.float64)
                assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and np.isfinite(res['warp'][e, 0]).all() and np.isfinite(res['h'][e, 0]).all(), name
                assert res['warp'][e, 0][2] @ np.array([HW[1] / 2, HW[0] / 2, 1.0]) > 0, name
            else:
                assert not res['warp'][e, 0].any() and not res['o'][e, 0].any() and not res['h'][e, 0].any(), name
                assert np.array_equal(res['R'][e, 0], np.eye(3, dtype=np.float32)), name
    # theta = 1e-8: the rotation is I + [r]x to float32
    res = pref.normalize(pref.pose_row(r=(1e-8, 0, 0))[None], HW)
    assert res['head_R'][0, 2, 1] == np.float32(1e-8) and res['head_R'][0, 1, 2] == -np.float32(1e-8) and res['head_R'][0, 0, 0] == 1
    # a head x axis parallel to forward: both cross products vanish exactly.  Plain float32 rows reach it (the origin a power of two
    # times the float32 head_R's first column); so does an injected head_R; the same geometry a hair off the axis is valid
    rows = np.stack(pref.parallel_rows())
    res = pref.normalize(rows, HW)
    assert np.isfinite(rows).all() and (rows[:, 9] > 0).all() and (res['d'] > 0).all() and not res['valid'].any()
    assert not res['warp'].any() and not res['o'].any() and not res['h'].any()
    assert all(np.array_equal(res['R'][e, n], np.eye(3, dtype=np.float32)) for e in range(2) for n in range(len(rows)))
    row = pref.pose_row(t=(0, 0, 600), eyes=NO_EYES)
    along = np.array([[0, 0, -1], [0, 1, 0], [1, 0, 0]], dtype=np.float32)
    res = pref.normalize(row[None], HW, head_R=along[None])
    assert res['valid'].tolist() == [[0], [0]] and not res['warp'].any() and np.array_equal(res['R'][0, 0], np.eye(3, dtype=np.float32))
    res = pref.normalize(pref.pose_row(r=(0, -math.pi / 2, 0), t=(0, 0, 600), eyes=NO_EYES)[None], HW)
    assert res['valid'].tolist() == [[1], [1]] and abs(np.linalg.det(res['R'][0, 0].astype(np.float64)) - 1) < 1e-6
    # the clamp of stage 5: rows whose m_1 rounding carries past -1 are valid and get h = (-pi/2, 0), not a NaN
    res = pref.normalize(np.stack(pref.clamp_rows()), HW)
    with np.errstate(invalid='ignore'):
        assert res['valid'].all() and (np.abs(res['m64'][:, :, 1]) > 1).all() and np.isnan(np.arcsin(res['m64'][:, :, 1])).all()
    assert (res['h'][..., 0] == np.float32(-math.pi / 2)).all() and np.abs(res['h'][..., 1]).max() < 1e-6
    # head_R= is honoured by every later stage
    P = pref.random_poses(5, seed=9)
    base = pref.normalize(P, HW)
    other = pref.normalize(P, HW, head_R=np.ascontiguousarray(base['head_R'][::-1]))
    assert not np.array_equal(other['o'], base['o']) and np.array_equal(pref.normalize(P, HW, head_R=base['head_R'])['warp'], base['warp'])


# ------------------------------------------------------------------------------------------------ data.eye_pose / normalize_eyes
def test_eye_pose_packs_checks_and_broadcasts():
    K = np.array([[1400.0, 0, 960.5], [0, 1390.0, 540.25], [0, 0, 1]])
    rvec, tvec = np.array([[0.1], [-0.2], [0.05]]), np.array([[10.0], [-20.0], [600.0]])          # solvePnP's [3, 1]
    eyes = np.array(pref.EYES)
    row = data.eye_pose(K, rvec, tvec, eyes, 960.0, 600.0)
    assert isinstance(row, np.ndarray) and row.dtype == np.float32 and row.shape == (18,)
    want = np.array([1400, 1390, 960.5, 540.25, 0.1, -0.2, 0.05, 10, -20, 600, -32, -35, 25, 32, -35, 25, 960, 600], dtype=np.float32)
    assert np.array_equal(row, want)
    assert np.array_equal(data.eye_pose(K, rvec[:, 0], tvec[:, 0], eyes, 960.0, 600.0), want)
    # torch in, torch out; one camera and one head model for a [2, 3] clip of poses
    rv = torch.from_numpy(np.random.default_rng(0).uniform(-0.5, 0.5, (2, 3, 3, 1)))
    tv = torch.from_numpy(np.random.default_rng(1).uniform(-50, 50, (2, 3, 3)))
    rows = data.eye_pose(torch.from_numpy(K), rv, tv, eyes, 960.0, np.array([600.0, 610.0, 620.0]))
    assert torch.is_tensor(rows) and rows.dtype == torch.float32 and tuple(rows.shape) == (2, 3, 18)
    assert torch.equal(rows[1, 2, 4:7], rv[1, 2, :, 0].float()) and torch.equal(rows[0, 1, 7:10], tv[0, 1].float())
    assert torch.equal(rows[..., 17], torch.tensor([[600.0, 610.0, 620.0]] * 2)) and torch.equal(rows[1, 0, :4], torch.from_numpy(want[:4]))
    assert torch.equal(rows[..., 10:16], torch.from_numpy(want[10:16]).expand(2, 3, 6))
    skew = K.copy()
    skew[0, 1] = 0.5
    with pytest.raises(ValueError, match='skew'):
        data.eye_pose(skew, rvec, tvec, eyes, 960.0, 600.0)
    for i, val in ((0, 1e-3), (1, 1.0), (2, 2.0)):
        last = K.copy()
        last[2, i] = val
        with pytest.raises(ValueError, match='last row'):
            data.eye_pose(last, rvec, tvec, eyes, 960.0, 600.0)
    for bad in (dict(K=K[:2]), dict(rvec=np.zeros(4)), dict(tvec=np.zeros((3, 2))), dict(eyes=np.zeros((3, 3))), dict(eyes=np.zeros(3))):
        args = dict(dict(K=K, rvec=rvec, tvec=tvec, eyes=eyes), **bad)
        with pytest.raises(ValueError, match='eye_pose'):
            data.eye_pose(args['K'], args['rvec'], args['tvec'], args['eyes'], 960.0, 600.0)
    with pytest.raises(TypeError):
        data.eye_pose(K, rvec, tvec, eyes)                                # no default pretends to be EVE's virtual camera


def test_normalize_eyes_names_the_contract_s_tensors(fake):
    P = torch.from_numpy(pref.random_poses(6, seed=4)).view(2, 3, 18)
    res = pref.normalize(P.view(6, 18).numpy(), (36, 60))
    got = data.normalize_eyes(P, size=(36, 60))
    assert set(got) == set(EYE_POSE_DERIVED)
    assert torch.equal(got['head_R'], torch.from_numpy(res['head_R']).view(2, 3, 3, 3))
    for e, side in enumerate(('left', 'right')):
        for key, name, tail in (('o', '_o', (3,)), ('R', '_R', (3, 3)), ('warp', '_eye_warp', (3, 3)), ('h', '_h', (2,))):
            assert torch.equal(got[side + name], torch.from_numpy(res[key][e]).view((2, 3) + tail)), side + name
    assert got['pose_valid'].dtype == torch.bool and tuple(got['pose_valid'].shape) == (2, 3, 2) and got['pose_valid'].all()
    assert torch.equal(data.normalize_eyes(P[1, 2], size=(36, 60))['left_eye_warp'], got['left_eye_warp'][1, 2])
    assert not torch.equal(data.normalize_eyes(P)['left_eye_warp'], got['left_eye_warp'])                    # eyes_size's default: 128 x 128
    eve_amd.get_config().import_dict(dict(eyes_size=[60, 36]))
    assert torch.equal(data.normalize_eyes(P)['left_eye_warp'], got['left_eye_warp'])
    for bad in (P.double(), P[..., :17], P.numpy()):
        with pytest.raises(TypeError):
            data.normalize_eyes(bad)
    with pytest.raises(ValueError, match='no pose rows'):
        data.normalize_eyes(P[:0])


# ------------------------------------------------------------------------------------------------ EyeNet / EVE / EVEStream keys
def poses_for(B, T, seed, invalid=()):
    """Random poses whose SIZE x SIZE patches look into FRAME-sized frames -> float32 [B, T, 18]; the (b, t) listed get a NaN."""
    g = np.random.default_rng(seed)
    rows = [pref.pose_row(K=(150.0, 150.0, FRAME[1] / 2, FRAME[0] / 2), r=g.uniform(-0.3, 0.3, 3),
                          t=(g.uniform(-30, 30), g.uniform(-10, 30), g.uniform(500, 700)), focal_norm=500.0) for _ in range(B * T)]
    P = torch.from_numpy(np.stack(rows)).view(B, T, 18).clone()
    for b, t in invalid:
        P[b, t, 8] = float('nan')
    return P


def derived(P, hw=(SIZE, SIZE)):
    B, T = P.shape[:2]
    res = pref.normalize(P.reshape(B * T, 18).numpy(), hw)
    d = {'head_R': torch.from_numpy(res['head_R']).view(B, T, 3, 3)}
    for e, side in enumerate(('left', 'right')):
        d.update({side + '_o': torch.from_numpy(res['o'][e]).view(B, T, 3), side + '_R': torch.from_numpy(res['R'][e]).view(B, T, 3, 3),
                  side + '_eye_warp': torch.from_numpy(res['warp'][e]).view(B, T, 3, 3), side + '_h': torch.from_numpy(res['h'][e]).view(B, T, 2)})
    return d, torch.from_numpy(res['valid']).view(2, B, T).permute(1, 2, 0) != 0


def pose_batch(batch, frames, P):
    b = {k_: v for k_, v in batch.items() if k_ not in ('left_eye_patch', 'right_eye_patch') + EYE_POSE_DERIVED}
    return dict(b, camera_frame=frames, eye_pose=P)


def test_eye_input_takes_the_pose_form_and_raises_on_mixtures():
    batch = clip(2, 3, seed=3, size=SIZE)
    frames, (lw, rw) = camera(2, 3, seed=4), warps_for(2, 3, seed=5)
    P = poses_for(2, 3, seed=6)
    pose = pose_batch(batch, frames, P)
    assert eye_input(pose) is frames and eye_input(dict(pose, camera_lens=small_lens(2, 3, seed=7))) is frames
    for key in EYE_POSE_DERIVED + ('left_eye_patch', 'right_eye_patch'):
        with pytest.raises(ValueError, match='eye_pose.*found %s' % key):
            eye_input(dict(pose, **{key: torch.zeros(2, 3, 2)}))
    with pytest.raises(ValueError, match='eye_pose goes with camera_frame'):
        eye_input({k_: v for k_, v in pose.items() if k_ != 'camera_frame'})
    for bad in (P.double(), P.half(), P[:, :2], P[..., :17], P.view(6, 18), P.numpy()):
        with pytest.raises(TypeError, match='eye_pose'):
            eye_input(dict(pose, eye_pose=bad))
    with pytest.raises(TypeError, match='camera_frame'):
        eye_input(dict(pose, camera_frame=frames.float()))
    with pytest.raises(TypeError, match='camera_lens'):
        eye_input(dict(pose, camera_lens=torch.zeros(2, 3, 5)))
    # today's batches: accepted and rejected as before, message for message
    cam = camera_batch(batch, frames, lw, rw)
    assert eye_input(batch) is batch['left_eye_patch'] and eye_input(cam) is frames and eye_pose_batch(cam) is cam and eye_pose_batch(batch) is batch
    with pytest.raises(ValueError, match='^give the eyes either as left_eye_patch / right_eye_patch or as camera_frame / left_eye_warp / '
                                         'right_eye_warp, not both \\(found left_eye_patch, right_eye_patch, left_eye_warp\\)$'):
        eye_input(dict(batch, left_eye_warp=lw))
    with pytest.raises(ValueError, match='^the camera form needs camera_frame, left_eye_warp, right_eye_warp: missing right_eye_warp$'):
        eye_input({k_: v for k_, v in cam.items() if k_ != 'right_eye_warp'})
    with pytest.raises(ValueError, match='^camera_lens goes with camera_frame / left_eye_warp / right_eye_warp: pre-cut patches were cut '
                                         'from an undistorted frame already$'):
        eye_input(dict(batch, camera_lens=small_lens(2, 3, seed=7)))
    with pytest.raises(TypeError, match='^camera_frame must be uint8 \\[B, T, IH, IW, 3 \\| 4\\], got torch.float32'):
        eye_input(dict(cam, camera_frame=frames.float()))
    with pytest.raises(TypeError, match='^left_eye_warp must be float32 \\(2, 3, 3, 3\\), got torch.float64'):
        eye_input(dict(cam, left_eye_warp=lw.double()))
    with pytest.raises(TypeError, match='^camera_lens must be float32 \\(2, 3, 12\\), got torch.float32 \\(2, 3, 5\\)$'):
        eye_input(dict(cam, camera_lens=torch.zeros(2, 3, 5)))


def test_eye_pose_batch_runs_the_kernel_once_and_copies(fake):
    eve_amd.get_config().import_dict(SMALL_EYES)
    batch = clip(2, 3, seed=3, size=SIZE)
    P = poses_for(2, 3, seed=6, invalid=[(1, 2)])
    pose = pose_batch(batch, camera(2, 3, seed=4), P)
    keys = set(pose)
    got = eye_pose_batch(pose)
    assert set(pose) == keys and 'eye_pose' not in got and set(got) == (keys - {'eye_pose'}) | set(EYE_POSE_DERIVED)
    want, valid = derived(P)
    for key, v in want.items():
        assert torch.equal(got[key], v), key
    assert got['pose_valid'].dtype == torch.bool and torch.equal(got['pose_valid'], valid) and not valid[1, 2].any() and valid.sum() == 10
    assert eye_input(got) is pose['camera_frame']                       # the copy is the warp form


def test_eyenet_takes_the_pose_form(fake):
    model = make_model(dict(CONFIGS['gru-cgru'][0], **SMALL_EYES))
    B, T = 2, 2
    batch = clip(B, T, seed=3, size=SIZE)
    frames, P = camera(B, T, seed=6), poses_for(B, T, seed=7)
    want_in, _ = derived(P)
    pose = pose_batch(batch, frames, P)
    lens = small_lens(B, T, seed=8)
    with torch.no_grad():
        got = model.eye_net.forward_sequence(pose)
        want = model.eye_net.forward_sequence({k_: v for k_, v in dict(pose, **want_in).items() if k_ != 'eye_pose'})
        got_lens = model.eye_net.forward_sequence(dict(pose, camera_lens=lens))
        want_lens = model.eye_net.forward_sequence({k_: v for k_, v in dict(pose, camera_lens=lens, **want_in).items() if k_ != 'eye_pose'})
    assert set(got) == set(want) and tuple(got['left_g_initial'].shape) == (B, T, 2)
    for key in want:
        assert torch.equal(got[key], want[key]), key
        assert torch.equal(got_lens[key], want_lens[key]), key
    assert not torch.equal(got['left_g_initial'], got_lens['left_g_initial'])
    with pytest.raises(ValueError, match='eye_pose'):
        model.eye_net.forward_sequence(dict(pose, left_h=batch['left_h']))
    with pytest.raises(TypeError, match='eye_pose'):
        model.eye_net.forward_sequence(dict(pose, eye_pose=P.double()))


def test_eve_forward_takes_the_pose_form(fake):
    model = make_model(dict(CONFIGS['gru-cgru'][0], **SMALL_EYES))
    B, T = 1, 2
    batch = clip(B, T, seed=3, size=SIZE)
    frames, P = camera(B, T, seed=9), poses_for(B, T, seed=10)
    want_in, valid = derived(P)
    pose = pose_batch(batch, frames, P)
    warp_form = {k_: v for k_, v in dict(pose, **want_in).items() if k_ not in ('eye_pose', 'pose_valid')}
    with torch.no_grad():
        got = model(dict(pose))
        want = model(dict(warp_form))
    assert set(got) == set(want) | {'pose_valid'} and torch.equal(got['pose_valid'], valid)
    for key in ('g_initial', 'PoG_px_initial', 'PoG_cm_initial', 'g_final', 'PoG_px_final', 'PoG_cm_final', 'left_pupil_size', 'right_pupil_size',
                'full_loss', 'head_R', 'left_R', 'o'):
        assert torch.equal(got[key], want[key]), key
    assert 'eye_pose' in pose and 'left_o' not in pose                  # the caller's dict is left alone
    with pytest.raises(ValueError, match='eye_pose'):
        model(dict(pose, head_R=batch['head_R']))
    with pytest.raises(ValueError, match='eye_pose goes with camera_frame'):
        model({k_: v for k_, v in pose.items() if k_ != 'camera_frame'})


@pytest.mark.parametrize('lengths', [None, [1, 2]], ids=['uniform', 'ragged'])
def test_stream_step_takes_the_pose_form(fake, lengths):
    model = make_model(dict(CONFIGS['gru-cgru'][0], **SMALL_EYES))
    B, T = 2, 2
    ch = chunk_of(clip(B, T, seed=3, size=SIZE), 0, T)
    frames = camera(B, T, seed=11, C=4)
    P = poses_for(B, T, seed=12, invalid=[(0, 1)])
    want_in, valid = derived(P)
    pose = pose_batch(ch, frames, P)
    warp_form = {k_: v for k_, v in dict(pose, **want_in).items() if k_ != 'eye_pose'}
    a, b, c, d = (eve_amd.EVEStream(model, B, use_graph=False) for _ in range(4))
    got = a.step(pose, return_heatmaps=True, lengths=lengths)
    want = b.step(warp_form, return_heatmaps=True, lengths=lengths)
    assert set(got) == set(want) | {'pose_valid'} and 'heatmap_final' in got and ('valid' in got) == (lengths is not None)
    assert torch.equal(got['pose_valid'], valid) and 'pose_valid' not in want
    for key in want:
        assert torch.equal(got[key], want[key]), key
        assert torch.isfinite(got[key].float()).all(), key
    sa, sb = a.get_state(), b.get_state()
    for key in sb:
        for x, y in zip(sa[key] if isinstance(sa[key], tuple) else (sa[key],), sb[key] if isinstance(sb[key], tuple) else (sb[key],)):
            assert torch.equal(x, y), key
    lens = small_lens(B, T, seed=13)
    got = c.step(dict(pose, camera_lens=lens), lengths=lengths)
    want = d.step(dict(warp_form, camera_lens=lens), lengths=lengths)
    for key in want:
        assert torch.equal(got[key], want[key]), key
    with pytest.raises(ValueError, match='eye_pose'):
        a.step(dict(pose, left_R=ch['left_R']))
    with pytest.raises(ValueError, match='eye_pose goes with camera_frame'):
        a.step({k_: v for k_, v in pose.items() if k_ != 'camera_frame'})
    with pytest.raises(TypeError, match='eye_pose'):
        a.step(dict(pose, eye_pose=P[..., :17]))
