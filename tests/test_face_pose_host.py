"""CPU: the contract of eve_face_pose_solve in numpy (tests/face_pose_ref.py) against an independent solver, data.face_rig, the key
rules of the face-landmark form (camera_frame + face_landmarks + face_rig), and -- with the contract installed as the kernels'
stand-in -- the form through eye_pose_batch, EVE.forward and EVEStream, whose carried pose makes chunks equal one pass."""
import numpy as np
import pytest
import torch
from scipy.optimize import least_squares
from scipy.spatial.transform import Rotation

import eve_amd
from eve_amd import data, kernels
from eve_amd.eye_net import EYE_POSE_DERIVED, FACE_LANDMARKS_KEY, FACE_RIG_KEY, eye_input, eye_pose_batch
import face_pose_ref as fr
from test_eye_pose_host import PoseFakes, poses_for
from test_eye_warp_host import FRAME, SIZE, SMALL_EYES, camera
from test_stream_host import chunk_of, clip
from test_stream_mask_host import MaskFakes
from test_stream_ragged_host import CONFIGS, make_model

SMALL_CAMERA = (150.0, 150.0, FRAME[1] / 2, FRAME[0] / 2)      # the camera behind the FRAME-sized frames of the host-path tests


class FaceFakes(PoseFakes, MaskFakes):
    face_pose_solve = fr.face_pose_solve
    eye_pose_normalize_rt = fr.eye_pose_normalize_rt


@pytest.fixture()
def fake():
    k = FaceFakes()
    kernels.set_default_kernels(k)
    yield k
    kernels.set_default_kernels(None)
    eve_amd.reset_standalone_config()


# ------------------------------------------------------------------------------------------------ (a) the reference itself
def scipy_pose(model, lm, R0, t0):
    """scipy.optimize.least_squares over (rvec, tvec) on the same float32 landmarks, from the true pose."""
    K = fr.CAMERA
    p, X = lm.astype(np.float64), model.astype(np.float64)
    w = p[:, 2] if p.shape[1] == 3 else np.ones(len(p))
    x, y = (p[:, 0] - K[2]) / K[0], (p[:, 1] - K[3]) / K[1]
    sw = np.sqrt(w)

    def residuals(v):
        P = X @ Rotation.from_rotvec(v[:3]).as_matrix().T + v[3:]
        return np.concatenate([sw * (P[:, 0] / P[:, 2] - x), sw * (P[:, 1] / P[:, 2] - y)])

    v0 = np.concatenate([Rotation.from_matrix(R0).as_rotvec(), t0])
    sol = least_squares(residuals, v0, xtol=1e-15, ftol=1e-15, gtol=1e-15, x_scale=np.array([1.0, 1.0, 1.0, 100.0, 100.0, 100.0]))
    return Rotation.from_rotvec(sol.x[:3]).as_matrix(), sol.x[3:]


def test_reference_agrees_with_an_independent_solver():
    """240 cold cases of the issue (L in 6, 7, 64, 65, 68; 24 seeds; with and without weights; pitch and yaw within +-40 degrees;
    1 px of noise): every one must be valid -- none is left out -- within the cap of 32 accepted steps, and agree with scipy."""
    worst, most = 0.0, 0
    for L in fr.MODEL_SIZES:
        for seed in range(24):
            for weights in (False, True):
                model, lm, R, t = fr.case(L, seed, weights)
                res = fr.solve_frame(lm, fr.rig_row(model))
                assert res['valid'], (L, seed, weights)
                Rs, ts = scipy_pose(model, lm, R, t)
                worst = max(worst, np.abs(Rs - res['R']).max(), np.abs(ts - res['t']).max() / np.abs(ts).max())
                most = max(most, res['accepted'])
                assert 0.0 < res['rms'] < 3.0                                        # 1 px of noise per coordinate
                assert np.abs(res['R'] @ res['R'].T - np.eye(3)).max() < 1e-14       # the Cayley update keeps R orthogonal
    print('worst max(|dR|, |dt| / |t|) = %.3g, most accepted steps = %d' % (worst, most))
    assert most <= 32
    assert worst < 4.4e-8            # 10 x the worst value measured on these cases, 4.32e-9 (most accepted steps: 16); the issue: <= 1e-6


def test_warm_starts_need_fewer_steps_and_chunks_equal_one_pass():
    lm, rig = fr.sequences(3, 5, 7, seed=3, weights=True)
    one = fr.solve(lm, rig)
    assert one['valid'].all() and (one['accepted'][:, 1:] <= one['accepted'][:, :1] + 2).all() and one['accepted'][:, 1:].max() <= 8
    state = np.zeros((3, 13))
    a = fr.solve(lm[:, :2], rig, state=state)
    assert (state[:, 12] == 1).all()
    keep = state.copy()
    b = fr.solve(lm[:, 2:], rig, state=state)
    for key in ('head_R', 'head_t', 'reproj_rms', 'valid'):
        assert np.array_equal(np.concatenate([a[key], b[key]], axis=1), one[key]), key
    # a reset is a cold start; a sequence with no frames keeps its pose
    after, state = state, keep.copy()
    c = fr.solve(lm[:, 2:], rig, state=state, reset=np.array([0, 1, 0]), lengths=np.array([3, 3, 0]))
    cold_state = np.zeros((1, 13))
    cold = fr.solve(lm[1:2, 2:], rig[1:2], state=cold_state)
    # (both starts reach the same float32 pose: the float64 state and the step counts tell them apart)
    assert np.array_equal(c['head_R'][1], cold['head_R'][0]) and np.array_equal(c['accepted'][1], cold['accepted'][0])
    assert c['accepted'][1, 0] > b['accepted'][1, 0] and np.array_equal(state[1], cold_state[0]) and not np.array_equal(state[1], after[1])
    assert np.array_equal(c['accepted'][0], b['accepted'][0]) and np.array_equal(state[0], after[0])
    assert np.array_equal(state[2], keep[2]) and not c['valid'][2].any()


def test_frames_without_a_solution():
    lm, rig = fr.sequences(1, 3, 6, seed=4, weights=True)
    ok = fr.solve(lm, rig)
    assert ok['valid'].all()

    nan = lm.copy()
    nan[0, 1, 2, 0] = np.nan
    res = fr.solve(nan, rig)
    assert res['valid'].tolist() == [[1, 0, 1]] and np.array_equal(res['head_R'][0, 1], np.eye(3)) and not res['head_t'][0, 1].any()
    assert res['accepted'][0, 2] == fr.solve(lm[:, 2:], rig)['accepted'][0, 0] > ok['accepted'][0, 2]     # the next frame started cold
    three = lm.copy()
    three[0, 1, 3:, 2] = 0.0
    assert fr.solve(three, rig)['valid'].tolist() == [[1, 0, 1]]
    line = rig.copy()
    line[0, 12:] = np.stack([np.linspace(-60, 60, 6), np.linspace(-30, 30, 6), np.linspace(-12, 12, 6)], axis=-1).reshape(-1)
    g = np.random.default_rng(5)
    R, t = fr.random_pose(g)
    lm_line = np.stack([fr.project(line[0, 12:].reshape(6, 3), R, t, g=g) for _ in range(3)])[None]
    assert not fr.solve(lm_line, line)['valid'].any()
    zero_f = rig.copy()
    zero_f[0, 0] = 0.0
    assert not fr.solve(lm, zero_f)['valid'].any()


# ------------------------------------------------------------------------------------------------ (b) data.face_rig
def test_face_rig_packs_checks_and_broadcasts():
    K = np.array([[1000.0, 0, 640], [0, 990.0, 360], [0, 0, 1]])
    model = fr.head_model(6, 1)
    rig = data.face_rig(K, model, np.array(fr.EYES), 220.0, 600.0)
    assert rig.dtype == np.float32 and rig.shape == (30,)
    assert np.array_equal(rig, fr.rig_row(model, K=(1000.0, 990.0, 640.0, 360.0)))
    many = data.face_rig(torch.from_numpy(K), torch.from_numpy(np.stack([model, 2 * model])), np.array(fr.EYES), [220.0, 230.0], 600.0)
    assert torch.is_tensor(many) and many.dtype == torch.float32 and tuple(many.shape) == (2, 30)
    assert np.array_equal(many[0].numpy(), rig) and many[1, 10] == 230.0 and np.array_equal(many[1, 12:].numpy(), 2 * model.reshape(-1))
    skew, last = K.copy(), K.copy()
    skew[0, 1], last[2, 2] = 0.5, 2.0
    for bad, word in ((dict(camera_matrix=skew), 'skew'), (dict(camera_matrix=last), 'last row'), (dict(camera_matrix=K[:2]), '3, 3'),
                      (dict(face_model=model[:3]), '4 <= L <= 68'), (dict(face_model=np.zeros((69, 3))), '4 <= L <= 68'),
                      (dict(face_model=model[:, :2]), 'face_model'), (dict(eye_centers=np.zeros((3,))), 'eye_centers')):
        kw = dict(dict(camera_matrix=K, face_model=model, eye_centers=np.array(fr.EYES), focal_norm=220.0, distance_norm=600.0), **bad)
        with pytest.raises(ValueError, match='face_rig.*' + word):
            data.face_rig(**kw)


# ------------------------------------------------------------------------------------------------ (c) the keys
def face_case(B, T, seed, L=7, invalid=()):
    """Landmarks of frontal heads in front of SMALL_CAMERA, whose SIZE patches look into FRAME-sized frames -> (landmarks float32
    [B, T, L, 3], rig float32 [B, 12 + 3L]) tensors; the (b, t) listed get a NaN."""
    lm, rig = fr.sequences(B, T, L, seed, weights=True, K=SMALL_CAMERA, frontal=True, focal_norm=500.0, step_deg=2.0, step_mm=4.0, noise=0.15)
    lm = lm.copy()
    for b, t in invalid:
        lm[b, t, 1, 1] = np.nan
    return torch.from_numpy(lm), torch.from_numpy(rig)


def face_batch(batch, frames, lm, rig):
    b = {k_: v for k_, v in batch.items() if k_ not in ('left_eye_patch', 'right_eye_patch') + EYE_POSE_DERIVED}
    return dict(b, camera_frame=frames, face_landmarks=lm, face_rig=rig)


def warp_form_of(face, lm, rig, lengths=None, state=None, reset=None):
    """The warp form the contract derives from the landmarks -> (the batch, pose_valid, head_t, rms)."""
    B, T = lm.shape[:2]
    sol = fr.solve(lm.numpy(), rig.numpy(), lengths, state, reset)
    res = fr.normalize_rt(rig.numpy(), sol['head_R'], sol['head_t'], sol['valid'], (SIZE, SIZE))
    d = {k_: v for k_, v in face.items() if k_ not in (FACE_LANDMARKS_KEY, FACE_RIG_KEY)}
    d['head_R'] = torch.from_numpy(sol['head_R'])
    for e, side in enumerate(('left', 'right')):
        d.update({side + '_o': torch.from_numpy(res['o'][e]).view(B, T, 3), side + '_R': torch.from_numpy(res['R'][e]).view(B, T, 3, 3),
                  side + '_eye_warp': torch.from_numpy(res['warp'][e]).view(B, T, 3, 3), side + '_h': torch.from_numpy(res['h'][e]).view(B, T, 2)})
    valid = torch.from_numpy(res['valid']).view(2, B, T).permute(1, 2, 0) != 0
    return d, valid, torch.from_numpy(sol['head_t']), torch.from_numpy(sol['reproj_rms'])


def test_eye_input_takes_the_face_landmark_form_and_raises_on_mixtures():
    batch = clip(2, 3, seed=3, size=SIZE)
    frames = camera(2, 3, seed=4)
    lm, rig = face_case(2, 3, seed=5)
    face = face_batch(batch, frames, lm, rig)
    assert eye_input(face) is frames and eye_input(dict(face, face_landmarks=lm[..., :2].contiguous())) is frames
    nv12 = {k_: v for k_, v in face.items() if k_ != 'camera_frame'}
    nv12['camera_frame_nv12'] = torch.zeros((2, 3, FRAME[0] * 3 // 2, FRAME[1]), dtype=torch.uint8)
    assert eye_input(nv12) is nv12['camera_frame_nv12']
    for key in EYE_POSE_DERIVED + ('head_t', 'face_reproj_rms', 'left_eye_patch', 'right_eye_patch', 'eye_pose'):
        with pytest.raises(ValueError, match='face_landmarks.*found %s' % key):
            eye_input(dict(face, **{key: torch.zeros(2, 3, 2)}))
    with pytest.raises(ValueError, match='two|one camera frame key'):
        eye_input(dict(face, camera_frame_bgr=frames))
    for half in (FACE_LANDMARKS_KEY, FACE_RIG_KEY):
        with pytest.raises(ValueError, match='needs face_landmarks and face_rig'):
            eye_input({k_: v for k_, v in face.items() if k_ != half})
    with pytest.raises(ValueError, match='face_landmarks goes with camera_frame'):
        eye_input({k_: v for k_, v in face.items() if k_ != 'camera_frame'})
    for bad in (lm.double(), lm[:, :2], lm[:, :, :3], lm[..., :1], lm.view(2, 3, 21), lm.numpy(), torch.zeros(2, 3, 69, 2)):
        with pytest.raises(TypeError, match='face_landmarks'):
            eye_input(dict(face, face_landmarks=bad))
    for bad in (rig.double(), rig[:1], rig[:, :-1], rig[:, None].expand(2, 3, 33), rig.numpy()):
        with pytest.raises(TypeError, match='face_rig'):
            eye_input(dict(face, face_rig=bad))
    with pytest.raises(TypeError, match='camera_lens'):
        eye_input(dict(face, camera_lens=torch.zeros(2, 3, 5)))
    # the pose form beside it is as it was
    P = poses_for(2, 3, seed=6)
    pose = dict({k_: v for k_, v in face.items() if k_ not in (FACE_LANDMARKS_KEY, FACE_RIG_KEY)}, eye_pose=P)
    assert eye_input(pose) is frames


def test_eye_pose_batch_solves_and_copies(fake):
    eve_amd.get_config().import_dict(SMALL_EYES)
    batch = clip(2, 3, seed=3, size=SIZE)
    lm, rig = face_case(2, 3, seed=6, invalid=[(1, 1)])
    face = face_batch(batch, camera(2, 3, seed=4), lm, rig)
    keys = set(face)
    got = eye_pose_batch(face)
    assert set(face) == keys and set(got) == (keys - {FACE_LANDMARKS_KEY, FACE_RIG_KEY}) | set(EYE_POSE_DERIVED) | {'head_t', 'face_reproj_rms'}
    want, valid, head_t, rms = warp_form_of(face, lm, rig)
    for key in EYE_POSE_DERIVED[:-1]:
        assert torch.equal(got[key], want[key]), key
    assert torch.equal(got['head_t'], head_t) and torch.equal(got['face_reproj_rms'], rms) and tuple(rms.shape) == (2, 3)
    assert got['pose_valid'].dtype == torch.bool and torch.equal(got['pose_valid'], valid) and not valid[1, 1].any() and valid.sum() == 10
    assert not got['left_eye_warp'][1, 1].any() and (rms[valid.all(-1)] > 0).all() and rms[1, 1] == 0
    assert eye_input(got) is face['camera_frame']                       # the copy is the warp form
    sol = data.solve_head_pose(lm, rig)                                 # the stand-alone entry: the same solve
    assert torch.equal(sol['head_R'], got['head_R']) and torch.equal(sol['head_t'], head_t) and torch.equal(sol['reproj_rms'], rms)
    assert sol['valid'].dtype == torch.bool and torch.equal(sol['valid'], valid.all(-1))
    single = data.solve_head_pose(lm[0], rig[0], )
    assert torch.equal(single['head_t'], head_t[0]) and tuple(single['valid'].shape) == (3,)
    ragged = data.solve_head_pose(lm, rig, lengths=[3, 1])
    assert ragged['valid'].tolist() == [[True, True, True], [True, False, False]]
    for bad in (lm.double(), lm[..., :1], lm.numpy()):
        with pytest.raises(TypeError, match='landmarks'):
            data.solve_head_pose(bad, rig)
    with pytest.raises(TypeError, match='rig'):
        data.solve_head_pose(lm, rig[:, :-3].contiguous())


def test_eve_forward_takes_the_face_landmark_form(fake):
    model = make_model(dict(CONFIGS['gru-cgru'][0], **SMALL_EYES))
    B, T = 1, 2
    batch = clip(B, T, seed=3, size=SIZE)
    lm, rig = face_case(B, T, seed=10)
    face = face_batch(batch, camera(B, T, seed=9), lm, rig)
    warp_form, valid, head_t, rms = warp_form_of(face, lm, rig)
    with torch.no_grad():
        got = model(dict(face))
        want = model(dict(warp_form))
    assert set(got) == set(want) | {'pose_valid', 'head_t', 'face_reproj_rms'} and torch.equal(got['pose_valid'], valid) and valid.all()
    assert torch.equal(got['head_t'], head_t) and torch.equal(got['face_reproj_rms'], rms)
    for key in ('g_initial', 'PoG_px_initial', 'g_final', 'PoG_px_final', 'left_pupil_size', 'full_loss', 'head_R', 'left_R', 'o'):
        assert torch.equal(got[key], want[key]), key
    assert FACE_LANDMARKS_KEY in face and 'left_o' not in face           # the caller's dict is left alone
    with pytest.raises(ValueError, match='face_landmarks'):
        model(dict(face, head_R=batch['head_R']))


# ------------------------------------------------------------------------------------------------ (d) the carried pose
def test_stream_chunks_equal_one_pass_and_a_reset_starts_cold(fake):
    """A 4-frame clip in one step, and as 2 + 2 frames through the EVEStream's carried pose: the same bits; with stream 1 reset in
    between, stream 1's second chunk equals a cold solve of those frames and stream 0 is as before."""
    model = make_model(dict(CONFIGS['gru-cgru'][0], **SMALL_EYES))
    B, T = 2, 4
    full = chunk_of(clip(B, T, seed=3, size=SIZE), 0, T)
    lm, rig = face_case(B, T, seed=12)
    face = face_batch(full, camera(B, T, seed=11), lm, rig)
    cut = lambda i: {k_: (v if k_ == FACE_RIG_KEY else v[:, 2 * i:2 * i + 2].contiguous()) for k_, v in face.items()}
    one, two, three = (eve_amd.EVEStream(model, B, use_graph=False) for _ in range(3))
    whole = one.step(face)
    assert {'pose_valid', 'head_t', 'face_reproj_rms'} <= set(whole) and whole['pose_valid'].all()
    R0, t0, has0 = two.get_head_pose()
    assert not has0.any() and tuple(R0.shape) == (B, 3, 3) and R0.dtype == torch.float64
    parts = [{k_: v.clone() for k_, v in two.step(cut(i)).items()} for i in range(2)]
    for key in whole:
        assert torch.equal(torch.cat([parts[0][key], parts[1][key]], dim=1), whole[key]), key
    for x, y in zip(one.get_head_pose(), two.get_head_pose()):
        assert torch.equal(x, y)
    assert two.get_head_pose()[2].all() and torch.equal(two.get_head_pose()[1].float(), whole['head_t'][:, -1])
    assert set(two.get_state()) == set(eve_amd.EVEStream(model, B, use_graph=False).get_state())      # the keys it always had
    # the same against the contract, warp form and all
    state = np.zeros((B, 13))
    for i in range(2):
        wf, valid, head_t, rms = warp_form_of(cut(i), lm[:, 2 * i:2 * i + 2], rig, state=state)
        assert torch.equal(parts[i]['head_t'], head_t) and torch.equal(parts[i]['face_reproj_rms'], rms) and torch.equal(parts[i]['pose_valid'], valid)
    assert np.array_equal(state, two._face_pose.numpy())
    # a reset of stream 1 between the chunks
    three.step(cut(0))
    three.reset([1])
    got = three.step(cut(1))
    cold = np.zeros((1, 13))                # (both starts reach the same float32 pose: the carried float64 pose tells them apart)
    fr.solve(lm[1:, 2:].numpy(), rig[1:].numpy(), state=cold)
    assert np.array_equal(three._face_pose[1].numpy(), cold[0]) and not np.array_equal(cold[0], two._face_pose[1].numpy())
    assert torch.equal(three._face_pose[0], two._face_pose[0]) and torch.equal(got['head_t'][0], parts[1]['head_t'][0])
    # set_head_pose puts a pose back: the second chunk from stream 0's carried pose after the first
    four = eve_amd.EVEStream(model, B, use_graph=False)
    four.set_head_pose(torch.from_numpy(state_after_first(lm, rig)[:, :9]).view(B, 3, 3), torch.from_numpy(state_after_first(lm, rig)[:, 9:12]), True)
    again = four.step(cut(1))
    assert torch.equal(again['head_t'], parts[1]['head_t']) and torch.equal(four._face_pose, two._face_pose)
    with pytest.raises(ValueError, match='set_head_pose'):
        four.set_head_pose(torch.zeros(3, 3), torch.zeros(3))


def state_after_first(lm, rig):
    state = np.zeros((lm.shape[0], 13))
    fr.solve(lm[:, :2].numpy(), rig.numpy(), state=state)
    return state


@pytest.mark.parametrize('lengths', [None, [1, 2]], ids=['uniform', 'ragged'])
def test_stream_step_takes_the_face_landmark_form(fake, lengths):
    """Against the warp form fed what the contract derives; frame (0, 1) has a NaN landmark.  With skip_invalid_pose the frame
    without a solution is skipped like any unusable frame."""
    model = make_model(dict(CONFIGS['gru-cgru'][0], **SMALL_EYES))
    B, T = 2, 2
    ch = chunk_of(clip(B, T, seed=3, size=SIZE), 0, T)
    lm, rig = face_case(B, T, seed=13, invalid=[(0, 1)])
    face = face_batch(ch, camera(B, T, seed=11, C=4), lm, rig)
    warp_form, valid, head_t, rms = warp_form_of(face, lm, rig, lengths)
    a, b, c, d = (eve_amd.EVEStream(model, B, use_graph=False) for _ in range(4))
    got = a.step(face, return_heatmaps=True, lengths=lengths)
    want = b.step(warp_form, return_heatmaps=True, lengths=lengths)
    assert set(got) == set(want) | {'pose_valid', 'head_t', 'face_reproj_rms'} and ('valid' in got) == (lengths is not None)
    assert torch.equal(got['pose_valid'], valid) and not valid[0, 1].any() and torch.equal(got['head_t'], head_t)
    for key in want:
        assert torch.equal(got[key], want[key]), key
        assert torch.isfinite(got[key].float()).all(), key
    assert a.get_head_pose()[2].tolist() == ([False, True] if lengths is None else [True, True])      # lengths [1, 2]: the NaN frame is never solved
    got = c.step(face, lengths=lengths, skip_invalid_pose=True)
    mask = valid if lengths is None else valid & (torch.arange(T)[None, :] < torch.tensor(lengths)[:, None])[..., None]
    want = d.step(warp_form, lengths=lengths, eye_mask=mask)
    for key in want:
        assert torch.equal(got[key], want[key]), key
    with pytest.raises(ValueError, match='skip_invalid_pose'):
        a.step(warp_form, skip_invalid_pose=True)
