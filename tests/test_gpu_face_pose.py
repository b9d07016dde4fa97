"""GPU: eve_face_pose_solve (csrc/face_pose.hip) against its contract in numpy (tests/face_pose_ref.py) bit for bit -- head_R,
head_t, valid and the carried float64 state; reproj_rms within one float32 ulp -- eve_eye_pose_normalize_rt against
tests/eye_pose_ref.py continued from the solved pose, and the face-landmark form (camera_frame + face_landmarks + face_rig)
through EVEStream, eager and under graph replay, against the warp form fed what data.solve_head_pose and the normalisation
produce.  Shapes S = 3, T = 5; both starts of a frame reach the same float32 pose, so what tells a cold start from a warm one is
the float64 state, which is compared as well."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import eve_amd
from eve_amd import data
from eve_amd.kernels import default_kernels
import face_pose_ref as fr
from test_gpu_eye_pose import ptr, ulps
from test_gpu_stream import gpu_clip, make_model

pytestmark = pytest.mark.gpu
S, T = 3, 5
GUARD = 64
SENTINEL, SENTINEL8 = -7.0, 0x5A
CAM = (64, 96)                # (IH, IW) of the end-to-end frames
CAM_K = (100.0, 100.0, CAM[1] / 2, CAM[0] / 2)


@functools.lru_cache(maxsize=None)
def shared(L, weights):
    """The landmarks, the rig and the contract's answer (with its final state), computed once -> read only."""
    lm, rig = fr.planar_sequences(S, T, seed=2) if L == 4 else fr.sequences(S, T, L, seed=10 + L, weights=weights)
    state = np.zeros((S, 13))
    want = fr.solve(lm, rig, state=state)
    for a in (lm, rig, state) + tuple(want.values()):
        a.setflags(write=False)
    return lm, rig, want, state


def solve(lm, rig, lengths=None, state=None, reset=None):
    """HipKernels.face_pose_solve on numpy arrays -> dict of numpy outputs (state, a cuda tensor, is updated in place)."""
    k = default_kernels()
    dev = lambda a, dtype: None if a is None else torch.as_tensor(np.asarray(a), dtype=dtype).cuda()
    out = k.face_pose_solve(torch.from_numpy(np.array(lm)).cuda(), torch.from_numpy(np.array(rig)).cuda(), dev(lengths, torch.int32), state,
                            dev(reset, torch.int32))
    assert k.lib.eve_last_kernel() == b'face_pose_solve_kernel'
    return dict(zip(('head_R', 'head_t', 'reproj_rms', 'valid'), (t.cpu().numpy() for t in out)))


def same(got, want, what=''):
    assert np.array_equal(got['valid'], want['valid']), (what, got['valid'], want['valid'])
    for name in ('head_R', 'head_t'):
        g, w = got[name].view(np.uint32), want[name].view(np.uint32)
        assert np.array_equal(g, w), '%s %s: %d of %d elements differ, first at %s' % (what, name, int((g != w).sum()), g.size, np.argwhere(g != w)[0])
    assert ulps(got['reproj_rms'], want['reproj_rms']) <= 1, what


# ------------------------------------------------------------------------------------------------ the kernel against its contract
@pytest.mark.parametrize('L,weights', [(4, False), (6, True), (6, False), (64, True), (65, False), (68, True)])
def test_kernel_equals_the_contract_bit_for_bit(L, weights):
    """Every sequence starts cold at up to +-40 degrees and then moves; L = 64, 65, 68 give lanes a second point; L = 4 is planar (bits
    only).  The float64 state after the clip is the contract's as well."""
    lm, rig, want, want_state = shared(L, weights)
    assert lm.shape == (S, T, L, 3 if weights else 2)
    if L != 4:
        assert want['valid'].all() and 3 <= want['accepted'].min() and want['accepted'].max() <= 32
    state = torch.zeros((S, 13), dtype=torch.float64, device='cuda')
    got = solve(lm, rig, state=state)
    same(got, want, 'L = %d' % L)
    assert np.array_equal(state.cpu().numpy().view(np.uint64), want_state.view(np.uint64))
    same(solve(lm, rig), want, 'without a state')


def test_raw_launch_stays_inside_its_buffers():
    k = default_kernels()
    lm, rig, want, _ = shared(68, True)
    N = S * T
    bufs = {name: torch.full((N * width + GUARD,), SENTINEL, dtype=torch.float32, device='cuda') for name, width in
            (('head_R', 9), ('head_t', 3), ('reproj_rms', 1))}
    valid = torch.full((N + GUARD,), SENTINEL8, dtype=torch.uint8, device='cuda')
    state = torch.full((S * 13 + GUARD,), SENTINEL, dtype=torch.float64, device='cuda')
    state[:S * 13] = 0
    lm_d, rig_d = torch.from_numpy(np.array(lm)).cuda(), torch.from_numpy(np.array(rig)).cuda()
    status = k.lib.eve_face_pose_solve(S, T, 68, 3, ptr(lm_d), ptr(rig_d), None, ptr(state), None, ptr(bufs['head_R']), ptr(bufs['head_t']),
                                       ptr(bufs['reproj_rms']), ptr(valid), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert status == 0, k.lib.eve_last_error()
    got = {}
    for name, width in (('head_R', 9), ('head_t', 3), ('reproj_rms', 1)):
        a = bufs[name].cpu().numpy()
        assert (a[N * width:] == SENTINEL).all(), 'guard of %s overwritten' % name
        got[name] = a[:N * width].reshape(want[name].shape)
    v = valid.cpu().numpy()
    assert (v[N:] == SENTINEL8).all() and (state[S * 13:].cpu().numpy() == SENTINEL).all()
    got['valid'] = v[:N].reshape(S, T)
    same(got, want)


def test_chunks_through_the_state_equal_one_call():
    lm, rig, want, want_state = shared(6, True)
    state = torch.zeros((S, 13), dtype=torch.float64, device='cuda')
    a = solve(lm[:, :2], rig, state=state)
    assert (state[:, 12] == 1).all()
    b = solve(lm[:, 2:], rig, state=state)
    same({k_: np.concatenate([a[k_], b[k_]], axis=1) for k_ in a}, want)
    assert np.array_equal(a['reproj_rms'], want['reproj_rms'][:, :2]) or ulps(a['reproj_rms'], want['reproj_rms'][:, :2]) <= 1
    assert np.array_equal(state.cpu().numpy().view(np.uint64), want_state.view(np.uint64))
    one = torch.zeros((S, 13), dtype=torch.float64, device='cuda')
    c = solve(lm, rig, state=one)
    for k_ in c:                                                           # device against device: every bit, rms included
        assert np.array_equal(np.concatenate([a[k_], b[k_]], axis=1).view(np.uint8), c[k_].view(np.uint8)), k_
    assert torch.equal(one, state)


def test_frames_without_a_solution_and_lengths():
    """Per sequence another reason in frame 1 of 3 (a NaN landmark, three positive weights) or in every frame (collinear model
    points, fx = 0): valid False, the identity pose, and the frame after it starts cold -- outputs and the float64 state are the
    contract's bits.  Then lengths: a sequence with no frames keeps its carried pose untouched, a reset is still applied."""
    lm, rig = fr.sequences(4, 3, 6, seed=21, weights=True)
    lm, rig = lm.copy(), rig.copy()
    lm[0, 1, 2, 0] = np.nan
    lm[1, 1, 3:, 2] = 0.0
    line = np.stack([np.linspace(-60, 60, 6), np.linspace(-30, 30, 6), np.linspace(-12, 12, 6)], axis=-1).astype(np.float32)
    g = np.random.default_rng(5)
    R, t = fr.random_pose(g)
    rig[2, 12:] = line.reshape(-1)
    lm[2] = np.stack([fr.project(line, R, t, g=g, weights=np.ones(6)) for _ in range(3)])
    rig[3, 0] = 0.0
    want_state = np.zeros((4, 13))
    want = fr.solve(lm, rig, state=want_state)
    assert want['valid'].tolist() == [[1, 0, 1], [1, 0, 1], [0, 0, 0], [0, 0, 0]]
    clean = fr.solve(fr.sequences(4, 3, 6, seed=21, weights=True)[0], rig)
    assert (want['accepted'][:2, 2] > clean['accepted'][:2, 2]).all()          # the contract's frame 2 started cold
    state = torch.zeros((4, 13), dtype=torch.float64, device='cuda')
    got = solve(lm, rig, state=state)
    same(got, want)
    assert np.array_equal(state.cpu().numpy().view(np.uint64), want_state.view(np.uint64))
    eye = np.eye(3, dtype=np.float32)
    for s_, f in ((0, 1), (1, 1), (2, 0), (2, 2), (3, 1)):
        assert np.array_equal(got['head_R'][s_, f], eye) and not got['head_t'][s_, f].any() and got['reproj_rms'][s_, f] == 0
    assert state[2:, 12].tolist() == [0.0, 0.0] and state[:2, 12].tolist() == [1.0, 1.0]
    # lengths (clamped to 0..T) and resets
    lengths, reset = np.array([0, 2, 7, 0]), np.array([0, 0, 0, 1])
    carried = np.zeros((4, 13))
    carried[:, :9], carried[:, 9:12], carried[:, 12] = np.eye(3).reshape(-1), (1.0, 2.0, 600.0), 2.0
    want_state = carried.copy()
    want = fr.solve(lm, rig, lengths=lengths, state=want_state, reset=reset)
    state = torch.from_numpy(carried).cuda()
    got = solve(lm, rig, lengths=lengths, state=state, reset=reset)
    same(got, want)
    assert not got['valid'][0].any() and not got['valid'][1, 2] and got['valid'][1, 0]
    assert np.array_equal(state.cpu().numpy().view(np.uint64), want_state.view(np.uint64))
    assert np.array_equal(state[0].cpu().numpy(), carried[0]) and state[3].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0]


def test_normalize_rt_continues_from_the_solved_pose():
    """o, R, warp, valid bit for bit from the device's float32 head_R / head_t; h within one float32 ulp (asin / atan2), as for the
    pose form.  Frame (0, 1) has no solution: valid_in turns both of its eyes off."""
    k = default_kernels()
    lm, rig = fr.sequences(S, T, 7, seed=31, weights=True)
    lm = lm.copy()
    lm[0, 1, 0, 1] = np.inf
    lm_d, rig_d = torch.from_numpy(lm).cuda(), torch.from_numpy(rig).cuda()
    head_R, head_t, rms, solved = k.face_pose_solve(lm_d, rig_d)
    assert solved.sum() == S * T - 1 and not solved[0, 1]
    for hw in ((16, 24), (128, 128)):
        for valid_in in (solved, None):
            o, R, warp, h, valid = k.eye_pose_normalize_rt(rig_d, head_R, head_t, valid_in, hw)
            assert k.lib.eve_last_kernel() == b'eye_pose_normalize_rt_kernel'
            want = fr.normalize_rt(rig, head_R.cpu().numpy(), head_t.cpu().numpy(), None if valid_in is None else solved.cpu().numpy(), hw)
            assert np.array_equal(valid.cpu().numpy(), want['valid'])
            assert bool(valid.view(2, S, T)[:, 0, 1].any()) == (valid_in is None) and valid.sum() >= 2 * (S * T - 1)
            for name, t in (('o', o), ('R', R), ('warp', warp)):
                g, w = t.cpu().numpy().view(np.uint32), want[name].view(np.uint32)
                assert np.array_equal(g, w), (name, hw, int((g != w).sum()))
            assert ulps(h.cpu().numpy(), want['h']) <= 1
    with pytest.raises(TypeError, match='head_t'):
        k.eye_pose_normalize_rt(rig_d, head_R, head_t[:, :1].contiguous(), None, (16, 24))
    with pytest.raises(TypeError, match='rows'):
        k.eye_pose_normalize_rt(rig_d[:, :11].contiguous(), head_R, head_t, None, (16, 24))


def test_refused_requests_launch_nothing():
    k = default_kernels()
    k.stream_state_rows(torch.zeros((2, 8), device='cuda'), torch.zeros((2, 8), device='cuda'))     # the last named launch
    before = k.lib.eve_last_kernel()
    assert b'pose' not in before
    lm, rig, _, _ = shared(6, True)
    lm_d, rig_d = torch.from_numpy(np.array(lm)).cuda(), torch.from_numpy(np.array(rig)).cuda()
    outs = [torch.full((S * T * 9,), SENTINEL, device='cuda') for _ in range(3)] + [torch.full((S * T,), SENTINEL8, dtype=torch.uint8, device='cuda')]
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(S_=S, T_=T, L=6, C=3, lm_=ptr(lm_d), rig_=ptr(rig_d), o=None):
        return k.lib.eve_face_pose_solve(S_, T_, L, C, lm_, rig_, None, None, None, *(o or [ptr(t) for t in outs]), s)

    for kw, word in ((dict(S_=0), 'bad arguments'), (dict(T_=0), 'bad arguments'), (dict(L=3), '4..68'), (dict(L=69), '4..68'),
                     (dict(C=4), '2 or 3 columns'), (dict(S_=1 << 30, T_=2), '31 bits'), (dict(lm_=None), 'bad arguments'),
                     (dict(rig_=None), 'bad arguments')):
        assert call(**kw) != 0
        msg = k.lib.eve_last_error().decode()
        assert msg.startswith('face_pose_solve:') and word in msg and k.lib.eve_last_kernel() == before, msg
    for i in range(4):
        o = [ptr(t) for t in outs]
        o[i] = None
        assert call(o=o) != 0 and k.lib.eve_last_kernel() == before, i
    rt = lambda **kw: k.lib.eve_eye_pose_normalize_rt(*[kw.get(n, v) for n, v in (
        ('N', S * T), ('per', T), ('rows', ptr(rig_d)), ('stride', 30), ('R', ptr(outs[0])), ('t', ptr(outs[1])), ('vin', None), ('OH', 16),
        ('OW', 24), ('o0', ptr(outs[0])), ('o1', ptr(outs[0])), ('o2', ptr(outs[0])), ('o3', ptr(outs[0])), ('o4', ptr(outs[3])))], s)
    for kw, word in ((dict(N=0), 'bad arguments'), (dict(per=0), 'bad arguments'), (dict(stride=11), 'at least 12'), (dict(OH=4097), 'too large'),
                     (dict(N=1 << 30), '31 bits'), (dict(rows=None), 'bad arguments'), (dict(o3=None), 'bad arguments')):
        assert rt(**kw) != 0
        msg = k.lib.eve_last_error().decode()
        assert msg.startswith('eye_pose_normalize_rt:') and word in msg and k.lib.eve_last_kernel() == before, msg
    torch.cuda.synchronize()
    assert all((t.cpu() == (SENTINEL8 if t.dtype == torch.uint8 else SENTINEL)).all() for t in outs)
    for bad in (lm_d.double(), lm_d[..., :1].contiguous(), lm_d.view(S * T, 6, 3), np.array(lm)):
        with pytest.raises(TypeError, match='landmarks'):
            k.face_pose_solve(bad, rig_d)
    for kw, word in ((dict(rig=rig_d[:, :-1].contiguous()), 'rig'), (dict(lengths=torch.zeros(S, device='cuda')), 'lengths'),
                     (dict(state=torch.zeros((S, 13), device='cuda')), 'state'), (dict(reset=torch.zeros(S + 1, dtype=torch.int32, device='cuda')), 'reset')):
        with pytest.raises(TypeError, match=word):
            k.face_pose_solve(lm_d, **dict(dict(rig=rig_d), **kw))
    with pytest.raises(RuntimeError):
        k.face_pose_solve(lm_d.cpu(), rig_d.cpu())
    with pytest.raises(RuntimeError):
        k.face_pose_solve(lm_d[:, :, :, :2], rig_d)
    assert k.lib.eve_last_kernel() == before
    assert call() == 0 and k.lib.eve_last_kernel() == b'face_pose_solve_kernel'             # the same call with sound arguments


# ------------------------------------------------------------------------------------------------ EVEStream
def face_chunks(B, Tn, seed, L=7, invalid=()):
    """Frontal heads in front of the CAM-sized frames' camera, noise scaled with its focal length -> (landmarks [B, Tn, L, 3], rig
    [B, 12 + 3L]) on the GPU; the (b, t) listed get a NaN."""
    lm, rig = fr.sequences(B, Tn, L, seed, weights=True, K=CAM_K, frontal=True, focal_norm=600.0, step_deg=2.0, step_mm=4.0, noise=0.1)
    lm = lm.copy()
    for b, t in invalid:
        lm[b, t, 1, 1] = np.nan
    return torch.from_numpy(lm).cuda(), torch.from_numpy(rig).cuda()


def warp_form(chunk, sol, rig):
    """The warp form of a face-landmark chunk from a solve's outputs -> (the batch, pose_valid)."""
    k = default_kernels()
    B, Tc = sol['head_R'].shape[:2]
    o, R, warp, h, valid = k.eye_pose_normalize_rt(rig, sol['head_R'].contiguous(), sol['head_t'].contiguous(),
                                                   sol['valid'].to(torch.uint8).contiguous(), data.eye_patch_hw())
    d = {k_: v for k_, v in chunk.items() if k_ not in ('face_landmarks', 'face_rig')}
    d['head_R'] = sol['head_R'].contiguous()
    for e, side in enumerate(('left', 'right')):
        d.update({side + '_o': o[e].view(B, Tc, 3), side + '_R': R[e].view(B, Tc, 3, 3), side + '_eye_warp': warp[e].view(B, Tc, 3, 3),
                  side + '_h': h[e].view(B, Tc, 2)})
    return d, valid.view(2, B, Tc).permute(1, 2, 0) != 0


def rest_of_clip(B, Tn, seed):
    _, d, _ = gpu_clip(B, Tn, seed=seed)
    return {k_: v for k_, v in d.items() if k_ not in ('left_eye_patch', 'right_eye_patch', 'left_h', 'right_h', 'left_o', 'right_o',
                                                      'left_R', 'right_R', 'head_R')}


def test_stream_steps_equal_the_warp_form_of_one_solve():
    """B = 2, Tc = 2, float32: two consecutive steps, stream 1 reset in between, graph and eager, against the warp form of ONE
    four-frame solve for stream 0 (the carried pose) and of a cold solve of frames 2..3 for stream 1 (the reset) -- every result
    key bit for bit, the second step a REPLAY of the first one's graph."""
    model, _ = make_model()
    B, Tn = 2, 4
    rest = rest_of_clip(B, Tn, seed=5)
    frames = torch.randint(0, 256, (B, Tn) + CAM + (3,), generator=torch.Generator().manual_seed(6), dtype=torch.uint8).cuda()
    lm, rig = face_chunks(B, Tn, seed=7)
    face = dict(rest, camera_frame=frames, face_landmarks=lm)
    ch = lambda src, i: dict({k_: v[:, 2 * i:2 * i + 2].contiguous() for k_, v in src.items()}, face_rig=rig)
    whole = data.solve_head_pose(lm, rig)
    tail1 = data.solve_head_pose(lm[1:, 2:].contiguous(), rig[1:])
    sols = [{k_: v[:, :2] for k_, v in whole.items()}, {k_: torch.cat([v[:1, 2:], tail1[k_]]) for k_, v in whole.items()}]
    assert whole['valid'].all() and tail1['valid'].all()
    g, e, w = eve_amd.EVEStream(model, B), eve_amd.EVEStream(model, B, use_graph=False), eve_amd.EVEStream(model, B, use_graph=False)
    for i in range(2):
        if i == 1:
            for st in (g, e, w):
                st.reset([1])
        og = {k_: v.clone() for k_, v in g.step(ch(face, i), return_heatmaps=True).items()}
        oe = e.step(ch(face, i), return_heatmaps=True)
        wf, valid = warp_form(ch(face, i), sols[i], rig)
        ow = w.step(wf, return_heatmaps=True)
        assert set(og) == set(oe) == set(ow) | {'pose_valid', 'head_t', 'face_reproj_rms'} and 'PoG_px_final' in ow
        for o in (og, oe):
            assert torch.equal(o['pose_valid'], valid) and torch.equal(o['head_t'], sols[i]['head_t']), i
            assert torch.equal(o['face_reproj_rms'], sols[i]['reproj_rms']), i
            for k_ in ow:
                assert torch.equal(o[k_], ow[k_]), (i, k_)
                assert torch.isfinite(o[k_].float()).all(), (i, k_)
    assert len(g._graphs) == 1
    for x, y in zip(g.get_head_pose(), e.get_head_pose()):
        assert torch.equal(x, y)
    R, t, has = g.get_head_pose()
    assert has.all() and torch.equal(t.float(), sols[1]['head_t'][:, -1]) and torch.equal(R.float(), sols[1]['head_R'][:, -1])
    assert set(g.get_state()) == set(w.get_state())


def test_stream_step_with_nv12_lengths_and_skipped_frames():
    """camera_frame_nv12, lengths = [2, 1] and skip_invalid_pose=True on a chunk whose frame (0, 1) has a NaN landmark: the step
    equals the warp-form step masked by the pose_valid the solve reports, graph and eager."""
    model, _ = make_model()
    B, Tc = 2, 2
    rest = rest_of_clip(B, Tc, seed=8)
    nv12 = torch.randint(0, 256, (B, Tc, CAM[0] * 3 // 2, CAM[1]), generator=torch.Generator().manual_seed(9), dtype=torch.uint8).cuda()
    lm, rig = face_chunks(B, Tc, seed=10, invalid=[(0, 1)])
    face = dict(rest, camera_frame_nv12=nv12, face_landmarks=lm, face_rig=rig)
    lengths = [2, 1]
    sol = data.solve_head_pose(lm, rig, lengths=lengths)
    assert sol['valid'].tolist() == [[True, False], [True, False]]
    wf, valid = warp_form(face, sol, rig)
    w = eve_amd.EVEStream(model, B, use_graph=False)
    ow = w.step(wf, lengths=lengths, eye_mask=valid)
    for use_graph in (True, False):
        st = eve_amd.EVEStream(model, B, use_graph=use_graph)
        o = st.step(face, lengths=lengths, skip_invalid_pose=True)
        assert set(o) == set(ow) | {'pose_valid', 'head_t', 'face_reproj_rms'} and torch.equal(o['pose_valid'], valid)
        assert o['valid'].tolist() == [[True, False], [True, False]]
        for k_ in ow:
            assert torch.equal(o[k_], ow[k_]), (use_graph, k_)
        assert st.get_head_pose()[2].tolist() == [False, True]            # stream 0's last solved frame had no solution
        sa, sb = st.get_state(), w.get_state()
        for key in sb:
            for x, y in zip(sa[key] if isinstance(sa[key], tuple) else (sa[key],), sb[key] if isinstance(sb[key], tuple) else (sb[key],)):
                assert torch.equal(x, y), key
