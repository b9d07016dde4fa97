"""GPU: eve_face_pose_solve_ex and eve_undistort_points (csrc/face_pose.hip) against their contract in numpy
(tests/face_pose_raw_ref.py) bit for bit -- head_R, head_t, reproj_rms, valid, inliers and the carried float64 state; the
normalised points and ok -- and face_landmarks_raw + camera_lens + face_huber_px through EVEStream, eager and under graph replay,
against the warp form fed one solve.  Shapes S = 3, T = 3."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import eve_amd
from eve_amd import data
from eve_amd.kernels import default_kernels
import eye_warp_lens_ref as lref
import face_pose_raw_ref as rr
import face_pose_ref as fr
from test_gpu_eye_pose import ptr, ulps
from test_gpu_face_pose import CAM, CAM_K, face_chunks, rest_of_clip
from test_gpu_stream import make_model

pytestmark = pytest.mark.gpu
S, T = 3, 3
GUARD = 64
SENTINEL, SENTINEL8 = -7.0, 0x5A
HUBER = 3.0
MODES = {'lens': (True, None), 'huber': (False, HUBER), 'both': (True, HUBER)}
FAR = 20000.0                 # a raw u no lens of the tests maps anything to: Newton gives up after its 12 steps
OUT = ('head_R', 'head_t', 'reproj_rms', 'valid', 'inliers')


@functools.lru_cache(maxsize=None)
def shared(L, mode, weights):
    """The landmarks, the rig, the lens rows and the contract's answer (with its final state), computed once -> read only.  With
    the loss and L >= 64, frames (0, 1) and (2, 2) are contaminated (5 landmarks moved by 40 and 55 px); with a lens, frames (1, 1)
    and (1, 2) hold a point that cannot be undistorted -- the last landmark (a lane's second point for L > 64) and landmark 2."""
    use_lens, k = MODES[mode]
    raw, rig, lens, lm = rr.raw_sequences(S, T, L, seed=50 + L, weights=weights)
    pts = (raw if use_lens else lm).copy()
    if k is not None and L >= 64:
        pts[0, 1, 3:8, 0] += 40.0
        pts[2, 2, 10:15, 1] -= 55.0
    if use_lens:
        pts[1, 1, L - 1, 0] = FAR
        pts[1, 2, 2, 0] = FAR
    state = np.zeros((S, 13))
    want = rr.solve(pts, rig, lens if use_lens else None, k, state=state)
    for a in (pts, rig, lens, state) + tuple(want.values()):
        a.setflags(write=False)
    return pts, rig, (lens if use_lens else None), k, want, state


def solve_ex(lm, rig, lens=None, huber=None, lengths=None, state=None, reset=None, name=b'face_pose_solve_ex_kernel'):
    """HipKernels.face_pose_solve_ex on numpy arrays -> dict of numpy outputs (state, a cuda tensor, is updated in place)."""
    k = default_kernels()
    dev = lambda a, dtype: None if a is None else torch.as_tensor(np.asarray(a), dtype=dtype).cuda()
    out = k.face_pose_solve_ex(torch.from_numpy(np.array(lm)).cuda(), torch.from_numpy(np.array(rig)).cuda(),
                               None if lens is None else torch.from_numpy(np.array(lens)).cuda(), huber, dev(lengths, torch.int32), state,
                               dev(reset, torch.int32))
    assert k.lib.eve_last_kernel() == name
    return dict(zip(OUT, (t.cpu().numpy() for t in out)))


def same(got, want, what=''):
    assert np.array_equal(got['valid'], want['valid']), (what, got['valid'], want['valid'])
    assert np.array_equal(got['inliers'], want['inliers']), (what, got['inliers'], want['inliers'])
    print(what, 'reproj_rms ulps', ulps(got['reproj_rms'], want['reproj_rms']))
    for name in ('head_R', 'head_t', 'reproj_rms'):
        g, w = got[name].view(np.uint32), want[name].view(np.uint32)
        assert np.array_equal(g, w), '%s %s: %d of %d elements differ, first at %s' % (what, name, int((g != w).sum()), g.size, np.argwhere(g != w)[0])


# ------------------------------------------------------------------------------------------------ 1. the kernel against its contract
@pytest.mark.parametrize('weights', [False, True], ids=['uv', 'uvw'])
@pytest.mark.parametrize('mode', sorted(MODES))
@pytest.mark.parametrize('L', [6, 64, 65, 68])
def test_kernel_equals_the_contract_bit_for_bit(L, mode, weights):
    pts, rig, lens, k, want, want_state = shared(L, mode, weights)
    assert pts.shape == (S, T, L, 3 if weights else 2)
    if L >= 64:
        assert want['valid'].all()
        if lens is not None:                                             # the point that cannot be undistorted was dropped, no more
            assert k is not None or (want['inliers'] == np.where(np.arange(S * T).reshape(S, T) // T == 1, [L, L - 1, L - 1], L)).all()
        if k is not None:                                                # the contaminated frames lost at least the moved landmarks
            assert want['inliers'][0, 1] <= L - 5 and want['inliers'][2, 2] <= L - 5 and want['inliers'].min() >= L - 12
    else:
        assert want['valid'].sum() >= S * T - 2
    state = torch.zeros((S, 13), dtype=torch.float64, device='cuda')
    got = solve_ex(pts, rig, lens, k, state=state)
    same(got, want, 'L = %d %s' % (L, mode))
    assert np.array_equal(state.cpu().numpy().view(np.uint64), want_state.view(np.uint64))
    same(solve_ex(pts, rig, lens, k), want, 'without a state')


# ------------------------------------------------------------------------------------------------ 2., 3. the reductions
@pytest.mark.parametrize('L,weights', [(6, False), (65, True), (68, True)])
def test_no_lens_and_no_loss_equals_the_plain_entry_bit_for_bit(L, weights):
    k = default_kernels()
    lm, rig = fr.sequences(S, T, L, seed=10 + L, weights=weights)
    lm_d, rig_d = torch.from_numpy(lm).cuda(), torch.from_numpy(rig).cuda()
    sa, sb, sc = (torch.zeros((S, 13), dtype=torch.float64, device='cuda') for _ in range(3))
    plain = k.face_pose_solve(lm_d, rig_d, state=sa)
    assert k.lib.eve_last_kernel() == b'face_pose_solve_kernel'
    ex = k.face_pose_solve_ex(lm_d, rig_d, state=sb)
    assert k.lib.eve_last_kernel() == b'face_pose_solve_ex_kernel'
    for a, b in zip(plain, ex[:4]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert torch.equal(sa, sb) and plain[3].all()
    assert (ex[4] == L).all()
    # zero-coefficient lens rows whose intrinsics are the rig's: face_landmarks' bits
    zero = torch.from_numpy(np.broadcast_to(rr.lens_row(()), (S, T, 12)).copy()).cuda()
    zl = k.face_pose_solve_ex(lm_d, rig_d, zero, state=sc)
    for a, b in zip(plain, zl[:4]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert torch.equal(sa, sc) and torch.equal(zl[4], ex[4])
    same(dict(zip(OUT, (t.cpu().numpy() for t in zl))), rr.solve(lm, rig), 'zero rows')


# ------------------------------------------------------------------------------------------------ 4. eve_undistort_points
def raw_points(N, seed):
    """N float32 raw pixels of the issue's field, seen through the lens each gets -> (points [N, 2], per-point rows [N, 12]); among
    the rows a zero-coefficient one, one with a NaN and one with fx = 0; among the points a NaN and one no lens maps anything to."""
    g = np.random.default_rng(seed)
    rows = [rr.LENSES[n] for n in sorted(rr.LENSES)] + [rr.lens_row(())]
    per = np.stack([rows[i % len(rows)] for i in range(N)])
    u, v = 640.0 + 1000.0 * g.uniform(-0.64, 0.64, N), 360.0 + 1000.0 * g.uniform(-0.36, 0.36, N)
    pts = np.zeros((N, 2), dtype=np.float32)
    for i in range(N):
        ud, vd, _ = lref.distort(u[i], v[i], per[i])
        pts[i] = ud, vd
    if N > 40:
        per[7, 5], per[12, 0], pts[20, 1], pts[33, 0] = np.nan, 0.0, np.nan, FAR
    return pts, per


@pytest.mark.parametrize('N', [1, 63, 65, 130])
def test_undistort_points_equals_the_contract_bit_for_bit(N):
    k = default_kernels()
    pts, per = raw_points(N, seed=N)
    for lens in (per, rr.LENSES['rational8'][None], rr.LENSES['barrel5'][None]):
        want_xy, want_ok = rr.undistort_points(pts, lens)
        xy, ok = k.undistort_points(torch.from_numpy(pts).cuda(), torch.from_numpy(lens).cuda())
        assert k.lib.eve_last_kernel() == b'undistort_points_kernel'
        assert xy.dtype == torch.float64 and tuple(xy.shape) == (N, 2) and ok.dtype == torch.uint8
        assert np.array_equal(ok.cpu().numpy(), want_ok)
        g, w = xy.cpu().numpy().view(np.uint64), want_xy.view(np.uint64)
        assert np.array_equal(g, w), '%d of %d differ, first at %s' % (int((g != w).sum()), g.size, np.argwhere(g != w)[0])
        if N > 40 and lens.shape[0] == N:
            assert want_ok.sum() == N - 4 and not want_ok[[7, 12, 20, 33]].any()
    got, good = data.undistort_points(torch.from_numpy(pts).cuda(), torch.from_numpy(per).cuda())
    want_xy, want_ok = rr.undistort_points(pts, per)
    p64 = per.astype(np.float64)
    want = np.where(want_ok[:, None] != 0, np.stack([p64[:, 0] * want_xy[:, 0] + p64[:, 2], p64[:, 1] * want_xy[:, 1] + p64[:, 3]], axis=-1), 0.0)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(good.cpu().numpy(), want_ok != 0)


# ------------------------------------------------------------------------------------------------ 5. guards
def test_raw_launches_stay_inside_their_buffers():
    k = default_kernels()
    pts, rig, lens, hub, want, _ = shared(68, 'both', True)
    N = S * T
    bufs = {name: torch.full((N * width + GUARD,), SENTINEL, dtype=torch.float32, device='cuda') for name, width in
            (('head_R', 9), ('head_t', 3), ('reproj_rms', 1))}
    valid, inliers = (torch.full((N + GUARD,), SENTINEL8, dtype=torch.uint8, device='cuda') for _ in range(2))
    state = torch.full((S * 13 + GUARD,), SENTINEL, dtype=torch.float64, device='cuda')
    state[:S * 13] = 0
    lm_d, rig_d, lens_d = (torch.from_numpy(np.array(a)).cuda() for a in (pts, rig, lens))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    status = k.lib.eve_face_pose_solve_ex(S, T, 68, 3, ptr(lm_d), ptr(rig_d), ptr(lens_d), HUBER, None, ptr(state), None, ptr(bufs['head_R']),
                                          ptr(bufs['head_t']), ptr(bufs['reproj_rms']), ptr(valid), ptr(inliers), stream)
    assert status == 0, k.lib.eve_last_error()
    got = {}
    for name, width in (('head_R', 9), ('head_t', 3), ('reproj_rms', 1)):
        a = bufs[name].cpu().numpy()
        assert (a[N * width:] == SENTINEL).all(), 'guard of %s overwritten' % name
        got[name] = a[:N * width].reshape(want[name].shape)
    for name, t in (('valid', valid), ('inliers', inliers)):
        v = t.cpu().numpy()
        assert (v[N:] == SENTINEL8).all(), 'guard of %s overwritten' % name
        got[name] = v[:N].reshape(S, T)
    assert (state[S * 13:].cpu().numpy() == SENTINEL).all()
    same(got, want)
    # eve_undistort_points, N = 65: the second block's one thread
    n = 65
    p, per = raw_points(n, seed=3)
    xy = torch.full((2 * n + GUARD,), SENTINEL, dtype=torch.float64, device='cuda')
    ok = torch.full((n + GUARD,), SENTINEL8, dtype=torch.uint8, device='cuda')
    p_d, per_d = torch.from_numpy(p).cuda(), torch.from_numpy(per).cuda()
    assert k.lib.eve_undistort_points(n, ptr(p_d), ptr(per_d), 12, ptr(xy), ptr(ok), stream) == 0, k.lib.eve_last_error()
    want_xy, want_ok = rr.undistort_points(p, per)
    assert (xy[2 * n:].cpu().numpy() == SENTINEL).all() and (ok[n:].cpu().numpy() == SENTINEL8).all()
    assert np.array_equal(xy[:2 * n].cpu().numpy().view(np.uint64), want_xy.reshape(-1).view(np.uint64))
    assert np.array_equal(ok[:n].cpu().numpy(), want_ok)


# ------------------------------------------------------------------------------------------------ 6. the state
def test_chunks_lengths_and_resets_behave_as_in_the_plain_form():
    pts, rig, lens, hub, want, want_state = shared(65, 'both', True)
    state = torch.zeros((S, 13), dtype=torch.float64, device='cuda')
    a = solve_ex(pts[:, :1], rig, lens[:, :1], hub, state=state)
    assert (state[:, 12] == 1).all()
    b = solve_ex(pts[:, 1:], rig, lens[:, 1:], hub, state=state)
    same({k_: np.concatenate([a[k_], b[k_]], axis=1) for k_ in a}, want, 'chunks')
    assert np.array_equal(state.cpu().numpy().view(np.uint64), want_state.view(np.uint64))
    # lengths (clamped to 0..T) and resets: a sequence with no frames keeps its carried pose, a reset is still applied
    lengths, reset = np.array([0, 2, 7]), np.array([0, 1, 0])
    carried = np.array(want_state)
    carried[0, 12] = 2.0
    ws = carried.copy()
    w2 = rr.solve(pts, rig, lens, hub, lengths=lengths, state=ws, reset=reset)
    st = torch.from_numpy(carried).cuda()
    g2 = solve_ex(pts, rig, lens, hub, lengths=lengths, state=st, reset=reset)
    same(g2, w2, 'lengths')
    assert not g2['valid'][0].any() and not g2['inliers'][0].any() and not g2['valid'][1, 2] and g2['valid'][1, 0]
    assert np.array_equal(st.cpu().numpy().view(np.uint64), ws.view(np.uint64)) and np.array_equal(st[0].cpu().numpy(), carried[0])
    # a lens row that is not usable: the frame is invalid, the next one starts cold -- the contract's bits
    bad = np.array(lens)
    bad[2, 1, 9] = np.nan
    bad[0, 0, 1] = 0.0
    ws = np.zeros((S, 13))
    w3 = rr.solve(pts, rig, bad, hub, state=ws)
    st = torch.zeros((S, 13), dtype=torch.float64, device='cuda')
    g3 = solve_ex(pts, rig, bad, hub, state=st)
    same(g3, w3, 'bad rows')
    assert not g3['valid'][2, 1] and not g3['valid'][0, 0] and g3['valid'].sum() == S * T - 2
    assert np.array_equal(st.cpu().numpy().view(np.uint64), ws.view(np.uint64))


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refused_requests_launch_nothing():
    k = default_kernels()
    k.stream_state_rows(torch.zeros((2, 8), device='cuda'), torch.zeros((2, 8), device='cuda'))     # the last named launch
    before = k.lib.eve_last_kernel()
    assert b'pose' not in before and b'undistort' not in before
    pts, rig, lens, hub, _, _ = shared(6, 'both', True)
    lm_d, rig_d, lens_d = (torch.from_numpy(np.array(a)).cuda() for a in (pts, rig, lens))
    outs = [torch.full((S * T * 9,), SENTINEL, device='cuda') for _ in range(3)] + [torch.full((S * T,), SENTINEL8, dtype=torch.uint8, device='cuda')
                                                                                     for _ in range(2)]
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(S_=S, T_=T, L=6, C=3, lm_=ptr(lm_d), rig_=ptr(rig_d), huber=HUBER, o=None):
        return k.lib.eve_face_pose_solve_ex(S_, T_, L, C, lm_, rig_, ptr(lens_d), huber, None, None, None, *(o or [ptr(t) for t in outs]), s)

    for kw, word in ((dict(S_=0), 'bad arguments'), (dict(T_=0), 'bad arguments'), (dict(L=3), '4..68'), (dict(L=69), '4..68'),
                     (dict(C=4), '2 or 3 columns'), (dict(S_=1 << 30, T_=2), '31 bits'), (dict(lm_=None), 'bad arguments'),
                     (dict(rig_=None), 'bad arguments'), (dict(huber=float('nan')), 'huber_px')):
        assert call(**kw) != 0
        msg = k.lib.eve_last_error().decode()
        assert msg.startswith('face_pose_solve_ex:') and word in msg and k.lib.eve_last_kernel() == before, msg
    for i in range(5):
        o = [ptr(t) for t in outs]
        o[i] = None
        assert call(o=o) != 0 and k.lib.eve_last_kernel() == before, i
    p_d = torch.zeros((4, 2), device='cuda')
    xy, ok = torch.full((8,), SENTINEL, dtype=torch.float64, device='cuda'), torch.full((4,), SENTINEL8, dtype=torch.uint8, device='cuda')
    und = lambda N=4, p=ptr(p_d), l=ptr(lens_d), stride=12, x=ptr(xy), o=ptr(ok): k.lib.eve_undistort_points(N, p, l, stride, x, o, s)
    for kw, word in ((dict(N=0), 'bad arguments'), (dict(p=None), 'bad arguments'), (dict(l=None), 'bad arguments'), (dict(x=None), 'bad arguments'),
                     (dict(o=None), 'bad arguments'), (dict(stride=5), 'lens_stride')):
        assert und(**kw) != 0
        msg = k.lib.eve_last_error().decode()
        assert msg.startswith('undistort_points:') and word in msg and k.lib.eve_last_kernel() == before, msg
    torch.cuda.synchronize()
    assert all((t.cpu() == (SENTINEL8 if t.dtype == torch.uint8 else SENTINEL)).all() for t in outs + [xy, ok])
    for bad in (lm_d.double(), lm_d[..., :1].contiguous(), np.array(pts)):
        with pytest.raises(TypeError, match='landmarks'):
            k.face_pose_solve_ex(bad, rig_d, lens_d, HUBER)
    for kw, word in ((dict(rig=rig_d[:, :-1].contiguous()), 'rig'), (dict(lens=lens_d.view(S * T, 12)), 'lens'), (dict(lens=lens_d.double()), 'lens'),
                     (dict(lengths=torch.zeros(S, device='cuda')), 'lengths'), (dict(state=torch.zeros((S, 13), device='cuda')), 'state'),
                     (dict(reset=torch.zeros(S + 1, dtype=torch.int32, device='cuda')), 'reset')):
        with pytest.raises(TypeError, match=word):
            k.face_pose_solve_ex(lm_d, **dict(dict(rig=rig_d, lens=lens_d), **kw))
    for bad in (0, -3.0, float('nan'), float('inf'), '3'):
        with pytest.raises(ValueError, match='huber_px'):
            k.face_pose_solve_ex(lm_d, rig_d, lens_d, bad)
    with pytest.raises(RuntimeError):
        k.face_pose_solve_ex(lm_d, rig_d, lens_d[:, :, :].transpose(0, 1).contiguous().transpose(0, 1))
    for bad_p, bad_l in ((p_d.double(), lens_d[0]), (p_d.view(2, 4), lens_d[0]), (p_d, lens_d[0, :2]), (p_d[:0], lens_d[0, :1])):
        with pytest.raises(TypeError):
            k.undistort_points(bad_p, bad_l)
    assert k.lib.eve_last_kernel() == before
    assert call() == 0 and k.lib.eve_last_kernel() == b'face_pose_solve_ex_kernel'         # the same call with sound arguments
    assert und() == 0 and k.lib.eve_last_kernel() == b'undistort_points_kernel'


# ------------------------------------------------------------------------------------------------ 8. EVEStream
def warp_form(chunk, sol, rig):
    """The warp form of a raw face-landmark chunk (camera_lens stays: the warp undistorts the pixels) -> (the batch, pose_valid)."""
    k = default_kernels()
    B, Tc = sol['head_R'].shape[:2]
    o, R, warp, h, valid = k.eye_pose_normalize_rt(rig, sol['head_R'].contiguous(), sol['head_t'].contiguous(),
                                                   sol['valid'].to(torch.uint8).contiguous(), data.eye_patch_hw())
    d = {k_: v for k_, v in chunk.items() if k_ not in ('face_landmarks_raw', 'face_rig')}
    d['head_R'] = sol['head_R'].contiguous()
    for e, side in enumerate(('left', 'right')):
        d.update({side + '_o': o[e].view(B, Tc, 3), side + '_R': R[e].view(B, Tc, 3, 3), side + '_eye_warp': warp[e].view(B, Tc, 3, 3),
                  side + '_h': h[e].view(B, Tc, 2)})
    return d, valid.view(2, B, Tc).permute(1, 2, 0) != 0


def test_stream_steps_equal_the_warp_form_of_one_solve():
    """B = 2, Tc = 2, float32: two consecutive steps with face_landmarks_raw + camera_lens and face_huber_px = 3, stream 1 reset in
    between, graph and eager, against the warp form of ONE four-frame solve for stream 0 (the carried pose) and of a cold solve of
    frames 2..3 for stream 1 -- a solve that is the contract's, bit for bit; every result key bit for bit, the second step a REPLAY
    of the first one's graph.  Then the attribute is cleared: a new graph, and the pose of the solve without the loss."""
    model, _ = make_model()
    B, Tn, L = 2, 4, 68
    rest = rest_of_clip(B, Tn, seed=5)
    frames = torch.randint(0, 256, (B, Tn) + CAM + (3,), generator=torch.Generator().manual_seed(6), dtype=torch.uint8).cuda()
    lm, rig = face_chunks(B, Tn, seed=7, L=L)
    row = rr.lens_row(rr.LENS_COEFFS['barrel5'], K=CAM_K)
    raw_np = rr.distort_landmarks(lm.cpu().numpy(), row)
    raw_np[0, 1, 4:9, :2] += (6.0, -5.0)                                   # five landmarks of frame (0, 1) are confidently wrong
    raw = torch.from_numpy(raw_np).cuda()
    lens = torch.from_numpy(np.broadcast_to(row, (B, Tn, 12)).copy()).cuda()
    face = dict(rest, camera_frame=frames, face_landmarks_raw=raw, camera_lens=lens)
    ch = lambda src, i: dict({k_: v[:, 2 * i:2 * i + 2].contiguous() for k_, v in src.items()}, face_rig=rig)
    whole = data.solve_head_pose(raw, rig, lens=lens, huber_px=HUBER)
    tail1 = data.solve_head_pose(raw[1:, 2:].contiguous(), rig[1:], lens=lens[1:, 2:].contiguous(), huber_px=HUBER)
    contract = rr.solve(raw_np, rig.cpu().numpy(), lens.cpu().numpy(), HUBER)
    for k_ in ('head_R', 'head_t', 'reproj_rms', 'inliers'):
        assert np.array_equal(whole[k_].cpu().numpy().view(np.uint8), contract[k_].view(np.uint8)), k_
    assert whole['valid'].all() and tail1['valid'].all() and whole['inliers'][0, 1] == L - 5 and whole['inliers'].min() >= L - 5
    sols = [{k_: v[:, :2] for k_, v in whole.items()}, {k_: torch.cat([v[:1, 2:], tail1[k_]]) for k_, v in whole.items()}]
    added = {'pose_valid', 'head_t', 'face_reproj_rms', 'face_inliers'}
    model.eye_net.face_huber_px = HUBER
    try:
        g, e, w = eve_amd.EVEStream(model, B), eve_amd.EVEStream(model, B, use_graph=False), eve_amd.EVEStream(model, B, use_graph=False)
        for i in range(2):
            if i == 1:
                for st in (g, e, w):
                    st.reset([1])
            og = {k_: v.clone() for k_, v in g.step(ch(face, i), return_heatmaps=True).items()}
            oe = e.step(ch(face, i), return_heatmaps=True)
            wf, valid = warp_form(ch(face, i), sols[i], rig)
            ow = w.step(wf, return_heatmaps=True)
            assert set(og) == set(oe) == set(ow) | added and 'PoG_px_final' in ow
            for o in (og, oe):
                assert torch.equal(o['pose_valid'], valid) and torch.equal(o['head_t'], sols[i]['head_t']), i
                assert torch.equal(o['face_reproj_rms'], sols[i]['reproj_rms']) and torch.equal(o['face_inliers'], sols[i]['inliers']), i
                for k_ in ow:
                    assert torch.equal(o[k_], ow[k_]), (i, k_)
                    assert torch.isfinite(o[k_].float()).all(), (i, k_)
        assert len(g._graphs) == 1
        for x, y in zip(g.get_head_pose(), e.get_head_pose()):
            assert torch.equal(x, y)
        R, t, has = g.get_head_pose()
        assert has.all() and torch.equal(t.float(), sols[1]['head_t'][:, -1]) and torch.equal(R.float(), sols[1]['head_R'][:, -1])
        # flipping the attribute re-captures: the lens-only solve from a cold start
        model.eye_net.face_huber_px = None
        for st in (g, e):
            st.reset()
        og, oe = g.step(ch(face, 0), return_heatmaps=True), e.step(ch(face, 0), return_heatmaps=True)
        lens_only = data.solve_head_pose(raw[:, :2].contiguous(), rig, lens=lens[:, :2].contiguous())
        assert len(g._graphs) == 2 and (lens_only['inliers'] == L).all()
        assert not torch.equal(lens_only['head_t'], sols[0]['head_t'])
        for o in (og, oe):
            assert torch.equal(o['head_t'], lens_only['head_t']) and torch.equal(o['face_inliers'], lens_only['inliers'])
        model.eye_net.face_huber_px = HUBER
        g.reset()
        assert torch.equal(g.step(ch(face, 0), return_heatmaps=True)['head_t'], sols[0]['head_t']) and len(g._graphs) == 2      # the first graph again
    finally:
        model.eye_net.face_huber_px = None
