"""GPU: the per-person gaze calibration -- eve_calib_append and eve_calib_fit against the numpy contract of tests/calib_ref.py, and
EVEStream's collect / fit / apply path around them (eager and captured).  Every test here needs the two entry points, so every one
fails on a library without them."""
import numpy as np
import pytest
import torch

import calib_ref
import eve_amd
from eve_amd import data
from eve_amd.eve import _fuse2, _mean2
from eve_amd.kernels import default_kernels
from test_gpu_stream import gpu_clip, make_model

pytestmark = pytest.mark.gpu
S, TC, C = 3, 5, 8
GUARD = 64
KAPPA_LEFT = np.array([np.deg2rad(2.5), np.deg2rad(-3.0)])
KAPPA_RIGHT = np.array([np.deg2rad(-1.5), np.deg2rad(2.0)])


def guarded(shape, dtype, sentinel):
    """-> (the whole buffer, its payload as a contiguous view): GUARD sentinel elements on either side of the payload."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device='cuda')
    return whole, whole[GUARD:GUARD + n].view(shape)


def guards_hold(whole, sentinel):
    return bool((whole[:GUARD] == sentinel).all()) and bool((whole[-GUARD:] == sentinel).all())


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------------- append
def test_append_matches_the_reference_in_frame_order():
    """Validity holes, ragged lengths with a 0, an eye masked out, a NaN target, a NaN head_R row, and a store that starts at 6 of
    8 and overflows.  Rows within 1e-12 * max(1, |reference|): double sin / cos are good to a couple of ulp and five chained 3 x 3
    products cost a few tens (about 100 x margin); a single float32 intermediate (6e-8) fails by four orders."""
    k = default_kernels()
    eyes = [calib_ref.make_scene(20 + e, S * TC, calib_ref.KAPPA_STAR) for e in range(2)]
    shared = eyes[0]
    head_R, inv_cam, ppm, target = (shared[n].copy() for n in ('head_R', 'inv_cam', 'ppm', 'target'))
    target[1] = np.nan                                   # stream 0, frame 1
    head_R[2 * TC + 0, 1, 2] = np.nan                    # stream 2, frame 0
    valid = np.ones((S, TC), dtype=np.uint8)
    valid[0, 3] = valid[2, 1] = 0
    lengths = np.array([5, 0, 4], dtype=np.int32)
    eye_valid = np.ones((S, TC, 2), dtype=np.uint8)
    eye_valid[2, :, 1] = 0                               # stream 2: the right eye is out
    eye_valid[0, 4, 1] = 0
    g = np.stack([e_['g'] for e_ in eyes]).reshape(2, S, TC, 2)
    origin = np.stack([e_['origin'] for e_ in eyes]).reshape(2, S, TC, 3)
    R = np.stack([e_['R'] for e_ in eyes]).reshape(2, S, TC, 3, 3)
    SENT, ISENT = -777.25, -7
    s_whole, samples = guarded((S, 2, C, 16), torch.float64, SENT)
    c_whole, count = guarded((S, 2), torch.int32, ISENT)
    d_whole, dropped = guarded((S, 2), torch.int32, ISENT)
    count.zero_()
    dropped.zero_()
    count[0, 0] = 6                                      # two free rows, three usable frames: the third is dropped
    k.calib_append(cuda(g), cuda(head_R.reshape(S, TC, 3, 3)), cuda(origin), cuda(R), cuda(inv_cam.reshape(S, TC, 4, 4)),
                   cuda(ppm.reshape(S, TC, 2)), cuda(target.reshape(S, TC, 2)), samples, count, dropped, cuda(valid), cuda(lengths),
                   cuda(eye_valid))
    torch.cuda.synchronize()
    want_rows = {(b, e): [] for b in range(S) for e in range(2)}
    for e in range(2):
        rows, usable = calib_ref.reduce(g[e].reshape(-1, 2), head_R, origin[e].reshape(-1, 3), R[e].reshape(-1, 3, 3), inv_cam, ppm, target)
        for b in range(S):
            for t in range(lengths[b]):
                if valid[b, t] and eye_valid[b, t, e] and usable[b * TC + t]:
                    want_rows[(b, e)].append(rows[b * TC + t])
    assert [len(want_rows[(0, e)]) for e in range(2)] == [3, 2] and len(want_rows[(2, 0)]) == 2 and not want_rows[(2, 1)] and not want_rows[(1, 0)]
    got, got_count, got_dropped = samples.cpu().numpy(), count.cpu().numpy(), dropped.cpu().numpy()
    for (b, e), rows in want_rows.items():
        start = 6 if (b, e) == (0, 0) else 0
        kept = min(len(rows), C - start)
        assert got_count[b, e] == start + kept and got_dropped[b, e] == len(rows) - kept, (b, e)
        for i in range(kept):
            ref = rows[i]
            assert (np.abs(got[b, e, start + i] - ref) <= 1e-12 * np.maximum(1.0, np.abs(ref))).all(), (b, e, i)
            assert got[b, e, start + i, 14] == 1.0 and got[b, e, start + i, 15] == 0.0
        untouched = np.ones(C, dtype=bool)
        untouched[start:start + kept] = False
        assert (got[b, e, untouched] == SENT).all(), (b, e)
    assert got_dropped[0, 0] == 1
    assert guards_hold(s_whole, SENT) and guards_hold(c_whole, ISENT) and guards_hold(d_whole, ISENT)


def test_calibration_samples_rows_line_up_with_their_frames():
    sc = calib_ref.make_scene(31, 7, calib_ref.KAPPA_STAR)
    sc['target'][2, 1] = np.nan
    rows, usable = calib_ref.reduce(sc['g'], sc['head_R'], sc['origin'], sc['R'], sc['inv_cam'], sc['ppm'], sc['target'])
    got = data.calibration_samples(cuda(sc['g']), cuda(sc['head_R']), cuda(sc['origin']), cuda(sc['R']), cuda(sc['inv_cam']), cuda(sc['ppm']),
                                   cuda(sc['target'])).cpu().numpy()
    assert usable.tolist() == [True, True, False, True, True, True, True] and (got[2] == 0.0).all()
    assert (np.abs(got[usable] - rows[usable]) <= 1e-12 * np.maximum(1.0, np.abs(rows[usable]))).all()
    fit = data.fit_gaze_offset(torch.from_numpy(got).cuda())
    assert bool(fit['ok']) and int(fit['used']) == 6 and np.abs(fit['kappa'].cpu().numpy() - calib_ref.KAPPA_STAR).max() < 5e-8


# ---------------------------------------------------------------------------------------------------------------- fit
def stores(row_sets, cap):
    """Row sets of different lengths -> (samples float64 [S, cap, 16] with garbage past each count, count int32 [S])."""
    s = np.full((len(row_sets), cap, 16), np.nan)
    for q, rows in enumerate(row_sets):
        s[q, :len(rows)] = rows
    return cuda(s), cuda(np.array([len(r) for r in row_sets], dtype=np.int32))


def test_fit_matches_the_reference_at_one_two_and_three_samples_per_lane():
    """n = 5, 64, 65, 130 noise-free samples.  The device kappa is within 1e-10 rad of the reference's: the reference's own kappa
    moves at most 3e-15 rad when its summation order is reversed (five orders of margin), and the float32 path that applies kappa
    resolves 1.2e-7 relative (three orders the other way).  The reference itself is within 5e-8 rad of kappa* (float32 target
    rounding: this judges the scene, not the kernel)."""
    ns = (5, 64, 65, 130)
    sets = [calib_ref.scene_rows(calib_ref.make_scene(100 + n, n, calib_ref.KAPPA_STAR)) for n in ns]
    samples, count = stores(sets, 130)
    k = default_kernels()
    kappa, rms, used, inliers, ok = (t.cpu().numpy() for t in k.calib_fit(samples, count))
    again = k.calib_fit(samples, count)
    for q, rows in enumerate(sets):
        ref = calib_ref.fit(rows)
        assert ref['ok'] and np.abs(ref['kappa'] - calib_ref.KAPPA_STAR).max() < 5e-8
        print('n = %d: device - reference %.3g rad, reference - kappa* %.3g rad' % (
            ns[q], np.abs(kappa[q] - ref['kappa']).max(), np.abs(ref['kappa'] - calib_ref.KAPPA_STAR).max()))
        assert ok[q] == 1 and used[q] == inliers[q] == ns[q] == ref['used']
        assert np.abs(kappa[q] - ref['kappa']).max() <= 1e-10
        assert abs(rms[q] - ref['rms_mm']) <= 1e-6     # 1e-10 rad over a lever of at most ~1500 mm / rad moves a residual 1.5e-7 mm
    for a, b in zip((kappa, rms, used, inliers, ok), again):     # two launches on one store: the same bits
        assert np.array_equal(a, b.cpu().numpy())


def test_fit_with_the_huber_loss_matches_the_reference():
    h = calib_ref.HUBER_SCENE
    rows = calib_ref.scene_rows(calib_ref.make_scene(2, h['n'], calib_ref.KAPPA_STAR, noise_mm=h['noise_mm'], outliers=h['outliers']))
    ref = calib_ref.fit(rows, huber_mm=h['huber_mm'])
    assert ref['ok'] and np.abs(ref['residuals'] - h['huber_mm']).min() > 1e-6      # one ulp cannot move a sample across the kink
    samples, count = stores([rows], h['n'])
    out = data.fit_gaze_offset(samples, count, huber_mm=h['huber_mm'])
    kappa = out['kappa'].cpu().numpy()[0]
    print('huber: device - reference %.3g rad' % np.abs(kappa - ref['kappa']).max())
    assert bool(out['ok'][0]) and int(out['used'][0]) == ref['used'] == h['n'] and int(out['inliers'][0]) == ref['inliers'] < h['n']
    assert np.abs(kappa - ref['kappa']).max() <= 1e-10
    assert abs(float(out['rms_mm'][0]) - ref['rms_mm']) <= 1e-6
    plain = data.fit_gaze_offset(samples, count)
    err = lambda kap: np.linalg.norm(kap - calib_ref.KAPPA_STAR)
    assert err(kappa) < 0.5 * err(plain['kappa'].cpu().numpy()[0])


def test_a_failed_fit_leaves_the_stored_kappa_alone():
    """4 samples, an empty store, targets generated at 0.5 rad, a singular system, a sequence not selected: ok False and the stored
    row and flag bit-unchanged; the one good sequence among them is written."""
    good = calib_ref.scene_rows(calib_ref.make_scene(8, 20, calib_ref.KAPPA_STAR))
    far = calib_ref.scene_rows(calib_ref.make_scene(7, 20, np.array([0.5, 0.0])))
    flat = good.copy()
    flat[:, [1, 4, 7]] = 0.0
    sets = [good[:4], good[:0], far, flat, good, good]
    for rows in sets[:4]:
        assert not calib_ref.fit(rows)['ok']
    samples, count = stores(sets, 20)
    select = cuda(np.array([1, 1, 1, 1, 1, 0], dtype=np.uint8))
    stored = torch.tensor([[0.011, -0.022], [0.0, 0.0], [0.033, 0.044], [-0.055, 0.066], [0.077, -0.088], [0.099, 0.0111]], device='cuda')
    flags = cuda(np.array([1, 0, 1, 1, 0, 1], dtype=np.uint8))
    before, flags_before = stored.clone(), flags.clone()
    kappa, rms, used, inliers, ok = default_kernels().calib_fit(samples, count, select, None, 5, stored, flags)
    assert ok.tolist() == [0, 0, 0, 0, 1, 0] and used.tolist() == [4, 0, 20, 20, 20, 0]
    keep = [0, 1, 2, 3, 5]
    assert torch.equal(stored[keep], before[keep]) and torch.equal(flags[keep], flags_before[keep])
    assert (kappa[keep] == 0).all() and (rms[keep] == 0).all() and (inliers[keep] == 0).all()
    ref = calib_ref.fit(good)
    assert torch.equal(stored[4], kappa[4].float()) and int(flags[4]) == 1
    assert np.abs(kappa[4].cpu().numpy() - ref['kappa']).max() <= 1e-10


# ---------------------------------------------------------------------------------------------------------------- apply
@pytest.fixture(scope='module')
def rig():
    """One model, one 3 x 20 clip and the uncalibrated EVEStream's results on its first chunk, shared and never modified."""
    model, _ = make_model(refine_net_rnn_type='CGRU')
    _, d, _ = gpu_clip(S, 4 * TC, seed=7)
    chunk = lambda t0, t1: {k: v[:, t0:t1].contiguous() for k, v in d.items()}
    keep = lambda out: {k: v.clone() for k, v in out.items()}
    c0 = chunk(0, TC)
    plain = keep(eve_amd.EVEStream(model, S, use_graph=False).step(c0))
    kappa = cuda(np.array([[KAPPA_LEFT, KAPPA_RIGHT], [-KAPPA_RIGHT, KAPPA_LEFT], [2 * KAPPA_LEFT, -KAPPA_RIGHT]], dtype=np.float32))
    return {'model': model, 'chunk': chunk, 'keep': keep, 'c0': c0, 'plain': plain, 'kappa': kappa}


def side_pog(model, plain, chunk, side, kappa=None):
    """eve_gaze_to_pog on the plain step's <side>_g_initial, optionally through a [B, 2] kappa per stream -> (g, mm, px) [B, T, 2]."""
    B, T = plain[side + '_g_initial'].shape[:2]
    N = B * T
    f = lambda key, *s: chunk[key].reshape((N,) + s).float().contiguous()
    kap = None if kappa is None else kappa[:, None, :].expand(B, T, 2).reshape(N, 2).contiguous()
    g, mm, px, _ = default_kernels().gaze_to_pog(plain[side + '_g_initial'].reshape(N, 2).contiguous(), f(side + '_o', 3), f(side + '_R', 3, 3),
                                                 f('inv_camera_transformation', 4, 4), f('pixels_per_millimeter', 2),
                                                 tuple(model.config.actual_screen_size), None if kappa is None else f('head_R', 3, 3), kap)
    return g.view(B, T, 2), mm.view(B, T, 2), px.view(B, T, 2)


def check_applied(model, out, plain, chunk, kappa, cal, frames=None, eye_valid=None):
    """out: a calibrated step's result; plain: the uncalibrated step's on the same chunk; cal: the calibrated streams (bool list).
    Calibrated streams: the kernel's own kappa path on the plain angles, bit for bit; the others: the plain bits on every key.
    frames: bool [B, T], the frames whose entries are specified (None: all)."""
    B, T = plain['left_g_initial'].shape[:2]
    sel = torch.tensor(cal, device='cuda')
    frames = torch.ones((B, T), dtype=torch.bool, device='cuda') if frames is None else frames
    assert out['calibrated'].tolist() == list(cal)
    px = []
    for e, side in enumerate(('left', 'right')):
        g_c, _, px_c = side_pog(model, plain, chunk, side, kappa[:, e])
        _, _, px_p = side_pog(model, plain, chunk, side)
        want = torch.where(sel[:, None, None], g_c, plain[side + '_g_initial'])
        ok = frames if eye_valid is None else eye_valid[:, :, e]
        assert torch.equal(out[side + '_g_initial'][ok], want[ok]), side
        assert torch.equal(out[side + '_g_initial_raw'][ok], plain[side + '_g_initial'][ok]), side
        assert not torch.equal(g_c[ok], plain[side + '_g_initial'][ok])
        px.append(torch.where(sel[:, None, None], px_c, px_p))
    want = _mean2(*px) if eye_valid is None else _fuse2(px[0], px[1], eye_valid)
    assert torch.equal(out['PoG_px_initial'][frames], want[frames])
    for b in range(B):
        if not cal[b]:
            for key in plain:
                assert torch.equal(out[key][b][frames[b]], plain[key][b][frames[b]]), key


def test_apply_is_the_kernels_kappa_path_and_spares_the_uncalibrated_stream(rig):
    model, c0, plain, kappa = rig['model'], rig['c0'], rig['plain'], rig['kappa']
    eager = eve_amd.EVEStream(model, S, use_graph=False)
    eager.set_calibration(kappa, streams=[0, 2])
    e = rig['keep'](eager.step(c0))
    check_applied(model, e, plain, c0, kappa, [True, False, True])
    graph = eve_amd.EVEStream(model, S)
    graph.set_calibration(kappa, streams=[0, 2])
    g = rig['keep'](graph.step(c0))
    assert sorted(g) == sorted(e)
    for key in e:                                        # the captured graph replays the eager step
        assert torch.equal(g[key], e[key]), key
    kap, cal = graph.get_calibration()
    assert cal.tolist() == [True, False, True] and torch.equal(kap[0], kappa[0]) and (kap[1] == 0).all()
    graph.clear_calibration()
    graph.reset()
    back = graph.step(c0)
    assert 'calibrated' not in back
    for key in plain:                                    # every stream back to the plain bits
        assert torch.equal(back[key], plain[key]), key


def test_apply_on_ragged_and_masked_steps(rig):
    model, c0, kappa = rig['model'], rig['c0'], rig['kappa']
    lengths = [5, 2, 0]
    mask = torch.ones((S, TC, 2), dtype=torch.bool, device='cuda')
    mask[0, 1, 0] = mask[0, 3, 1] = mask[2, 2, 0] = mask[2, 2, 1] = False
    mask[1, :, 1] = False
    for kw in (dict(lengths=lengths), dict(eye_mask=mask), dict(eye_mask=mask, lengths=[5, 4, 3])):
        plain = rig['keep'](eve_amd.EVEStream(model, S, use_graph=False).step(c0, **kw))
        s = eve_amd.EVEStream(model, S, use_graph=False)
        s.set_calibration(kappa, streams=[0, 2])
        out = s.step(c0, **kw)
        assert torch.equal(out['valid'], plain['valid'])
        check_applied(model, out, plain, c0, kappa, [True, False, True], frames=plain['valid'], eye_valid=plain.get('eye_valid'))


def test_the_patch_form_needs_head_r(rig):
    model, c0 = rig['model'], rig['c0']
    bare = {k: v for k, v in c0.items() if k != 'head_R'}
    s = eve_amd.EVEStream(model, S, use_graph=False)
    with pytest.raises(ValueError, match='head_R'):
        s.step(dict(bare, calibration_target=torch.zeros((S, TC, 2), device='cuda')))
    with pytest.raises(ValueError, match='inv_camera_transformation'):
        s.step(dict({k: v for k, v in c0.items() if k != 'inv_camera_transformation'}, calibration_target=torch.zeros((S, TC, 2), device='cuda')))
    s.set_calibration(rig['kappa'])
    with pytest.raises(ValueError, match='head_R'):
        s.step(bare)
    assert s.calibration_counts()[0].sum().item() == 0


# ---------------------------------------------------------------------------------------------------------------- end to end
def unclamped_targets(model, plain, chunk, side, kappa):
    """The float32 kernel's own point of gaze of one eye at kappa, in pixels: its pog_mm times pixels_per_millimeter -- the product
    it clamps to the screen for PoG_px, without the clamp (which the fitted model does not have either)."""
    B = plain[side + '_g_initial'].shape[0]
    kap = torch.tensor(kappa, dtype=torch.float32, device='cuda').expand(B, 2)
    _, mm, _ = side_pog(model, plain, chunk, side, kap)
    return mm * chunk['pixels_per_millimeter'].float()


def raw_angles(rig, sizes):
    """<side>_g_initial of an uncalibrated eager EVEStream over the clip in chunks of `sizes`, [S, sum(sizes), 2] each."""
    stream, t0, parts = eve_amd.EVEStream(rig['model'], S, use_graph=False), 0, []
    for n in sizes:
        out = stream.step(rig['chunk'](t0, t0 + n))
        parts.append({k: out[k].clone() for k in ('left_g_initial', 'right_g_initial')})
        t0 += n
    return {k: torch.cat([p[k] for p in parts], dim=1) for k in parts[0]}


def collect(stream, rig, targets, sizes):
    t0 = 0
    stream.reset()
    for n in sizes:
        stream.step(dict(rig['chunk'](t0, t0 + n), calibration_target=targets[:, t0:t0 + n].contiguous()))
        t0 += n


def test_collect_fit_and_apply_end_to_end(rig):
    """Four steps of 5 frames collect 20 samples per (stream, eye), fit_calibration recovers the offset the targets were made with.
    A chunk holds ONE target per frame and the two eyes have offsets of their own, so the run is made twice on one EVEStream: with
    the left eye's points of gaze at its kappa* as targets (the left fit is judged), then -- the store emptied, the recurrent
    state reset, the left calibration by now applied, which the collected raw angles must not feel -- with the right eye's.  The
    device kappa is within 1e-10 rad of calib_ref.fit on the store read back, and no further from kappa* than ten times the
    reference's own distance plus that 1e-10: the float32 noise of the path that made the targets (recorded in
    profiles/calibration_notes.md)."""
    model = rig['model']
    whole = rig['chunk'](0, 4 * TC)
    plain = raw_angles(rig, [TC] * 4)
    stream = eve_amd.EVEStream(model, S, calibration_capacity=32)
    for e, (side, star) in enumerate((('left', KAPPA_LEFT), ('right', KAPPA_RIGHT))):
        targets = unclamped_targets(model, plain, whole, side, star)
        stream.clear_calibration_samples()
        collect(stream, rig, targets, [TC] * 4)
        count, dropped = stream.calibration_counts()
        assert (count == 4 * TC).all() and (dropped == 0).all()
        fit = stream.fit_calibration()
        store = stream.calibration_samples().cpu().numpy()
        for b in range(S):
            ref = calib_ref.fit(store[b, e, :4 * TC])
            dev = fit['kappa'][b, e].cpu().numpy()
            print('%s eye, stream %d: device - reference %.3g rad, reference - kappa* %.3g rad, rms %.3g mm' % (
                side, b, np.abs(dev - ref['kappa']).max(), np.abs(ref['kappa'] - star).max(), float(fit['rms_mm'][b, e])))
            assert ref['ok'] and bool(fit['ok'][b, e]) and int(fit['used'][b, e]) == 4 * TC
            assert np.abs(dev - ref['kappa']).max() <= 1e-10
            assert np.abs(dev - star).max() <= 10 * np.abs(ref['kappa'] - star).max() + 1e-10
            assert torch.equal(stream.get_calibration()[0][b, e], fit['kappa'][b, e].float())
    assert fit['calibrated'].all() and stream.get_calibration()[1].all()
    # an uncalibrated eager EVEStream over the same chunks: the same store, bit for bit (the applied calibration is not felt)
    eager = eve_amd.EVEStream(model, S, use_graph=False, calibration_capacity=32)
    collect(eager, rig, targets, [TC] * 4)
    assert torch.equal(eager.calibration_samples(), stream.calibration_samples())


def test_a_split_into_chunks_of_two_and_three_gives_the_same_store(rig):
    targets = torch.full((S, 4 * TC, 2), 600.0, device='cuda')
    fives = eve_amd.EVEStream(rig['model'], S, use_graph=False, calibration_capacity=32)
    collect(fives, rig, targets, [TC] * 4)
    split = eve_amd.EVEStream(rig['model'], S, use_graph=False, calibration_capacity=32)
    collect(split, rig, targets, [2, 3] * 4)
    a, b = raw_angles(rig, [TC] * 4), raw_angles(rig, [2, 3] * 4)
    print('raw angles, chunks of 5 against chunks of 2 and 3: %.3g rad' % max(float((a[k] - b[k]).abs().max()) for k in a))
    assert torch.equal(split.calibration_counts()[0], fives.calibration_counts()[0])
    assert torch.equal(split.calibration_samples(), fives.calibration_samples())


def test_capturing_a_new_shape_appends_once(rig):
    targets = torch.full((S, 4 * TC, 2), 600.0, device='cuda')
    stream = eve_amd.EVEStream(rig['model'], S, calibration_capacity=32)
    step = lambda t0, t1: stream.step(dict(rig['chunk'](t0, t1), calibration_target=targets[:, t0:t1].contiguous()))
    step(0, 5)
    assert (stream.calibration_counts()[0] == 5).all()
    step(5, 8)                                           # a new chunk shape: two eager warm-up steps and a capture, appended once
    assert (stream.calibration_counts()[0] == 8).all()
    step(8, 13)                                          # a replay
    count, dropped = stream.calibration_counts()
    assert (count == 13).all() and (dropped == 0).all()
    eager = eve_amd.EVEStream(rig['model'], S, use_graph=False, calibration_capacity=32)
    for t0, t1 in ((0, 5), (5, 8), (8, 13)):
        eager.step(dict(rig['chunk'](t0, t1), calibration_target=targets[:, t0:t1].contiguous()))
    assert torch.equal(eager.calibration_samples(), stream.calibration_samples())
