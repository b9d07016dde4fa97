"""CPU: the per-person gaze calibration's contract in numpy (tests/calib_ref.py) on its own scenes, the argument checks of
eve_amd.data.calibration_samples / fit_gaze_offset, and the EVEStream plumbing (collect, fit, apply, the refusals) over a
stand-in whose two calibration entry points are calib_ref itself.  The GPU suite (test_gpu_calibration.py) checks the HIP kernels."""
import numpy as np
import pytest
import torch

import calib_ref
import eve_amd
from eve_amd import data, kernels
from test_stream_host import chunk_of, clip, make_model
from test_stream_mask_host import MaskFakes


# ---------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize('n', [5, 64, 65, 130])
def test_the_reference_recovers_kappa_from_noise_free_scenes(n):
    """Targets are the model's own at kappa*, rounded to float32 (6e-8 relative of ~1000 px: 6e-5 px, 2e-5 mm, over ~600 mm of
    lever: a few 1e-8 rad at n = 5, less with more samples): within 5e-8 rad."""
    rows = calib_ref.scene_rows(calib_ref.make_scene(100 + n, n, calib_ref.KAPPA_STAR))
    f = calib_ref.fit(rows)
    assert f['ok'] and f['used'] == n and f['inliers'] == n and f['accepted'] <= 8
    assert np.abs(f['kappa'] - calib_ref.KAPPA_STAR).max() < 5e-8
    assert f['rms_mm'] < 1e-3
    assert np.abs(calib_ref.pog(rows, f['kappa']) - rows[:, 12:14]).max() < 1e-3
    back = calib_ref.fit(rows, reverse=True)
    assert np.abs(back['kappa'] - f['kappa']).max() < 1e-14              # the summation order is worth nothing here


def test_the_huber_fit_beats_the_plain_one():
    h = calib_ref.HUBER_SCENE
    rows = calib_ref.scene_rows(calib_ref.make_scene(2, h['n'], calib_ref.KAPPA_STAR, noise_mm=h['noise_mm'], outliers=h['outliers']))
    robust, plain = calib_ref.fit(rows, huber_mm=h['huber_mm']), calib_ref.fit(rows)
    assert robust['ok'] and plain['ok'] and robust['used'] == plain['used'] == plain['inliers'] == h['n']
    assert h['n'] - 2 * h['outliers'] <= robust['inliers'] <= h['n'] - h['outliers'] + 2
    err = lambda f: np.rad2deg(np.linalg.norm(f['kappa'] - calib_ref.KAPPA_STAR))
    assert err(robust) < 0.35 and err(robust) < 0.5 * err(plain)
    assert robust['rms_mm'] > h['noise_mm']                               # the rms is over ALL used samples, outliers included


def test_the_reference_refuses_what_the_header_refuses():
    rows = calib_ref.scene_rows(calib_ref.make_scene(8, 20, calib_ref.KAPPA_STAR))
    assert not calib_ref.fit(rows[:4])['ok'] and calib_ref.fit(rows[:4])['used'] == 4
    assert calib_ref.fit(rows[:4], min_samples=4)['ok']
    assert not calib_ref.fit(rows[:0])['ok']
    far = calib_ref.scene_rows(calib_ref.make_scene(7, 20, np.array([0.5, 0.0])))
    assert not calib_ref.fit(far)['ok']
    flat = rows.copy()
    flat[:, [1, 4, 7]] = 0.0                                              # A's middle column: the pitch moves nothing
    assert not calib_ref.fit(flat)['ok']
    absent = rows.copy()
    absent[4:, 14] = 0.0
    assert calib_ref.fit(absent)['used'] == 4 and not calib_ref.fit(absent)['ok']


def test_reduce_marks_the_unusable():
    sc = calib_ref.make_scene(3, 6, calib_ref.KAPPA_STAR)
    sc['target'][1, 0] = np.nan
    sc['head_R'][2, 1, 1] = np.nan
    sc['ppm'][3, 0] = 0.0                                                 # m = c / 0
    sc['origin'][4, 2] = -600.0                                           # behind the screen plane: the target is behind the eye
    rows, usable = calib_ref.reduce(sc['g'], sc['head_R'], sc['origin'], sc['R'], sc['inv_cam'], sc['ppm'], sc['target'])
    assert usable.tolist() == [True, False, False, False, False, True]
    assert (rows[usable][:, 14] == 1.0).all() and (rows[usable][:, 15] == 0.0).all()


# ---------------------------------------------------------------------------------------------------------------- data.*
def test_data_argument_checks():
    for bad in (0, -1.0, float('nan'), float('inf'), True, '3'):
        with pytest.raises(ValueError, match='huber_mm'):
            data.check_huber_mm(bad, 'x')
    assert data.check_huber_mm(None, 'x') is None and data.check_huber_mm(25, 'x') == 25.0
    s = torch.zeros(2, 8, 16, dtype=torch.float64)
    with pytest.raises(TypeError, match='float64'):
        data.fit_gaze_offset(s.float())
    with pytest.raises(TypeError, match='16'):
        data.fit_gaze_offset(torch.zeros(2, 8, 15, dtype=torch.float64))
    with pytest.raises(ValueError, match='huber_mm'):
        data.fit_gaze_offset(s, huber_mm=-1)
    with pytest.raises(ValueError, match='min_samples'):
        data.fit_gaze_offset(s, min_samples=0)
    with pytest.raises(ValueError, match='counts'):
        data.fit_gaze_offset(s, counts=[1, 2, 3])
    g = torch.zeros(4, 2)
    good = dict(g=g, head_R=torch.zeros(4, 3, 3), origin=torch.zeros(4, 3), R=torch.zeros(4, 3, 3),
                inv_camera_transformation=torch.zeros(4, 4, 4), pixels_per_millimeter=torch.zeros(4, 2), target_px=torch.zeros(4, 2))
    for key, wrong in (('g', g.double()), ('head_R', torch.zeros(4, 9)), ('origin', torch.zeros(3, 3)), ('target_px', torch.zeros(4, 2).double())):
        with pytest.raises(TypeError, match=key):
            data.calibration_samples(**dict(good, **{key: wrong}))


# ---------------------------------------------------------------------------------------------------------------- EVEStream
class CalibFakes(MaskFakes):
    """MaskFakes (the ragged and masked steps' stand-ins) plus the two calibration entry points, evaluated by tests/calib_ref.py."""

    def calib_append(self, g, head_R, origin, R, inv_cam, ppm, target, samples, count, dropped, valid=None, lengths=None, eye_valid=None):
        self.calls.append('calib_append')
        E, B, T = g.shape[:3]
        C = samples.shape[2]
        n = lambda t: t.detach().numpy()
        for b in range(B):
            for e in range(E):
                rows, usable = calib_ref.reduce(n(g[e, b]), n(head_R[b]), n(origin[e, b]), n(R[e, b]), n(inv_cam[b]), n(ppm[b]), n(target[b]))
                for t in range(T if lengths is None else int(lengths[b])):
                    if (valid is not None and not valid[b, t]) or (eye_valid is not None and not eye_valid[b, t, e]) or not usable[t]:
                        continue
                    if int(count[b, e]) >= C:
                        dropped[b, e] += 1
                        continue
                    samples[b, e, int(count[b, e])] = torch.from_numpy(rows[t])
                    count[b, e] += 1

    def calib_fit(self, samples, count=None, select=None, huber_mm=None, min_samples=5, kappa_store=None, ok_store=None):
        self.calls.append('calib_fit')
        S = samples.shape[0]
        kappa, rms = torch.zeros(S, 2, dtype=torch.float64), torch.zeros(S, dtype=torch.float64)
        used, inliers, ok = torch.zeros(S, dtype=torch.int32), torch.zeros(S, dtype=torch.int32), torch.zeros(S, dtype=torch.uint8)
        for q in range(S):
            if select is not None and not select[q]:
                continue
            f = calib_ref.fit(samples[q, :samples.shape[1] if count is None else int(count[q])].numpy(), huber_mm, min_samples)
            kappa[q], rms[q], used[q], inliers[q], ok[q] = torch.from_numpy(f['kappa']), f['rms_mm'], f['used'], f['inliers'], int(f['ok'])
            if f['ok'] and kappa_store is not None:
                kappa_store[q] = kappa[q].float()
                ok_store[q] = 1
        return kappa, rms, used, inliers, ok


@pytest.fixture()
def fake():
    k = CalibFakes()
    kernels.set_default_kernels(k)
    yield k
    kernels.set_default_kernels(None)
    eve_amd.reset_standalone_config()


B, T = 2, 3
KAPPA = torch.tensor([[[0.04, -0.05], [0.03, 0.02]], [[-0.02, 0.01], [0.05, -0.03]]])


@pytest.fixture()
def scene(fake):
    model, _ = make_model(dict(refine_net_rnn_type='CGRU'))
    batch = clip(B, 2 * T, size=32)
    return model, chunk_of(batch, 0, T), chunk_of(batch, T, 2 * T)


def run(stream, chunk, **kw):
    return {k: v.clone() for k, v in stream.step(chunk, **kw).items()}


def targets_of(model, chunk, kappa):
    """The float32 path's own PoG_px of the chunk at the given offsets, both eyes' mean: targets a fit can recover them from."""
    s = eve_amd.EVEStream(model, B, use_graph=False)
    s.set_calibration(kappa)
    return run(s, chunk)['PoG_px_initial']


def test_an_untouched_stream_issues_what_it_always_did(fake, scene):
    model, c0, _ = scene
    s = eve_amd.EVEStream(model, B, use_graph=False)
    out = run(s, c0)
    assert 'calib_append' not in fake.calls and 'calibrated' not in out and 'left_g_initial_raw' not in out
    assert s._calib_store is None
    k0 = s._graph_key(c0, False)
    s.set_calibration(KAPPA)
    assert s._graph_key(c0, False) != k0
    assert s._graph_key(dict(c0, calibration_target=torch.zeros(B, T, 2)), False) != s._graph_key(c0, False)
    s.clear_calibration()
    assert s._graph_key(c0, False) == k0


def test_collect_fit_apply(fake, scene):
    model, c0, c1 = scene
    plain = eve_amd.EVEStream(model, B, use_graph=False)
    p0 = run(plain, c0)
    t0 = targets_of(model, c0, KAPPA)
    s = eve_amd.EVEStream(model, B, use_graph=False, calibration_capacity=8)
    valid = torch.ones(B, T, dtype=torch.bool)
    valid[1, 1] = False
    out = run(s, dict(c0, calibration_target=t0, calibration_valid=valid))
    assert fake.calls.count('calib_append') == 1
    for k in p0:                                       # collecting changes no result
        assert torch.equal(out[k], p0[k]), k
    count, dropped = s.calibration_counts()
    assert count.tolist() == [[3, 3], [2, 2]] and dropped.tolist() == [[0, 0], [0, 0]]
    # the rows are the reference's reduction of the raw angles, in frame order
    rows, usable = calib_ref.reduce(p0['left_g_initial'][0].numpy(), c0['head_R'][0].numpy(), c0['left_o'][0].numpy(), c0['left_R'][0].numpy(),
                                    c0['inv_camera_transformation'][0].numpy(), c0['pixels_per_millimeter'][0].numpy(), t0[0].numpy())
    assert usable.all() and np.array_equal(s.calibration_samples()[0, 0, :3].numpy(), rows)
    fit = s.fit_calibration(min_samples=3, streams=[0])
    assert fit['ok'].tolist() == [[True, True], [False, False]] and fit['calibrated'].tolist() == [True, False]
    assert fit['used'].tolist() == [[3, 3], [0, 0]]
    kap, cal = s.get_calibration()
    assert cal.tolist() == [True, False] and torch.equal(kap[0], fit['kappa'][0].float()) and (kap[1] == 0).all()
    # (the targets are the two eyes' MEAN PoG, so each eye's own fit is not kappa*: only the plumbing is judged here)
    s.reset()
    second = run(s, c0)
    assert second['calibrated'].tolist() == [True, False]
    for k in p0:                                       # the uncalibrated stream: the plain bits, inside the applying step
        assert torch.equal(second[k][1], p0[k][1]), k
    for side in ('left', 'right'):
        assert torch.equal(second[side + '_g_initial_raw'], p0[side + '_g_initial'])
        assert not torch.equal(second[side + '_g_initial'][0], p0[side + '_g_initial'][0])
    assert s.calibration_counts()[0].tolist() == [[3, 3], [2, 2]]        # reset() and a plain step leave the store alone
    # collecting while calibrated reads the raw angles: the same rows again
    s.clear_calibration_samples([0])
    s.reset()
    run(s, dict(c0, calibration_target=t0))
    assert s.calibration_counts()[0].tolist() == [[3, 3], [5, 5]]
    assert np.array_equal(s.calibration_samples()[0, 0, :3].numpy(), rows)
    s.clear_calibration()
    s.reset()
    third = run(s, c0)
    assert 'calibrated' not in third
    for k in p0:
        assert torch.equal(third[k], p0[k]), k


def test_apply_is_the_kernels_own_kappa_path(fake, scene):
    model, c0, _ = scene
    p0 = run(eve_amd.EVEStream(model, B, use_graph=False), c0)
    s = eve_amd.EVEStream(model, B, use_graph=False)
    s.set_calibration(KAPPA, streams=[1])
    out = run(s, c0)
    N = B * T
    px = []
    for e, side in enumerate(('left', 'right')):
        g, _, p, _ = fake.gaze_to_pog(p0[side + '_g_initial'].reshape(N, 2), c0[side + '_o'].reshape(N, 3), c0[side + '_R'].reshape(N, 3, 3),
                                      c0['inv_camera_transformation'].reshape(N, 4, 4), c0['pixels_per_millimeter'].reshape(N, 2),
                                      tuple(model.config.actual_screen_size), c0['head_R'].reshape(N, 3, 3),
                                      KAPPA[:, e, None, :].expand(B, T, 2).reshape(N, 2))
        assert torch.equal(out[side + '_g_initial'][1], g.view(B, T, 2)[1])
        px.append(p.view(B, T, 2))
    assert torch.equal(out['PoG_px_initial'][1], torch.stack(px, dim=-1).mean(dim=-1)[1])
    for k in p0:
        assert torch.equal(out[k][0], p0[k][0]), k


def test_ragged_and_overflow(fake, scene):
    model, c0, c1 = scene
    t0 = targets_of(model, c0, KAPPA)
    s = eve_amd.EVEStream(model, B, use_graph=False, calibration_capacity=4)
    run(s, dict(c0, calibration_target=t0), lengths=[2, 0])
    assert s.calibration_counts()[0].tolist() == [[2, 2], [0, 0]]
    mask = torch.ones(B, T, 2, dtype=torch.bool)
    mask[1, :, 0] = False
    run(s, dict(c1, calibration_target=t0), eye_mask=mask)
    count, dropped = s.calibration_counts()
    assert count.tolist() == [[4, 4], [0, 3]] and dropped.tolist() == [[1, 1], [0, 0]]


def test_refusals(fake, scene):
    model, c0, _ = scene
    s = eve_amd.EVEStream(model, B, use_graph=False)
    t0 = torch.zeros(B, T, 2)
    with pytest.raises(ValueError, match='head_R'):
        s.step(dict({k: v for k, v in c0.items() if k != 'head_R'}, calibration_target=t0))
    with pytest.raises(ValueError, match='inv_camera_transformation'):
        s.step(dict({k: v for k, v in c0.items() if k != 'inv_camera_transformation'}, calibration_target=t0))
    with pytest.raises(ValueError, match='calibration_target'):
        s.step(dict(c0, calibration_valid=torch.ones(B, T, dtype=torch.bool)))
    with pytest.raises(ValueError, match='calibration_target'):
        s.step(dict(c0, calibration_target=t0.double()))
    with pytest.raises(ValueError, match='calibration_valid'):
        s.step(dict(c0, calibration_target=t0, calibration_valid=torch.ones(B, T)))
    with pytest.raises(ValueError, match='huber_mm'):
        s.fit_calibration(huber_mm=0)
    with pytest.raises(ValueError, match='kappa'):
        s.set_calibration(torch.zeros(B, 2))
    with pytest.raises(ValueError, match='calibration_capacity'):
        eve_amd.EVEStream(model, B, use_graph=False, calibration_capacity=0)
    assert 'calib_append' not in fake.calls and 'calib_fit' not in fake.calls
    s.set_calibration(KAPPA)
    with pytest.raises(ValueError, match='head_R'):
        s.step({k: v for k, v in c0.items() if k != 'head_R'})
