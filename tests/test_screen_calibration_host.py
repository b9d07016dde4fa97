"""CPU: the screen-space gaze calibration's contract in numpy (tests/screen_calib_ref.py) on its own scenes, the argument checks of
eve_amd.data.screen_calibration_samples / fit_screen_map / evaluate_screen_map / apply_screen_map, and the EVEStream plumbing (collect,
fit, apply, evaluate, the refusals) over a stand-in whose three entry points are screen_calib_ref itself.  The GPU suite
(test_gpu_screen_calibration.py) checks the HIP kernels."""
import numpy as np
import pytest
import torch

import eve_amd
import screen_calib_ref as ref
from eve_amd import data, kernels
from eve_amd.data import SCREEN_CALIB_REPORT, GazeEventSpec, OverlaySpec
from eve_amd.eve import _mean2
from test_calibration_host import CalibFakes
from test_gaze_events_host import EventOverlayFakes
from test_overlay_host import stream_chunk
from test_stream_host import chunk_of, clip, make_model

MODELS = ('offset', 'affine', 'quadratic')


# ---------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize('dots', [(3, 3), (4, 3)])
@pytest.mark.parametrize('model', MODELS)
def test_the_reference_recovers_the_known_map(model, dots):
    """Noise-free: the raw points are the targets through the inverse of the known map, rounded to float32 -- one ulp at 1920 px is
    1.2e-4 px = 3.6e-5 mm -- so the map comes back within 1e-3 mm (about 30 ulp) at the nine points u, v in {-1, 0, 1}."""
    sc = ref.make_scene(11, dots=dots, model=model)
    rows = ref.scene_rows(sc)
    f = ref.fit(rows, model)
    assert f['ok'] and f['used'] == rows.shape[0] and f['inliers'] == f['used'] and f['solves'] == 1 and f['kind'] == sc['kind']
    assert ref.map_error_mm(f['coef'], f['kind'], sc['coef'], sc['kind']) < 1e-3
    assert f['rms_mm'] < 1e-3 and f['max_mm'] < 1e-3 and f['mean_deg'] < 1e-3 and f['rms_mm_raw'] > 5.0 and f['mean_deg_raw'] > 0.5
    assert (f['coef'][:, ref.terms_of(f['kind']):] == 0).all()
    # the Huber fit of clean data: every sample an inlier from the second pass on, the same map
    h = ref.fit(rows, model, huber_mm=25.0)
    assert h['ok'] and h['inliers'] == h['used'] and 2 <= h['solves'] <= ref.MAX_SOLVES
    assert ref.map_error_mm(h['coef'], h['kind'], sc['coef'], sc['kind']) < 1e-3


@pytest.mark.parametrize('seed', [1, 2, 3])
@pytest.mark.parametrize('model', ['affine', 'quadratic'])
def test_the_huber_fit_beats_the_plain_one(model, seed):
    """135 samples (3 x 3 dots, 15 frames each), 8 mm of noise, 10 % outliers 80 .. 200 mm away: the Huber fit's worst error over the
    nine points is at most half the plain fit's.  max_shift_mm is 400 here: an outlier up to 200 mm off its dot can lie far outside
    the screen, where a quadratic legitimately corrects by more than the default guard of 100 mm."""
    sc = ref.make_scene(seed, dots=(3, 3), per_dot=15, noise_mm=8.0, outliers=13, model=model)
    rows = ref.scene_rows(sc)
    robust, plain = ref.fit(rows, model, huber_mm=25.0, max_shift_mm=400.0), ref.fit(rows, model, max_shift_mm=400.0)
    assert robust['ok'] and robust['solves'] <= ref.MAX_SOLVES and plain['ok'] and plain['solves'] == 1
    assert robust['used'] == plain['used'] == plain['inliers'] == 135
    assert 135 - 2 * 13 <= robust['inliers'] <= 135 - 13 + 2
    err = lambda f: ref.map_error_mm(f['coef'], f['kind'], sc['coef'], sc['kind'])
    print('%s seed %d: huber %.2f mm (%d solves), plain %.2f mm' % (model, seed, err(robust), robust['solves'], err(plain)))
    assert err(robust) <= 0.5 * err(plain)
    assert robust['rms_mm'] > 8.0 and robust['rms_mm'] < robust['rms_mm_raw']       # over ALL used samples, outliers included


def test_the_reference_refuses_what_the_header_refuses():
    line = ref.scene_rows(ref.make_scene(5, dots=(3, 1), per_dot=2, model='affine'))
    assert not ref.fit(line, 'affine')['ok'] and ref.fit(line, 'affine')['used'] == 6
    assert ref.fit(line, 'offset')['ok']
    row = ref.scene_rows(ref.make_scene(5, dots=(5, 1), per_dot=2, model='quadratic'))
    assert not ref.fit(row, 'quadratic')['ok'] and ref.fit(row, 'quadratic')['used'] == 10
    five = ref.scene_rows(ref.make_scene(5, dots=(3, 3), per_dot=2, model='quadratic'))[:10]       # five distinct positions
    assert not ref.fit(five, 'quadratic')['ok']
    grid = ref.scene_rows(ref.make_scene(5, dots=(3, 3), model='affine'))
    assert not ref.fit(grid[:2], 'affine')['ok'] and ref.fit(grid[:2], 'affine')['used'] == 2        # fewer samples than K
    assert ref.fit(grid[:4], 'affine')['ok'] and not ref.fit(grid[:4], 'affine', min_samples=5)['ok']
    assert not ref.fit(grid[:0], 'offset')['ok']
    absent = grid.copy()
    absent[2:, 9] = 0.0
    assert ref.fit(absent, 'affine')['used'] == 2 and not ref.fit(absent, 'affine')['ok']
    far = ref.coef_star('affine')
    far[0, 0] = 150.0
    rows = ref.scene_rows(ref.make_scene(5, dots=(3, 3), model='affine', coef=far))
    refused = ref.fit(rows, 'affine')
    assert not refused['ok'] and refused['used'] == 9 and not refused['coef'].any() and refused['rms_mm'] == 0.0
    assert ref.fit(rows, 'affine', max_shift_mm=400.0)['ok']


def test_reduce_marks_the_unusable():
    sc = ref.make_scene(3, dots=(4, 2), model='affine')
    sc['target'][1, 0] = np.nan
    sc['inv_cam'][2, 1, 1] = np.inf
    sc['ppm'][3, 0] = 0.0
    sc['ppm'][4, 1] = -3.5
    sc['origin'][5] = 0.0
    sc['inv_cam'][5, 2, 3] = 0.0                                          # e_2 = 0: the eye in the screen plane
    sc['pog'][6, 1] = np.nan
    rows, usable = ref.reduce(sc['pog'], sc['origin'], sc['inv_cam'], sc['ppm'], sc['target'], sc['screen_size'])
    assert usable.tolist() == [True, False, False, False, False, False, False, True]
    assert (rows[usable][:, 9] == 1.0).all() and (rows[usable][:, 10:] == 0.0).all()
    x = sc['pog'][0].astype(np.float64)
    assert rows[0, 0] == (x[0] + x[0]) / 1920.0 - 1.0 and rows[0, 3] == x[1] / np.float64(np.float32(3.5))


def test_apply_clamps_keeps_a_nan_and_the_bits_of_kind_0():
    coef = np.zeros((2, 6))
    coef[:, 0] = (10.0, -10.0)
    px = np.array([[1.0, 1079.0], [1919.0, 1.0], [960.0, 540.0], [np.nan, 540.0], [-0.0, 5.0]], dtype=np.float32)
    ppm = np.tile(np.array([3.4, 3.5], dtype=np.float32), (5, 1))
    out = ref.apply(px, ppm, coef, 1, ref.SCREEN)
    assert out[0, 1] == 1044.0 and out[1, 0] == 1920.0 and out[1, 1] == 0.0 and np.isnan(out[3, 0]) and out[3, 1] == 505.0
    assert out[2, 0] == np.float32(960.0 + 10.0 * np.float64(np.float32(3.4)))
    assert ref.apply(px, ppm, -coef, 1, ref.SCREEN)[0].tolist() == [0.0, 1080.0]
    assert ref.apply(px, ppm, coef, 0, ref.SCREEN).tobytes() == px.tobytes()
    assert ref.apply(px, ppm, coef, 7, ref.SCREEN).tobytes() == px.tobytes()


def test_evaluate_is_the_fits_own_report_and_kind_0_reports_the_raw_numbers():
    sc = ref.make_scene(9, dots=(3, 3), per_dot=3, noise_mm=4.0, model='quadratic')
    rows = ref.scene_rows(sc)
    f = ref.fit(rows, 'quadratic')
    e = ref.evaluate(rows, f['coef'], f['kind'])
    assert e['ok'] and e['solves'] == 0 and e['inliers'] == e['used'] == 27
    for k in SCREEN_CALIB_REPORT:
        assert e[k] == f[k], k
    assert f['rms_mm'] < 8.0 < f['rms_mm_raw'] and f['mean_mm'] <= f['rms_mm'] <= f['max_mm'] and f['mean_deg'] < f['mean_deg_raw']
    none = ref.evaluate(rows, f['coef'], 0)
    assert none['ok'] and not none['coef'].any()
    for k in ('rms_mm', 'mean_mm', 'max_mm', 'mean_deg'):
        assert none[k] == none[k + '_raw'] == f[k + '_raw'], k
    assert not ref.evaluate(rows[:0], f['coef'], 3)['ok']
    # the angle: 10 mm beside the target seen from 600 mm straight in front of it
    one = np.array([[0.0, 0.0, 10.0, 0.0, 0.0, 0.0, 0.0, 0.0, 600.0, 1.0, 0.0, 0.0]])
    assert abs(ref.evaluate(one, np.zeros((2, 6)), 0)['mean_deg'] - np.degrees(np.arctan(10.0 / 600.0))) < 1e-12


# ---------------------------------------------------------------------------------------------------------------- data.*
def test_data_argument_checks():
    for bad in ('cubic', None, 2, b'affine'):
        with pytest.raises(ValueError, match='model'):
            data.check_screen_model(bad, 'x')
    assert [data.check_screen_model(m, 'x') for m in MODELS] == [1, 2, 3]
    for bad in (0, -1.0, float('nan'), float('inf'), True, '3', None):
        with pytest.raises(ValueError, match='max_shift_mm'):
            data.check_max_shift_mm(bad, 'x')
    for bad in ((1920,), (1920, 0), (1920, float('nan')), 1920, ('a', 'b'), (True, 5)):
        with pytest.raises(ValueError, match='screen_size'):
            data.check_screen_size(bad, 'x')
    s = torch.zeros(2, 8, 12, dtype=torch.float64)
    with pytest.raises(TypeError, match='float64'):
        data.fit_screen_map(s.float())
    with pytest.raises(TypeError, match='12'):
        data.fit_screen_map(torch.zeros(2, 8, 16, dtype=torch.float64))
    with pytest.raises(ValueError, match='model'):
        data.fit_screen_map(s, model='cubic')
    with pytest.raises(ValueError, match='huber_mm'):
        data.fit_screen_map(s, huber_mm=-1)
    with pytest.raises(ValueError, match='min_samples'):
        data.fit_screen_map(s, min_samples=0)
    with pytest.raises(ValueError, match='max_shift_mm'):
        data.fit_screen_map(s, max_shift_mm=0)
    with pytest.raises(ValueError, match='counts'):
        data.fit_screen_map(s, counts=[1, 2, 3])
    with pytest.raises(ValueError, match='coef'):
        data.evaluate_screen_map(s, torch.zeros(2, 6), [1, 1])
    with pytest.raises(ValueError, match='kind'):
        data.evaluate_screen_map(s, torch.zeros(2, 2, 6), [1.0, 1.0])
    good = dict(pog_px=torch.zeros(4, 2), o=torch.zeros(4, 3), inv_camera_transformation=torch.zeros(4, 4, 4),
                pixels_per_millimeter=torch.zeros(4, 2), target_px=torch.zeros(4, 2), screen_size=(1920, 1080))
    for key, wrong in (('pog_px', torch.zeros(4, 2).double()), ('o', torch.zeros(4, 2)), ('inv_camera_transformation', torch.zeros(4, 16)),
                       ('target_px', torch.zeros(3, 2))):
        with pytest.raises(TypeError, match=key):
            data.screen_calibration_samples(**dict(good, **{key: wrong}))
    with pytest.raises(ValueError, match='screen_size'):
        data.screen_calibration_samples(**dict(good, screen_size=(0, 1080)))
    with pytest.raises(TypeError, match='pixels_per_millimeter'):
        data.apply_screen_map(torch.zeros(2, 3, 2), torch.zeros(2, 3), torch.zeros(2, 2, 6), [1, 1], (1920, 1080))
    assert eve_amd.fit_screen_map is data.fit_screen_map and eve_amd.apply_screen_map is data.apply_screen_map


# ---------------------------------------------------------------------------------------------------------------- EVEStream
class ScreenFakes(EventOverlayFakes, CalibFakes):
    """The ragged, masked, calibration, gaze-event and overlay stand-ins plus the three screen calibration entry points, evaluated
    by tests/screen_calib_ref.py."""

    def screen_calib_append(self, pog, origin, inv_cam, ppm, target, screen_size, samples, count, dropped, valid=None, lengths=None,
                            frame_valid=None):
        self.calls.append('screen_calib_append')
        B, T = pog.shape[:2]
        C = samples.shape[1]
        n = lambda t: t.detach().numpy()
        for b in range(B):
            rows, usable = ref.reduce(n(pog[b]), n(origin[b]), n(inv_cam[b]), n(ppm[b]), n(target[b]), screen_size)
            for t in range(T if lengths is None else min(max(int(lengths[b]), 0), T)):
                if (valid is not None and not valid[b, t]) or (frame_valid is not None and not frame_valid[b, t]) or not usable[t]:
                    continue
                if int(count[b]) >= C:
                    dropped[b] += 1
                    continue
                samples[b, int(count[b])] = torch.from_numpy(rows[t])
                count[b] += 1

    def screen_calib_fit(self, samples, count=None, select=None, mode=0, kind=2, huber_mm=None, min_samples=1, max_shift_mm=100.0,
                         coef_store=None, kind_store=None):
        self.calls.append('screen_calib_fit')
        S = samples.shape[0]
        coef, report = torch.zeros(S, 2, 6, dtype=torch.float64), torch.zeros(S, 8, dtype=torch.float64)
        used, inliers, solves = (torch.zeros(S, dtype=torch.int32) for _ in range(3))
        ok = torch.zeros(S, dtype=torch.uint8)
        for q in range(S):
            if select is not None and not select[q]:
                continue
            rows = samples[q, :samples.shape[1] if count is None else min(max(int(count[q]), 0), samples.shape[1])].numpy()
            if mode == 1:
                f = ref.evaluate(rows, coef_store[q].numpy(), int(kind_store[q]))
            else:
                f = ref.fit(rows, kind, huber_mm, min_samples, max_shift_mm)
            coef[q], used[q], inliers[q], solves[q], ok[q] = torch.from_numpy(f['coef']), f['used'], f['inliers'], f['solves'], int(f['ok'])
            report[q] = torch.tensor([f[k] for k in SCREEN_CALIB_REPORT], dtype=torch.float64)
            if f['ok'] and mode == 0 and coef_store is not None:
                coef_store[q] = coef[q]
                kind_store[q] = kind
        return coef, report, used, inliers, solves, ok

    def screen_calib_apply(self, px, ppm, coef, kind, screen_size):
        self.calls.append('screen_calib_apply')
        out = torch.empty_like(px)
        for b in range(px.shape[0]):
            out[b] = torch.from_numpy(ref.apply(px[b].numpy(), ppm[b].numpy(), coef[b].numpy(), int(kind[b]), screen_size))
        return out

    def overlay_render(self, frames, format, out_format='nv12', matrix='bt601', centres=None, **kw):
        self.last_centres = None if centres is None else centres.clone()
        return EventOverlayFakes.overlay_render(self, frames, format, out_format, matrix, centres=centres, **kw)


NEW_CALLS = ('screen_calib_append', 'screen_calib_fit', 'screen_calib_apply')


@pytest.fixture()
def fake():
    k = ScreenFakes()
    kernels.set_default_kernels(k)
    yield k
    kernels.set_default_kernels(None)
    eve_amd.reset_standalone_config()


B, T = 2, 3
SHIFT_MM = (5.0, -3.0)


@pytest.fixture()
def scene(fake):
    model, _ = make_model(dict(refine_net_rnn_type='CGRU'))
    batch = clip(B, 2 * T, size=32)
    return model, chunk_of(batch, 0, T), chunk_of(batch, T, 2 * T)


def run(stream, chunk, **kw):
    return {k: v.clone() for k, v in stream.step(chunk, **kw).items()}


def size_of(model):
    return tuple(model.config.actual_screen_size)


def targets_of(px, chunk, shift_mm=SHIFT_MM):
    """Targets a known shift in millimetres away from the uncorrected point."""
    return (px + torch.tensor(shift_mm) * chunk['pixels_per_millimeter']).contiguous()


def rows_of(px, chunk, target, model):
    o = _mean2(chunk['left_o'], chunk['right_o'])
    n = lambda t: t.reshape((-1,) + tuple(t.shape[2:])).numpy()
    rows, usable = ref.reduce(n(px), n(o), n(chunk['inv_camera_transformation']), n(chunk['pixels_per_millimeter']), n(target), size_of(model))
    return rows.reshape(px.shape[0], px.shape[1], 12), usable.reshape(px.shape[:2])


def test_an_untouched_stream_issues_what_it_always_did(fake, scene):
    model, c0, _ = scene
    seen = []
    inner = model._predict_sequence
    model._predict_sequence = lambda *a, **kw: seen.append(sorted(kw)) or inner(*a, **kw)
    s = eve_amd.EVEStream(model, B, use_graph=False)
    out = run(s, c0)
    plain_calls = list(fake.calls)
    assert not set(NEW_CALLS) & set(plain_calls) and 'screen_calibration' not in seen[-1]
    assert 'screen_calibrated' not in out and 'PoG_px_final_raw' not in out and s._screen_store is None
    k0 = s._graph_key(c0, False)
    # a map set and cleared again: the same key, the same keyword arguments, the same launches
    s.set_screen_calibration(torch.zeros(B, 2, 6), [1, 0])
    assert s._graph_key(c0, False) != k0
    assert s._graph_key(dict(c0, screen_calibration_target=torch.zeros(B, T, 2)), False) != s._graph_key(c0, False)
    s.clear_screen_calibration()
    assert s._graph_key(c0, False) == k0
    s.reset()
    del fake.calls[:]
    again = run(s, c0)
    assert fake.calls == plain_calls and seen[-1] == seen[0] and sorted(again) == sorted(out)
    for k in out:
        assert torch.equal(again[k], out[k]), k


def test_collect_fit_apply(fake, scene):
    model, c0, c1 = scene
    p0 = run(eve_amd.EVEStream(model, B, use_graph=False), c0)
    t0 = targets_of(p0['PoG_px_final'], c0)
    s = eve_amd.EVEStream(model, B, use_graph=False, screen_calibration_capacity=8)
    valid = torch.ones(B, T, dtype=torch.bool)
    valid[1, 1] = False
    del fake.calls[:]
    out = run(s, dict(c0, screen_calibration_target=t0, screen_calibration_valid=valid))
    assert fake.calls.count('screen_calib_append') == 1 and 'screen_calib_apply' not in fake.calls
    assert sorted(out) == sorted(p0)
    for k in p0:                                       # collecting changes no result
        assert torch.equal(out[k], p0[k]), k
    count, dropped = s.screen_calibration_counts()
    assert count.tolist() == [3, 2] and dropped.tolist() == [0, 0]
    rows, usable = rows_of(p0['PoG_px_final'], c0, t0, model)
    assert usable.all() and np.array_equal(s.screen_calibration_samples()[0, :3].numpy(), rows[0])
    assert np.array_equal(s.screen_calibration_samples()[1, :2].numpy(), rows[1, [0, 2]])
    fit = s.fit_screen_calibration(model='offset', streams=[0])
    assert fit['ok'].tolist() == [True, False] and fit['screen_calibrated'].tolist() == [True, False] and fit['kind'].tolist() == [1, 0]
    assert fit['used'].tolist() == [3, 0] and fit['solves'].tolist() == [1, 0]
    assert (fit['coef'][0, :, 0] - torch.tensor(SHIFT_MM, dtype=torch.float64)).abs().max() < 1e-3 and not fit['coef'][0, :, 1:].any()
    assert fit['rms_mm'][0] < 1e-3 and abs(float(fit['rms_mm_raw'][0]) - np.hypot(*SHIFT_MM)) < 1e-3 and fit['mean_deg_raw'][0] > 0.1
    coef, kind = s.get_screen_calibration()
    assert kind.tolist() == [1, 0] and torch.equal(coef[0], fit['coef'][0]) and not coef[1].any()
    # the applying step
    s.reset()
    del fake.calls[:]
    second = run(s, c0)
    assert fake.calls.count('screen_calib_apply') == 1 and 'screen_calib_append' not in fake.calls
    assert sorted(second) == sorted(list(p0) + ['PoG_px_final_raw', 'screen_calibrated'])
    assert second['screen_calibrated'].tolist() == [True, False] and torch.equal(second['PoG_px_final_raw'], p0['PoG_px_final'])
    want = ref.apply(p0['PoG_px_final'][0].numpy(), c0['pixels_per_millimeter'][0].numpy(), coef[0].numpy(), 1, size_of(model))
    assert second['PoG_px_final'][0].numpy().tobytes() == want.tobytes()
    assert (second['PoG_px_final'][0] - t0[0]).abs().max() < 1e-2                                    # it lands on the dots
    # PoG_cm_final and g_final follow by the existing expressions; everything else is untouched
    cm = second['PoG_px_final'] * (0.1 * c0['millimeters_per_pixel'])
    assert torch.equal(second['PoG_cm_final'][0], cm[0])
    N = B * T
    g = fake.combined_gaze(_mean2(c0['left_o'], c0['right_o']).reshape(N, 3), (10.0 * cm).reshape(N, 2), c0['left_R'].reshape(N, 3, 3),
                           c0['camera_transformation'].reshape(N, 4, 4)).view(B, T, 2)
    assert torch.equal(second['g_final'][0], g[0]) and not torch.equal(second['g_final'][0], p0['g_final'][0])
    for k in p0:
        assert torch.equal(second[k][1], p0[k][1]), k                   # the stream without a map: the plain bits
        if k not in ('PoG_px_final', 'PoG_cm_final', 'g_final'):
            assert torch.equal(second[k], p0[k]), k
    assert s.screen_calibration_counts()[0].tolist() == [3, 2]          # reset() and a plain step leave the store alone
    # collecting while the map is applied reads the uncorrected point: the same rows again
    s.clear_screen_calibration_samples([0])
    s.reset()
    third = run(s, dict(c0, screen_calibration_target=t0))
    assert s.screen_calibration_counts()[0].tolist() == [3, 5]
    assert np.array_equal(s.screen_calibration_samples()[0, :3].numpy(), rows[0])
    assert torch.equal(third['PoG_px_final'], second['PoG_px_final'])
    # the validation pass: the stored map over the store, nothing changes
    before = s.get_screen_calibration()
    ev = s.evaluate_screen_calibration()
    assert ev['ok'].tolist() == [True, True] and ev['solves'].tolist() == [0, 0] and ev['used'].tolist() == [3, 5]
    assert ev['rms_mm'][0] == fit['rms_mm'][0] and ev['rms_mm'][1] == ev['rms_mm_raw'][1] and ev['rms_mm_raw'][1] > 5.0
    assert all(torch.equal(a, b) for a, b in zip(before, s.get_screen_calibration()))
    assert s.evaluate_screen_calibration(streams=[1])['ok'].tolist() == [False, True]
    # a failed fit leaves the map the stream had; reset(), get_state() and set_state() do not touch it
    refused = s.fit_screen_calibration(model='quadratic')
    assert refused['ok'].tolist() == [False, False] and refused['kind'].tolist() == [1, 0] and refused['used'].tolist() == [3, 5]
    assert not s.fit_screen_calibration(model='offset', max_shift_mm=1.0)['ok'].any()
    s.reset()
    st = s.get_state()
    assert not any('screen' in k for k in st)
    s.set_state(st)
    assert all(torch.equal(a, b) for a, b in zip(before, s.get_screen_calibration()))
    s.clear_screen_calibration()
    s.reset()
    last = run(s, c0)
    assert sorted(last) == sorted(p0)
    for k in p0:
        assert torch.equal(last[k], p0[k]), k


def test_an_eyenet_only_model_corrects_the_initial_point(fake):
    model, _ = make_model(dict(refine_net_enabled=False))
    c0 = chunk_of(clip(B, T, size=32), 0, T)
    p0 = run(eve_amd.EVEStream(model, B, use_graph=False), c0)
    assert 'PoG_px_final' not in p0
    s = eve_amd.EVEStream(model, B, use_graph=False)
    run(s, dict(c0, screen_calibration_target=targets_of(p0['PoG_px_initial'], c0)))
    assert s.fit_screen_calibration(model='offset')['ok'].all()
    coef, kind = s.get_screen_calibration()
    s.reset()
    out = run(s, c0)
    assert sorted(out) == sorted(list(p0) + ['PoG_px_initial_raw', 'screen_calibrated'])
    for b in range(B):
        want = ref.apply(p0['PoG_px_initial'][b].numpy(), c0['pixels_per_millimeter'][b].numpy(), coef[b].numpy(), int(kind[b]), size_of(model))
        assert out['PoG_px_initial'][b].numpy().tobytes() == want.tobytes()
    assert torch.equal(out['PoG_cm_initial'], out['PoG_px_initial'] * (0.1 * c0['millimeters_per_pixel']))
    assert torch.equal(out['PoG_px_initial_raw'], p0['PoG_px_initial'])
    for k in p0:
        if k not in ('PoG_px_initial', 'PoG_cm_initial', 'g_initial'):
            assert torch.equal(out[k], p0[k]), k


def test_events_and_overlay_markers_read_the_corrected_point(fake, scene):
    from test_gaze_events_host import reference_on
    model, c0, _ = scene
    s = eve_amd.EVEStream(model, B, use_graph=False)
    coef = torch.zeros(B, 2, 6, dtype=torch.float64)
    coef[:, :, 0] = torch.tensor([30.0, -20.0])
    coef[:, 0, 1] = 12.0
    s.set_screen_calibration(coef, [2, 2])
    spec = GazeEventSpec(fps=30)
    out = run(s, c0, events=spec)
    assert fake.calls.index('screen_calib_apply') < fake.calls.index('gaze_events')
    assert not torch.equal(out['PoG_px_final'], out['PoG_px_final_raw'])
    want, _, _ = reference_on(out, c0, spec, 'PoG_px_final', np.zeros((B, 32)))
    for k in want:
        assert out[k].numpy().tobytes() == want[k].tobytes(), k
    from test_stream_ragged_host import CONFIGS, make_model as ragged_model
    model2 = ragged_model(*CONFIGS['gru-cgru'])
    Bc, Tc = 2, 2
    ch = stream_chunk(Bc, Tc)
    s2 = eve_amd.EVEStream(model2, Bc, use_graph=False)
    s2.set_screen_calibration(coef, [2, 0])
    overlay = OverlaySpec(markers=[dict(key='PoG_px_final', r_fill=3, r_outline=5), dict(key='PoG_px_final_raw', r_fill=2, r_outline=3)],
                          inset=None, out_format='rgb')
    del fake.calls[:]
    res = s2.step(ch, render=overlay)
    assert fake.calls.index('screen_calib_apply') < fake.calls.index('overlay_render')
    assert torch.equal(fake.last_centres[:, 0], res['PoG_px_final'].reshape(-1, 2))
    assert torch.equal(fake.last_centres[:, 1], res['PoG_px_final_raw'].reshape(-1, 2))
    assert not torch.equal(fake.last_centres[:Tc, 0], fake.last_centres[:Tc, 1]) and torch.equal(fake.last_centres[Tc:, 0], fake.last_centres[Tc:, 1])


def test_ragged_masked_and_overflow(fake, scene):
    model, c0, c1 = scene
    t0 = torch.full((B, T, 2), 500.0)
    s = eve_amd.EVEStream(model, B, use_graph=False, screen_calibration_capacity=4)
    run(s, dict(c0, screen_calibration_target=t0), lengths=[2, 0])
    assert s.screen_calibration_counts()[0].tolist() == [2, 0]
    mask = torch.ones(B, T, 2, dtype=torch.bool)
    mask[1, 1] = False                                                  # frame (1, 1) has no usable eye: not valid
    mask[1, 2, 0] = False                                               # one eye is enough
    run(s, dict(c1, screen_calibration_target=t0), eye_mask=mask)
    count, dropped = s.screen_calibration_counts()
    assert count.tolist() == [4, 2] and dropped.tolist() == [1, 0]
    s.clear_screen_calibration_samples()
    assert s.screen_calibration_counts()[0].tolist() == [0, 0] and s.screen_calibration_counts()[1].tolist() == [0, 0]
    # both collectors in one chunk
    run(s, dict(c0, screen_calibration_target=t0, calibration_target=t0))
    assert s.screen_calibration_counts()[0].tolist() == [3, 3] and s.calibration_counts()[0].tolist() == [[3, 3], [3, 3]]


def test_get_set_clear_round_trip(fake, scene):
    model, c0, _ = scene
    s = eve_amd.EVEStream(model, B, use_graph=False)
    coef = torch.arange(B * 12, dtype=torch.float64).reshape(B, 2, 6) + 1.0
    s.set_screen_calibration(coef, torch.tensor([3, 1]))
    got, kind = s.get_screen_calibration()
    assert kind.tolist() == [3, 1] and got.dtype == torch.float64 and torch.equal(got[0], coef[0])
    assert torch.equal(got[1, :, 0], coef[1, :, 0]) and not got[1, :, 1:].any()                     # unused terms are stored as 0
    s.set_screen_calibration(torch.zeros(B, 2, 6), [0, 2], streams=[1])
    assert s.get_screen_calibration()[1].tolist() == [3, 2] and torch.equal(s.get_screen_calibration()[0][0], coef[0])
    s.reset()
    assert s.get_screen_calibration()[1].tolist() == [3, 2]
    s.clear_screen_calibration([0])
    got, kind = s.get_screen_calibration()
    assert kind.tolist() == [0, 2] and not got[0].any() and s._screen_apply
    s.clear_screen_calibration()
    assert not s._screen_apply and not s.get_screen_calibration()[1].any()


def test_refusals(fake, scene):
    model, c0, _ = scene
    s = eve_amd.EVEStream(model, B, use_graph=False)
    t0 = torch.zeros(B, T, 2)
    without = lambda *keys: {k: v for k, v in c0.items() if k not in keys}
    with pytest.raises(ValueError, match='inv_camera_transformation'):
        s.step(dict(without('inv_camera_transformation'), screen_calibration_target=t0))
    with pytest.raises(ValueError, match='origins'):
        s.step(dict(without('left_o', 'right_o'), screen_calibration_target=t0))
    with pytest.raises(ValueError, match='screen_calibration_target'):
        s.step(dict(c0, screen_calibration_valid=torch.ones(B, T, dtype=torch.bool)))
    with pytest.raises(ValueError, match='screen_calibration_target'):
        s.step(dict(c0, screen_calibration_target=t0.double()))
    with pytest.raises(ValueError, match='screen_calibration_target'):
        s.step(dict(c0, screen_calibration_target=torch.zeros(B, T + 1, 2)))
    with pytest.raises(ValueError, match='screen_calibration_valid'):
        s.step(dict(c0, screen_calibration_target=t0, screen_calibration_valid=torch.ones(B, T)))
    with pytest.raises(ValueError, match='model'):
        s.fit_screen_calibration(model='cubic')
    with pytest.raises(ValueError, match='huber_mm'):
        s.fit_screen_calibration(huber_mm=0)
    with pytest.raises(ValueError, match='min_samples'):
        s.fit_screen_calibration(min_samples=0)
    with pytest.raises(ValueError, match='max_shift_mm'):
        s.fit_screen_calibration(max_shift_mm=-1)
    with pytest.raises(ValueError, match='coef'):
        s.set_screen_calibration(torch.zeros(B, 6), [1, 1])
    with pytest.raises(ValueError, match='kind'):
        s.set_screen_calibration(torch.zeros(B, 2, 6), [1, 4])
    with pytest.raises(ValueError, match='kind'):
        s.set_screen_calibration(torch.zeros(B, 2, 6), [1.0, 2.0])
    with pytest.raises(ValueError, match='screen_calibration_capacity'):
        eve_amd.EVEStream(model, B, use_graph=False, screen_calibration_capacity=0)
    assert not set(NEW_CALLS) & set(fake.calls) and not s._screen_apply
    s.set_screen_calibration(torch.zeros(B, 2, 6), [1, 1])
    with pytest.raises(ValueError, match='millimeters_per_pixel'):
        s.step(without('millimeters_per_pixel'))


def test_the_stored_map_survives_each_refusal_of_the_fit(fake):
    """Through the stand-in's store arguments, as the kernel handles them: where the fit is refused the stored map stays."""
    k = fake
    sentinel = torch.full((1, 2, 6), 7.0, dtype=torch.float64)
    cases = [(ref.make_scene(5, dots=(3, 1), per_dot=2, model='affine'), 2, {}),
             (ref.make_scene(5, dots=(5, 1), per_dot=2, model='quadratic'), 3, {}),
             (ref.make_scene(5, dots=(1, 1), per_dot=2, model='affine'), 2, {}),
             (ref.make_scene(5, dots=(3, 3), model='affine'), 2, dict(max_shift_mm=1.0))]
    for sc, kind, kw in cases:
        store, kinds = sentinel.clone(), torch.tensor([3], dtype=torch.uint8)
        rows = torch.from_numpy(ref.scene_rows(sc))[None]
        res = k.screen_calib_fit(rows, None, None, 0, kind, None, 1, kw.get('max_shift_mm', 100.0), store, kinds)
        assert not res[5].any() and torch.equal(store, sentinel) and kinds.tolist() == [3]
    store, kinds = sentinel.clone(), torch.tensor([3], dtype=torch.uint8)
    res = k.screen_calib_fit(rows, None, None, 0, 2, None, 1, 100.0, store, kinds)
    assert res[5].all() and torch.equal(store, res[0]) and kinds.tolist() == [2]
