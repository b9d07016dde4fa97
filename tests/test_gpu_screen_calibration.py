"""GPU: the screen-space gaze calibration -- eve_screen_calib_append, eve_screen_calib_fit (both modes) and eve_screen_calib_apply against
the numpy contract of tests/screen_calib_ref.py, bit for bit (the two degree outputs, which pass through atan2, at relative 1e-12),
and EVEStream's collect / fit / apply path around them (eager and captured).  Every test here needs the three entry points, so every
one fails on a library without them."""
import numpy as np
import pytest
import torch

import eve_amd
import screen_calib_ref as ref
from eve_amd import data
from eve_amd.data import SCREEN_CALIB_REPORT
from eve_amd.eve import _mean2
from eve_amd.kernels import default_kernels
from test_stream_host import chunk_of, clip, make_model

pytestmark = pytest.mark.gpu
GUARD = 64
SENT, ISENT = -777.25, -7
DEG = ('mean_deg', 'mean_deg_raw')


def guarded(shape, dtype, sentinel):
    """-> (the whole buffer, its payload as a contiguous view): GUARD sentinel elements on either side of the payload."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device='cuda')
    return whole, whole[GUARD:GUARD + n].view(shape)


def guards_hold(whole, sentinel):
    return bool((whole[:GUARD] == sentinel).all()) and bool((whole[-GUARD:] == sentinel).all())


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ---------------------------------------------------------------------------------------------------------------- append
@pytest.mark.parametrize('T', [1, 5, 70])
@pytest.mark.parametrize('B', [1, 3])
def test_append_matches_the_reference_bit_for_bit(B, T):
    """Validity and frame_valid holes, ragged lengths with a 0, NaN inputs, ppm = 0, an eye in the screen plane, into a store of
    C = 4 that overflows and one that holds everything; a store that starts part full.  Rows, counts and dropped are exact."""
    k = default_kernels()
    sc = ref.make_scene(40 + 7 * B + T, dots=(T, B), noise_mm=6.0, model='quadratic')
    N = B * T
    pog, origin, inv_cam, ppm, target = (sc[n].copy() for n in ('pog', 'origin', 'inv_cam', 'ppm', 'target'))
    valid, frame_valid = np.ones((B, T), dtype=np.uint8), np.ones((B, T), dtype=np.uint8)
    lengths = np.full(B, T, dtype=np.int32)
    if T >= 5:
        target[1, 0] = np.nan
        pog[2, 1] = np.inf
        ppm[3, 1] = 0.0
        origin[4], inv_cam[4, 2, 3] = 0.0, 0.0
        valid[0, 0] = 0
        frame_valid[B - 1, T - 1] = 0
    if T == 70:
        inv_cam[9, 0, 1], origin[11, 2] = np.nan, np.nan
        valid[0, 64:66] = 0
    if B == 3:
        lengths[:] = [T, 0, max(T - 1, 1)]
    rows, usable = ref.reduce(pog, origin, inv_cam, ppm, target, sc['screen_size'])
    for C, start in ((4, 0), (N + 2, 1)):
        s_whole, samples = guarded((B, C, 12), torch.float64, SENT)
        c_whole, count = guarded((B,), torch.int32, ISENT)
        d_whole, dropped = guarded((B,), torch.int32, ISENT)
        count.fill_(start)
        dropped.zero_()
        shape = lambda a, *s: cuda(a.reshape((B, T) + s))
        k.screen_calib_append(shape(pog, 2), shape(origin, 3), shape(inv_cam, 4, 4), shape(ppm, 2), shape(target, 2), sc['screen_size'],
                              samples, count, dropped, cuda(valid), cuda(lengths), cuda(frame_valid))
        torch.cuda.synchronize()
        got, got_count, got_dropped = samples.cpu().numpy(), count.cpu().numpy(), dropped.cpu().numpy()
        for b in range(B):
            want = [rows[b * T + t] for t in range(lengths[b]) if valid[b, t] and frame_valid[b, t] and usable[b * T + t]]
            kept = min(len(want), C - start)
            assert got_count[b] == start + kept and got_dropped[b] == len(want) - kept, (C, b)
            if kept:
                assert bits(got[b, start:start + kept], np.stack(want[:kept])), (C, b)
            untouched = np.ones(C, dtype=bool)
            untouched[start:start + kept] = False
            assert (got[b, untouched] == SENT).all(), (C, b)
        assert guards_hold(s_whole, SENT) and guards_hold(c_whole, ISENT) and guards_hold(d_whole, ISENT)
    if T >= 5:
        assert usable[:5].tolist() == [True, False, False, False, False]
    # without the optional arguments every usable frame is appended
    samples = torch.zeros((B, N, 12), dtype=torch.float64, device='cuda')
    count, dropped = torch.zeros(B, dtype=torch.int32, device='cuda'), torch.zeros(B, dtype=torch.int32, device='cuda')
    k.screen_calib_append(shape(pog, 2), shape(origin, 3), shape(inv_cam, 4, 4), shape(ppm, 2), shape(target, 2), sc['screen_size'],
                          samples, count, dropped)
    assert count.tolist() == [int(usable[b * T:(b + 1) * T].sum()) for b in range(B)] and not dropped.any()


def test_screen_calibration_samples_rows_line_up_with_their_frames():
    sc = ref.make_scene(31, dots=(4, 2), model='affine')
    sc['target'][2, 1] = np.nan
    rows, usable = ref.reduce(sc['pog'], sc['origin'], sc['inv_cam'], sc['ppm'], sc['target'], sc['screen_size'])
    got = data.screen_calibration_samples(cuda(sc['pog']), cuda(sc['origin']), cuda(sc['inv_cam']), cuda(sc['ppm']), cuda(sc['target']),
                                          sc['screen_size']).cpu().numpy()
    assert usable.tolist() == [True, True, False] + [True] * 5 and (got[2] == 0.0).all() and bits(got[usable], rows[usable])
    fit = data.fit_screen_map(torch.from_numpy(got).cuda())
    want = ref.fit(rows[usable], 'affine')
    assert bool(fit['ok']) and int(fit['used']) == 7 and int(fit['kind']) == 2 and bits(fit['coef'].cpu().numpy(), want['coef'])
    ev = data.evaluate_screen_map(torch.from_numpy(got).cuda(), fit['coef'], 2)
    assert bool(ev['ok']) and float(ev['rms_mm']) == float(fit['rms_mm']) == want['rms_mm']
    px = data.apply_screen_map(cuda(sc['pog']), cuda(sc['ppm']), fit['coef'], 2, sc['screen_size']).cpu().numpy()
    assert bits(px, ref.apply(sc['pog'], sc['ppm'], want['coef'], 2, sc['screen_size']))
    assert np.abs(px[usable] - sc['target'][usable]).max() < 1e-2


# ---------------------------------------------------------------------------------------------------------------- fit
def stores(row_sets, cap):
    """Row sets of different lengths -> (samples float64 [S, cap, 12] with garbage past each count, count int32 [S])."""
    s = np.full((len(row_sets), cap, 12), np.nan)
    for q, rows in enumerate(row_sets):
        s[q, :len(rows)] = rows
    return cuda(s), cuda(np.array([len(r) for r in row_sets], dtype=np.int32))


def check_against(res, want, stores_after=None, stores_before=None, kind=None):
    """res: screen_calib_fit's tuple; want: the reference's dicts, one per stream."""
    coef, report, used, inliers, solves, ok = (t.cpu().numpy() for t in res)
    for q, w in enumerate(want):
        tag = (q, w['ok'], w['used'], w['solves'])
        assert bool(ok[q]) == w['ok'] and used[q] == w['used'] and inliers[q] == w['inliers'] and solves[q] == w['solves'], tag
        assert bits(coef[q], w['coef']), tag
        for i, name in enumerate(SCREEN_CALIB_REPORT):
            if name in DEG:
                assert abs(report[q, i] - w[name]) <= 1e-12 * abs(w[name]), (tag, name, report[q, i], w[name])
            else:
                assert report[q, i] == w[name], (tag, name, report[q, i], w[name])
        if stores_after is not None:
            c_after, k_after = (t.cpu().numpy() for t in stores_after)
            if w['ok']:
                assert bits(c_after[q], w['coef']) and k_after[q] == kind, tag
            else:
                assert bits(c_after[q], stores_before[0][q]) and k_after[q] == stores_before[1][q], tag


NOISY = dict(dots=(5, 3), per_dot=9, noise_mm=8.0, outliers=13)


def shuffled_rows(seed, model):
    rows = ref.scene_rows(ref.make_scene(seed, model=model, **NOISY))
    return rows[np.random.RandomState(seed).permutation(rows.shape[0])]


@pytest.mark.parametrize('huber', [None, 25.0])
@pytest.mark.parametrize('model', ['offset', 'affine', 'quadratic'])
def test_fit_matches_the_reference_bit_for_bit(model, huber):
    """One launch of eight streams: n = 0, 1, K - 1, K, 63, 64, 65 and 130 rows (none, fewer than the terms, exactly the terms, one
    and two and three rows per lane) of a scene with 8 mm of noise and 10 % outliers, shuffled.  coef, used, inliers, solves, ok,
    the six millimetre numbers and the stores equal the reference; so do the refusals among them (max_shift_mm 400, as in the host
    suite's Huber test: the quadratic at an outlier far off the screen)."""
    kind = ref.KINDS[model]
    K = ref.terms_of(kind)
    rows = shuffled_rows(60 + kind, model)
    sets = [rows[:n] for n in (0, 1, K - 1, K, 63, 64, 65, 130)]
    samples, count = stores(sets, 130)
    c_whole, c_store = guarded((8, 2, 6), torch.float64, SENT)
    k_whole, k_store = guarded((8,), torch.uint8, 9)
    before = (c_store.cpu().numpy(), k_store.cpu().numpy())
    res = default_kernels().screen_calib_fit(samples, count, None, 0, kind, huber, 1, 400.0, c_store, k_store)
    torch.cuda.synchronize()
    want = [ref.fit(r, kind, huber, None, 400.0) for r in sets]
    assert [w['ok'] for w in want][-4:] == [True] * 4 and not want[0]['ok'] and (K == 1 or not want[2]['ok'])
    if huber is not None:
        assert max(w['solves'] for w in want) > 2
    check_against(res, want, (c_store, k_store), before, kind)
    assert guards_hold(c_whole, SENT) and guards_hold(k_whole, 9)


@pytest.mark.parametrize('S', [1, 3])
def test_fit_select_absent_rows_and_the_refusals(S):
    """select = 0 leaves a stream alone; rows of weight 0 are absent; count = None reads all C rows; dots on one line ('affine'), a
    5 x 1 row ('quadratic'), fewer rows than min_samples and a map past max_shift_mm are refused as the reference refuses them, and
    leave the stored map."""
    k = default_kernels()
    rows = shuffled_rows(77, 'affine')[:40].copy()
    rows[5:12, 9] = 0.0                                                   # absent
    rows[20, 9] = -1.0
    sets = [rows, rows[:30], rows[:12]][:S]
    select = np.array([1, 0, 1], dtype=np.uint8)[:S]
    samples, count = stores(sets, 40)
    c_store, k_store = torch.full((S, 2, 6), 3.5, dtype=torch.float64, device='cuda'), torch.full((S,), 3, dtype=torch.uint8, device='cuda')
    before = (c_store.cpu().numpy(), k_store.cpu().numpy())
    res = k.screen_calib_fit(samples, count, cuda(select), 0, 2, 25.0, 1, 400.0, c_store, k_store)
    none = dict(ref.fit(rows[:0], 2), used=0)
    want = [ref.fit(r, 2, 25.0, None, 400.0) if select[q] else none for q, r in enumerate(sets)]
    assert want[0]['ok'] and want[0]['used'] == 32
    check_against(res, want, (c_store, k_store), before, 2)
    # count = None: all C rows, here exactly the first set
    res = k.screen_calib_fit(samples[:1].contiguous(), None, None, 0, 2, 25.0, 1, 400.0)
    check_against(res, want[:1])
    far = ref.coef_star('affine')
    far[0, 0] = 150.0
    cases = [(ref.make_scene(5, dots=(3, 1), per_dot=2, model='affine'), 2, 1, 100.0),
             (ref.make_scene(5, dots=(5, 1), per_dot=2, model='quadratic'), 3, 1, 100.0),
             (ref.make_scene(5, dots=(3, 3), model='affine'), 2, 10, 100.0),
             (ref.make_scene(5, dots=(3, 3), model='affine', coef=far), 2, 1, 100.0),
             (ref.make_scene(5, dots=(3, 3), model='affine', coef=far), 2, 1, 400.0)]
    for i, (sc, kind, min_samples, max_shift) in enumerate(cases):
        r = ref.scene_rows(sc)
        samples, count = stores([r] * S, r.shape[0])
        c_store.fill_(3.5), k_store.fill_(3)
        res = k.screen_calib_fit(samples, count, None, 0, kind, None, min_samples, max_shift, c_store, k_store)
        want = ref.fit(r, kind, None, min_samples, max_shift)
        assert want['ok'] == (i == 4), i
        check_against(res, [want] * S, (c_store, k_store), before, kind)


def test_mode_1_matches_evaluate_and_changes_nothing():
    """Four streams holding no map, an offset, an affine and a quadratic map, over 130, 5, 65 and 0 rows: the report of the stored
    maps; kind 0 reports the raw numbers in both sets; the stores keep their bits."""
    rows = shuffled_rows(91, 'quadratic')
    sets = [rows[:130], rows[:5], rows[:65], rows[:0]]
    samples, count = stores(sets, 130)
    coef = np.stack([np.full((2, 6), 99.0), ref.coef_star('offset'), ref.coef_star('affine'), ref.coef_star('quadratic')])
    kinds = np.array([0, 1, 2, 3], dtype=np.uint8)
    c_store, k_store = cuda(coef), cuda(kinds)
    res = default_kernels().screen_calib_fit(samples, count, None, 1, 0, None, 1, 100.0, c_store, k_store)
    want = [ref.evaluate(r, coef[q], kinds[q]) for q, r in enumerate(sets)]
    assert [w['ok'] for w in want] == [True, True, True, False]
    check_against(res, want)
    report = res[1].cpu().numpy()
    assert bits(report[0, :4], report[0, 4:]) and not bits(report[2, :4], report[2, 4:])
    assert bits(c_store.cpu().numpy(), coef) and bits(k_store.cpu().numpy(), kinds)
    with pytest.raises(ValueError, match='mode'):
        default_kernels().screen_calib_fit(samples, count, None, 1)


# ---------------------------------------------------------------------------------------------------------------- apply
@pytest.mark.parametrize('B,T', [(1, 1), (1, 65), (3, 70)])
def test_apply_matches_the_reference_bit_for_bit(B, T):
    """Mixed kinds per stream, points that the map pushes over all four edges of the screen, a NaN row, kind 0 (and a kind byte out
    of range) returning the input bits."""
    rng = np.random.RandomState(B * 100 + T)
    px = np.stack([rng.uniform(-50, 1970, (B, T)), rng.uniform(-50, 1130, (B, T))], axis=-1).astype(np.float32)
    ppm = np.tile(np.array([3.4, 3.5], dtype=np.float32), (B, T, 1))
    if T >= 8:
        px[0, 0], px[0, 1], px[0, 2], px[0, 3] = (2.0, 500.0), (1918.0, 500.0), (900.0, 1.0), (900.0, 1079.0)
        px[0, 4, 0], px[0, 5, 1] = np.nan, np.nan
        px[0, 6] = (-0.0, 0.0)
    coef = np.stack([ref.coef_star(m) for m in ('quadratic', 'affine', 'offset')])[:B] * 3.0
    for kinds in ([3, 0, 1], [1, 2, 7], [0, 0, 0], [2, 3, 3]):
        kinds = np.array(kinds[:B], dtype=np.uint8)
        whole, out = guarded((B, T, 2), torch.float32, SENT)
        got = default_kernels().screen_calib_apply(cuda(px), cuda(ppm), cuda(coef), cuda(kinds), ref.SCREEN).cpu().numpy()
        for b in range(B):
            want = ref.apply(px[b], ppm[b], coef[b], kinds[b], ref.SCREEN)
            assert bits(got[b], want), (kinds.tolist(), b)
            if kinds[b] in (0, 7):
                assert bits(got[b], px[b])
    if T >= 8:
        edge = ref.apply(px[0], ppm[0], coef[0], 3, ref.SCREEN)
        back = ref.apply(px[0], ppm[0], -coef[0], 3, ref.SCREEN)
        hit = np.concatenate([edge[:4].reshape(-1), back[:4].reshape(-1)])
        assert {0.0, 1920.0, 1080.0} <= set(hit.tolist())                # the clamp is exercised on every edge
        assert np.isnan(edge[4, 0]) and np.isnan(edge[5, 1])


# ---------------------------------------------------------------------------------------------------------------- EVEStream
S, TC = 3, 2


def rig_for(over):
    model, _ = make_model(over)
    model = model.cuda()
    batch = clip(S, 4 * TC, seed=7)
    d = {k: v.cuda() for k, v in chunk_of(batch, 0, 4 * TC).items()}
    chunk = lambda i: {k: v[:, i * TC:(i + 1) * TC].contiguous() for k, v in d.items()}
    keep = lambda out: {k: v.clone() for k, v in out.items()}
    twin = eve_amd.EVEStream(model, S, use_graph=False)
    plain = [keep(twin.step(chunk(i))) for i in range(4)]                # the uncorrected results, chunk by chunk
    return {'model': model, 'chunk': chunk, 'keep': keep, 'plain': plain, 'size': tuple(model.config.actual_screen_size)}


@pytest.fixture(scope='module')
def refined():
    return rig_for(dict(refine_net_rnn_type='CGRU'))


@pytest.fixture(scope='module')
def eye_only():
    return rig_for(dict(refine_net_enabled=False))


def forward_map(px, ppm, coef, kind, size):
    """Targets: the known map applied to the uncorrected points, without the clamp (numpy, float64 -> float32)."""
    x, s = px.cpu().numpy().astype(np.float64), ppm.cpu().numpy().astype(np.float64)
    u, v = (x[..., 0] + x[..., 0]) / size[0] - 1.0, (x[..., 1] + x[..., 1]) / size[1] - 1.0
    p = ref.shift(ref.phi_of(u, v), coef, ref.terms_of(kind))
    return cuda((x + np.stack(p, axis=-1) * s).astype(np.float32))


def end_to_end(rig, suffix, model_name, star, use_graph):
    """Collect over three chunks of 3 x 2 frames against targets made from the twin's uncorrected points by the known map, fit, and
    judge the fourth chunk's step: the corrected point has the bits the reference predicts from the store read back, PoG_cm and g
    equal the existing expressions on it, everything else keeps the twin's bits."""
    model, size, kind = rig['model'], rig['size'], ref.KINDS[model_name]
    key = 'PoG_px_' + suffix
    stream = eve_amd.EVEStream(model, S, use_graph=use_graph, screen_calibration_capacity=16)
    targets = []
    for i in range(3):
        c = rig['chunk'](i)
        targets.append(forward_map(rig['plain'][i][key], c['pixels_per_millimeter'], star, kind, size))
        out = stream.step(dict(c, screen_calibration_target=targets[-1]))
        for k in rig['plain'][i]:                      # collecting changes no result
            assert torch.equal(out[k], rig['plain'][i][k]), k
    count, dropped = stream.screen_calibration_counts()
    assert count.tolist() == [3 * TC] * S and not dropped.any()
    store = stream.screen_calibration_samples().cpu().numpy()
    want = [ref.fit(store[b, :3 * TC], kind) for b in range(S)]
    assert all(w['ok'] for w in want), [w['ok'] for w in want]           # the reference's own fit, before the device is judged
    fit = stream.fit_screen_calibration(model=model_name)
    assert fit['ok'].all() and fit['screen_calibrated'].all() and fit['kind'].tolist() == [kind] * S
    coef, kinds = stream.get_screen_calibration()
    for b in range(S):
        assert bits(fit['coef'][b].cpu().numpy(), want[b]['coef']) and bits(coef[b].cpu().numpy(), want[b]['coef'])
        assert float(fit['rms_mm'][b]) == want[b]['rms_mm'] and float(fit['rms_mm_raw'][b]) == want[b]['rms_mm_raw']
    c, plain = rig['chunk'](3), rig['plain'][3]
    out = rig['keep'](stream.step(c))
    assert sorted(out) == sorted(list(plain) + [key + '_raw', 'screen_calibrated'])
    assert out['screen_calibrated'].all() and torch.equal(out[key + '_raw'], plain[key])
    for b in range(S):
        pred = ref.apply(plain[key][b].cpu().numpy(), c['pixels_per_millimeter'][b].cpu().numpy(), want[b]['coef'], kind, size)
        assert bits(out[key][b].cpu().numpy(), pred), b
    cm = out[key] * (0.1 * c['millimeters_per_pixel'])
    N = S * TC
    g = default_kernels().combined_gaze(_mean2(c['left_o'], c['right_o']).reshape(N, 3).float(), (10.0 * cm).reshape(N, 2),
                                        c['left_R'].reshape(N, 3, 3).float(), c['camera_transformation'].reshape(N, 4, 4).float()).view(S, TC, 2)
    assert torch.equal(out['PoG_cm_' + suffix], cm) and torch.equal(out['g_' + suffix], g)
    for k in plain:
        if k not in (key, 'PoG_cm_' + suffix, 'g_' + suffix):
            assert torch.equal(out[k], plain[k]), k
    held_out = forward_map(plain[key], c['pixels_per_millimeter'], star, kind, size)
    inside = ((held_out >= 0) & (held_out <= torch.tensor(size, device='cuda', dtype=torch.float32))).all(dim=-1)
    dist = ((out[key] - held_out) / c['pixels_per_millimeter']).norm(dim=-1)
    raw = ((plain[key] - held_out) / c['pixels_per_millimeter']).norm(dim=-1)
    print('%s / %s (graph %s): corrected point to held-out targets %.3g mm max over %d frames on the screen (uncorrected %.3g mm); fit rms %s mm'
          % (suffix, model_name, use_graph, float(dist[inside].max()) if inside.any() else float('nan'), int(inside.sum()),
             float(raw[inside].max()) if inside.any() else float('nan'), ['%.3g' % float(v) for v in fit['rms_mm']]))
    return stream


def test_offset_on_a_refinenet_stream_end_to_end(refined):
    star = np.zeros((2, 6))
    star[:, 0] = (6.0, -4.0)
    end_to_end(refined, 'final', 'offset', star, use_graph=True)


def test_affine_on_an_eyenet_only_stream_end_to_end(eye_only):
    star = np.zeros((2, 6))
    star[:, :3] = [[6.0, -9.0, 4.0], [-4.0, 5.0, 8.0]]
    end_to_end(eye_only, 'initial', 'affine', star, use_graph=False)


def test_graph_replay_equals_eager_and_a_stream_without_a_map_keeps_its_bits(refined):
    """One applying AND collecting step, captured and replayed against eager; stream 1 holds no map and keeps the twin's bits."""
    model, c, plain = refined['model'], refined['chunk'](0), refined['plain'][0]
    coef = torch.zeros((S, 2, 6), dtype=torch.float64)
    coef[:, :, 0] = torch.tensor([25.0, -15.0])
    coef[:, 0, 1], coef[:, 1, 5] = 14.0, -9.0
    target = torch.full((S, TC, 2), 700.0, device='cuda')
    valid = torch.ones((S, TC), dtype=torch.bool, device='cuda')
    valid[2, 0] = False
    outs, rows = [], []
    for use_graph in (False, True):
        s = eve_amd.EVEStream(model, S, use_graph=use_graph, screen_calibration_capacity=4)
        s.set_screen_calibration(coef, [3, 0, 2])
        step = lambda: s.step(dict(c, screen_calibration_target=target, screen_calibration_valid=valid), lengths=[2, 2, 1])
        first = refined['keep'](step())
        assert s.screen_calibration_counts()[0].tolist() == [2, 2, 0]    # the capture's warm-up steps appended nothing of their own
        s.reset()
        outs.append(refined['keep'](step()))                             # (a replay, under use_graph)
        count, dropped = s.screen_calibration_counts()
        assert count.tolist() == [4, 4, 0] and not dropped.any()
        rows.append(s.screen_calibration_samples())
        for k in first:
            assert torch.equal(first[k], outs[-1][k]), k
    eager, graph = outs
    assert sorted(eager) == sorted(graph) and torch.equal(rows[0], rows[1])
    for k in eager:
        assert torch.equal(eager[k], graph[k]), k
    assert eager['screen_calibrated'].tolist() == [True, False, True]
    for k in plain:
        assert torch.equal(eager[k][1], plain[k][1]), k
    assert not torch.equal(eager['PoG_px_final'][0], plain['PoG_px_final'][0])
    # the store holds the UNCORRECTED point
    want, usable = ref.reduce(plain['PoG_px_final'][0].cpu().numpy(), _mean2(c['left_o'], c['right_o'])[0].cpu().numpy(),
                              c['inv_camera_transformation'][0].cpu().numpy(), c['pixels_per_millimeter'][0].cpu().numpy(),
                              target[0].cpu().numpy(), refined['size'])
    assert usable.all() and bits(rows[0][0, :2].cpu().numpy(), want) and bits(rows[0][0, 2:4].cpu().numpy(), want)
