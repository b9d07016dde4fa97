"""CPU: pupillometry -- the numpy contract (tests/pupil_ref.py) against an independent, slow formulation and its own properties, chunk
splits, eve_amd.PupilSpec, and the EVEStream plumbing (step(pupil=...), the refusals, the graph key, reset, the light response, the
readouts) over a stand-in whose pupil_track is the reference itself.  The GPU suite (test_gpu_pupil.py) checks the HIP kernel."""
import numpy as np
import pytest
import torch

import pupil_ref as ref
import eve_amd
from eve_amd import data, kernels
from eve_amd.data import PupilSpec
from test_gaze_events_host import EventOverlayFakes
from test_stream_host import chunk_of, clip, make_model

FLOATS = ref.KEYS[:5]
D = 1.0 / 32.0                                           # the exact scenes' frame period


def dyadic_cutoff(rc):
    """cutoff_hz for which the contract's 1 / (6.283185307179586 * cutoff_hz) is exactly rc."""
    c = np.float64(1.0) / (ref.TWO_PI * np.float64(rc))
    for _ in range(8):
        for cand in (c, np.nextafter(c, 0), np.nextafter(c, np.inf)):
            if np.float64(1.0) / (ref.TWO_PI * cand) == rc:
                return float(cand)
        c = np.nextafter(c, np.inf)
    raise AssertionError('no cutoff gives rc = %r exactly' % rc)


def exact_spec(**kw):
    """Every coefficient dyadic at a frame period of 1/32 s: the filter's a, the light's al and the offset's rate are 1/2."""
    base = dict(min_mm=1.0, max_mm=8.0, max_speed_mm_s=32.0, max_gap_s=3 * D, offset_rate=0.5, cutoff_hz=dyadic_cutoff(D), light_tau_s=D,
                dilate_mm_s=1.0, constrict_mm_s=1.0, min_amplitude_mm=0.0625)
    return ref.Spec(**dict(base, **kw))


# ---------------------------------------------------------------------------------------------------------------- the slow formulation
def slow_run(spec, sc, light, capacity, marks=None, tau=None):
    """From fresh state, no reset, flushed at the end.  Per frame brute force over explicit histories, in other algebra than the
    contract's (a = dt / (dt + rc), x + a * (y - x), the speed test multiplied out); then the tallies and the episodes rebuilt from the
    list of samples.  -> (outputs as float64 / ints, table, episodes as a list per stream, dropped)."""
    left, right, tt_all, ev, lum_all, lengths = sc['left'], sc['right'], sc['frame_time'], sc['eye_valid'], sc.get('luminance'), sc['lengths']
    B, T = left.shape
    out = {k: np.full((B, T), np.nan) for k in FLOATS}
    out.update(valid=np.zeros((B, T), np.uint8), eye_used=np.zeros((B, T, 2), np.uint8), eye_reason=np.zeros((B, T, 2), np.uint8), event=np.zeros((B, T), np.uint8))
    table, episodes, dropped = np.zeros((B, 24)), [], np.zeros(B, np.int32)
    rc = 1.0 / (2.0 * np.pi * spec.cutoff_hz)
    for b in range(B):
        samples, accepted, lums, off, rejects = [], ([], []), [], None, np.zeros((2, 3))
        base, prev_mark, run_values = None, False, []
        for f in range(int(lengths[b])):
            tt = tt_all[b, f]
            if not np.isfinite(tt) or (samples and not tt > samples[-1]['t']):
                continue
            if lum_all is not None and np.isfinite(lum_all[b, f]) and (not lums or tt > lums[-1][0]):
                lum = np.float64(lum_all[b, f])
                if not lums or tt - lums[-1][0] > spec.max_gap_s:
                    lums.append((tt, lum))
                else:
                    dtl = tt - lums[-1][0]
                    lums.append((tt, lums[-1][1] + dtl / (dtl + spec.light_tau_s) * (lum - lums[-1][1])))
            values = []
            for e, side in enumerate((left, right)):
                v, why = np.float64(side[b, f]), 0
                if not ev[b, f, e]:
                    why = 1
                elif not np.isfinite(v):
                    why = 2
                elif v < spec.min_mm or v > spec.max_mm:
                    why = 4
                elif accepted[e] and tt - accepted[e][-1][0] <= spec.max_gap_s and \
                        abs(v - accepted[e][-1][1]) > spec.max_speed_mm_s * (tt - accepted[e][-1][0]):
                    why = 8
                out['eye_reason'][b, f, e] = why
                if why > 1:
                    rejects[e, (2, 4, 8).index(why)] += 1
                values.append(v if why == 0 else None)
            mark = marks is not None and bool(marks[b, f])
            if values[0] is not None or values[1] is not None:
                l, r = values
                if l is not None and r is not None:
                    off = l - r if off is None else (1.0 - spec.offset_rate) * off + spec.offset_rate * (l - r)
                    d = (l + r) / 2.0
                elif l is not None:
                    d = l if off is None else l - off / 2.0
                else:
                    d = r if off is None else r + off / 2.0
                connected = bool(samples) and not tt - samples[-1]['t'] > spec.max_gap_s
                if connected:
                    dt = tt - samples[-1]['t']
                    df = samples[-1]['df'] + dt / (dt + rc) * (d - samples[-1]['df'])
                    vel = (df - samples[-1]['df']) / dt
                else:
                    dt, df, vel = (tt - samples[-1]['t'] if samples else None), d, np.nan
                lit = lum_all is not None and bool(lums)
                dc = df - light[b, 1] * (lums[-1][1] - light[b, 2]) if lit and light[b, 0] != 0 else df
                if marks is not None:
                    if mark:
                        if not prev_mark:
                            run_values = []
                        run_values.append(dc)
                        base = run_values[0] + sum(v - run_values[0] for v in run_values) / len(run_values)
                elif tau:
                    base = dc if base is None else base + dt / (dt + tau) * (dc - base)
                if base is not None:
                    out['change_mm'][b, f], out['change_pct'][b, f] = dc - base, 100.0 * (dc - base) / base
                phase = 1 if vel > spec.dilate_mm_s else (-1 if vel < -spec.constrict_mm_s else 0)
                samples.append(dict(f=f, t=tt, d=d, df=df, dc=dc, vel=vel, dt=dt, connected=connected, phase=phase, kind=(l is not None) + 2 * (r is not None),
                                    lf=lums[-1][1] if lit else None))
                for e in range(2):
                    if values[e] is not None:
                        accepted[e].append((tt, values[e]))
                out['mm'][b, f], out['raw_mm'][b, f], out['velocity'][b, f], out['valid'][b, f] = dc, d, vel, 1
                out['eye_used'][b, f] = (l is not None, r is not None)
                out['event'][b, f] = {1: 1, -1: 2, 0: 0}[phase]
            prev_mark = mark
        # ---- the tallies from the list of samples
        tab = table[b]
        tab[0] = sum(s['dt'] for s in samples if s['connected'])
        tab[1] = sum(s['dt'] for i, s in enumerate(samples) if s['connected'] and s['f'] - samples[i - 1]['f'] != 1)
        tab[2], tab[3], tab[4] = (sum(1 for s in samples if s['kind'] == k) for k in (3, 1, 2))
        tab[5:11] = rejects.reshape(-1)
        if samples:
            dcs = np.array([s['dc'] for s in samples])
            tab[11], tab[12], tab[13], tab[14], tab[15] = dcs[0], sum(dcs - dcs[0]), sum((dcs - dcs[0]) ** 2), dcs.min(), dcs.max()
        pairs = [(s['lf'], s['df']) for s in samples if s['lf'] is not None]
        if pairs:
            x, y = np.array(pairs).T
            x, y = x - x[0], y - y[0]
            tab[16:24] = (len(pairs), pairs[0][0], pairs[0][1], sum(x), sum(y), sum(x * x), sum(x * y), sum(y * y))
        # ---- the episodes: maximal runs of connected samples in one non-zero phase, each begun at the sample before its first
        runs = []
        for i, s in enumerate(samples):
            if s['phase'] == 0:
                continue
            if runs and runs[-1][-1] == i - 1 and samples[i - 1]['phase'] == s['phase']:
                runs[-1].append(i)
            else:
                runs.append([i])
        rows = []
        for run in runs:
            first, last, before = samples[run[0]], samples[run[-1]], samples[run[0] - 1]
            if abs(last['df'] - before['df']) >= spec.min_amplitude_mm:
                rows.append((first['phase'], before['t'], last['t'], before['df'], last['df'], max(abs(samples[i]['vel']) for i in run), len(run),
                             0.0 if first['lf'] is None else first['lf']))
        dropped[b] = max(len(rows) - capacity, 0)
        episodes.append(np.array(rows[:capacity]).reshape(-1, 8))
    return out, table, episodes, dropped


def exact_scene():
    """B = 2, T = 48 at 32 Hz: four blocks of at most ten frames between holes (both eyes withheld, luminance NaN) longer than
    max_gap_s, so that no value ever needs more than 53 bits.  Sizes in eighths with a constant left - right difference per stream,
    single-eye frames (the withheld eye holds NaN or garbage), one range reject, one speed reject, integer luminance."""
    rng = np.random.RandomState(3)
    B, T = 2, 48
    c = 4.0 + np.cumsum(rng.randint(-2, 3, (B, T)), axis=1) / 8.0
    c = np.clip(c, 2.0, 6.0)
    left, right = (c + np.array([[0.125], [-0.25]])).astype(np.float32), (c - np.array([[0.125], [-0.25]])).astype(np.float32)
    ev = np.ones((B, T, 2), np.uint8)
    lum = rng.randint(10, 21, (B, T)).astype(np.float32)
    for a, z in ((10, 14), (23, 28), (38, 42)):
        ev[:, a:z] = 0
        lum[:, a:z] = np.nan
        left[:, a:z], right[:, a:z] = np.nan, 1e30
    ev[0, 3:5, 1] = 0
    right[0, 3:5] = np.nan
    ev[1, 16:19, 0] = 0
    left[1, 16:19] = -7.0
    left[0, 30] = 16.0                                   # range
    right[1, 32] = right[1, 31] + 2.0                    # speed: 64 mm/s
    tt = np.arange(T)[None] * D + np.array([[0.0], [64.0]])
    return dict(left=left, right=right, frame_time=tt, eye_valid=ev, luminance=lum, lengths=np.array([48, 40], np.int32))


def random_scene(seed, B=3, T=120):
    """Sizes that wander with noise and an inter-eye difference that drifts, on a jittered clock with gaps, a stall, a step backwards
    and a NaN; withheld eyes (garbage behind them), spikes, values out of range; a luminance with NaNs; marks in runs."""
    rng = np.random.RandomState(seed)
    c = 4.0 + np.cumsum(rng.normal(0, 0.03, (B, T)), axis=1) + 0.5 * np.sin(np.arange(T) / 9.0)[None]
    diff = 0.2 + np.cumsum(rng.normal(0, 0.002, (B, T)), axis=1)
    left, right = (c + diff / 2 + rng.normal(0, 0.01, (B, T))).astype(np.float32), (c - diff / 2 + rng.normal(0, 0.01, (B, T))).astype(np.float32)
    left[rng.rand(B, T) < 0.04] += 1.5                   # spikes
    right[rng.rand(B, T) < 0.03] = 12.0
    left[rng.rand(B, T) < 0.02] = np.nan
    ev = (rng.rand(B, T, 2) > 0.12).astype(np.uint8)
    ev[0, 40:52] = 0
    ev[1, 60:64, 0] = 0
    left[ev[..., 0] == 0] = np.where(rng.rand((ev[..., 0] == 0).sum()) < 0.5, np.nan, 1e9)
    dt = rng.uniform(0.028, 0.038, (B, T))
    dt[rng.rand(B, T) < 0.03] = 0.6
    tt = np.cumsum(dt, axis=1) + 100.0 * np.arange(B)[:, None]
    tt[0, 20] = tt[0, 19]
    tt[1, 30] = tt[1, 29] - 1.0
    tt[2, 10] = np.nan
    lum = (50.0 + 20.0 * np.sin(np.arange(T) / 15.0)[None] + rng.normal(0, 1.0, (B, T))).astype(np.float32)
    lum[rng.rand(B, T) < 0.05] = np.nan
    marks = np.zeros((B, T), np.uint8)
    marks[:, 5:15], marks[:, 70:74], marks[0, 72] = 1, 1, 0
    return dict(left=left, right=right, frame_time=tt, eye_valid=ev, luminance=lum, baseline_mark=marks, lengths=np.array([T, T - 13, 45], np.int32)[:B])


FRAME_INPUTS = ('eye_valid', 'frame_time', 'luminance', 'baseline_mark')


def run_ref(spec, sc, buffers, cut=None, flush=True, reset=None, use=FRAME_INPUTS):
    B = sc['left'].shape[0]
    c = (lambda a: a) if cut is None else (lambda a: a[:, cut[0]:cut[1]])
    lengths = sc['lengths'] if cut is None else np.clip(sc['lengths'] - cut[0], 0, cut[1] - cut[0]).astype(np.int32)
    return ref.run(spec, c(sc['left']), c(sc['right']), *buffers, lengths=lengths, flush=np.ones(B, np.int32) if flush else None, reset=reset,
                   **{k: c(sc[k]) for k in use if sc.get(k) is not None})


def test_the_contract_equals_the_slow_formulation_exactly_on_dyadic_data():
    sc = exact_scene()
    spec = exact_spec()
    buffers = ref.fresh(2, 32)
    buffers[2][1] = (1.0, 0.25, 16.0, 0.0)               # stream 1 has a light response
    want = run_ref(spec, sc, buffers)
    got, table, episodes, dropped = slow_run(spec, sc, buffers[2], 32)
    for k in ref.KEYS:
        assert np.array_equal(want[k].astype(np.float64), got[k].astype(np.float64), equal_nan=k in FLOATS), k
        if k in FLOATS:                                  # ... and the float32 outputs lost nothing: the scene is exact in float32 too
            assert np.array_equal(want[k].astype(np.float64), got[k], equal_nan=True)
    assert buffers[1].tobytes() == table.tobytes()
    for b in range(2):
        assert buffers[4][b] == len(episodes[b]) and buffers[3][b, :buffers[4][b]].tobytes() == episodes[b].tobytes() and not dropped[b]
    # what the scene is meant to hold
    assert want['eye_reason'][0, 30, 0] == ref.RANGE and want['eye_reason'][1, 32, 1] == ref.SPEED and (want['eye_reason'][0, 3:5, 1] == ref.WITHHELD).all()
    assert want['valid'][0].sum() == 48 - 13 and want['valid'][1].sum() == 40 - 11 and (want['valid'][1, 40:] == 0).all()
    assert buffers[4].min() >= 3 and set(buffers[3][0, :buffers[4][0], 0]) == {1.0, -1.0}
    assert buffers[1][0, 16] == 35 and buffers[1][1, 16] == 29 and buffers[1][:, 1].tolist() == [0.0, 0.0] and buffers[1][0, 2:5].tolist() == [32, 2, 1]


def close(a, b, scale):
    """|a - b| <= 1e-12 * (|b| + scale) elementwise, NaNs at the same places.  1e-12: a few hundred ulps of the dozen float64 operations
    behind a value, with `scale` the size of the operands where the value is a difference of them."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and bool(np.all(np.abs(a - b)[~np.isnan(a)] <= 1e-12 * (np.abs(b)[~np.isnan(a)] + scale)))


@pytest.mark.parametrize('seed, baseline', [(1, 'marks'), (2, 'follower'), (3, 'none')])
def test_the_contract_equals_the_slow_formulation(seed, baseline):
    sc = random_scene(seed)
    tau = 2.0 if baseline == 'follower' else None
    spec = ref.Spec(max_speed_mm_s=8.0, max_gap_s=0.25, offset_rate=0.1, cutoff_hz=4.0, light_tau_s=0.4, baseline_tau_s=tau, dilate_mm_s=0.3,
                    constrict_mm_s=0.3, min_amplitude_mm=0.02)
    use = FRAME_INPUTS if baseline == 'marks' else FRAME_INPUTS[:3]
    buffers = ref.fresh(3, 4)
    buffers[2][0] = (1.0, -0.01, 50.0, 0.0)
    want = run_ref(spec, sc, buffers, use=use)
    got, table, episodes, dropped = slow_run(spec, sc, buffers[2], 4, marks=sc['baseline_mark'] if baseline == 'marks' else None, tau=tau)
    for k in ref.KEYS[5:]:
        assert np.array_equal(want[k], got[k]), k
    # the float32 outputs: the contract's double rounded once, so half a float32 ulp (2^-24 relative) on top of the doubles' bound
    mm, v_scale = 12.0, 12.0 / 0.028                     # sizes up to max_mm + the offset; a velocity is a difference of two over >= 28 ms
    for k, scale in (('mm', mm), ('raw_mm', mm), ('velocity', v_scale), ('change_mm', mm), ('change_pct', 100.0 * mm / 1.5)):
        a, b = want[k].astype(np.float64), got[k]
        assert np.array_equal(np.isnan(a), np.isnan(b)), k
        ok = ~np.isnan(a)
        assert np.all(np.abs(a - b)[ok] <= 2.0 ** -24 * np.abs(b)[ok] + 1e-12 * (np.abs(b)[ok] + scale)), k
    n = 120.0
    scales = [n] * 2 + [0.0] * 9 + [0.0, n * mm, n * mm * mm, 0.0, 0.0, 0.0, 0.0, 0.0, n * 100.0, n * mm, n * 1e4, n * 100.0 * mm, n * mm * mm]
    for i, scale in enumerate(scales):
        assert close(buffers[1][:, i], table[:, i], scale), i
    assert (buffers[1][:, 1] > 0).all() and (buffers[1][:, 0] > buffers[1][:, 1]).all() and buffers[1][:, 5:11].sum() >= 8
    for b in range(3):
        assert buffers[4][b] == len(episodes[b]) and buffers[5][b] == dropped[b]
        assert close(buffers[3][b, :buffers[4][b]], episodes[b], v_scale)
        assert (buffers[3][b, :buffers[4][b], [0, 6]] == episodes[b][:, [0, 6]].T).all()
    assert buffers[5][:2].min() > 0 and (buffers[4][:2] == 4).all()         # the four-row stores of the two long streams overflowed
    assert want['valid'].sum() > 150 and (want['eye_reason'] == ref.SPEED).sum() >= 3 and (want['eye_reason'] == ref.RANGE).sum() >= 3
    if baseline != 'none':
        assert np.isfinite(want['change_pct']).sum() > 100
    else:
        assert np.isnan(want['change_mm']).all() and np.isnan(want['change_pct']).all()


# ---------------------------------------------------------------------------------------------------------------- properties
def simple(left, right, spec, eye_valid=None, capacity=8, light=None, **kw):
    """One stream at 32 Hz from fresh state, flushed -> (outputs, buffers)."""
    left, right = np.float32(left)[None], np.float32(right)[None]
    buffers = ref.fresh(1, capacity)
    if light is not None:
        buffers[2][0] = light
    out = ref.run(spec, left, right, *buffers, eye_valid=None if eye_valid is None else np.uint8(eye_valid)[None],
                  frame_time=np.arange(left.shape[1])[None] * D, flush=np.ones(1, np.int32), **{k: np.asarray(v)[None] for k, v in kw.items()})
    return {k: v[0] for k, v in out.items()}, buffers


def test_constant_equal_eyes_give_the_constant():
    out, buffers = simple([3.5] * 20, [3.5] * 20, exact_spec())
    assert (out['mm'] == 3.5).all() and (out['raw_mm'] == 3.5).all() and np.isnan(out['velocity'][0]) and (out['velocity'][1:] == 0).all()
    assert (out['event'] == 0).all() and buffers[4][0] == 0 and (out['valid'] == 1).all() and (out['eye_used'] == 1).all()
    assert buffers[1][0, :5].tolist() == [19 * D, 0.0, 20.0, 0.0, 0.0] and buffers[1][0, 11:16].tolist() == [3.5, 0.0, 0.0, 3.5, 3.5]


def test_a_constant_offset_keeps_the_trace_still_when_an_eye_drops_out():
    n = 24
    ev = np.ones((n, 2), np.uint8)
    ev[8:14, 0], ev[16:20, 1] = 0, 0
    left, right = np.full(n, 4.25, np.float32), np.full(n, 3.75, np.float32)
    left[8:14] = np.nan
    out, _ = simple(left, right, exact_spec(), ev)
    assert (out['raw_mm'] == 4.0).all() and (out['mm'] == 4.0).all() and (out['eye_used'][8:14] == (0, 1)).all() and (out['eye_used'][16:20] == (1, 0)).all()
    # without the offset (the left eye alone from the first frame on) the trace would sit at the eye's own size
    ev[:, 1] = 0
    out, _ = simple(left, right, exact_spec(), ev)
    assert (out['raw_mm'][:8] == 4.25).all() and out['valid'][8:14].sum() == 0 and np.isnan(out['mm'][8:14]).all()


def test_a_spike_is_rejected_for_speed_until_max_gap_s_has_passed():
    n = 16
    left, right = np.full(n, 4.0, np.float32), np.full(n, 4.0, np.float32)
    left[5:] = 7.0                                       # a step of 3 mm in one frame (96 mm/s) that stays
    spec = exact_spec()
    out, buffers = simple(left, right, spec)
    # frames 5, 6, 7: 1, 2 and 3 frame periods after the last accepted value, all within max_gap_s = 3/32 s and too fast (3 mm in at most 3/32 s
    # is 32 mm/s or more -- 32 mm/s exactly at frame 7, which the <= of the bound admits)
    assert out['eye_reason'][:, 0].tolist() == [0] * 5 + [8, 8] + [0] * 9 and (out['eye_reason'][:, 1] == 0).all()
    assert (out['raw_mm'][:7] == 4.0).all() and (out['mm'][:7] == 4.0).all() and (out['eye_used'][5:7] == (0, 1)).all() and buffers[1][0, 7] == 2
    out, buffers = simple(left, right, exact_spec(max_speed_mm_s=31.0))
    # a tighter bound: rejected until the last accepted value is more than max_gap_s old (frame 9: 4/32 s), then re-admitted untested
    assert out['eye_reason'][:, 0].tolist() == [0] * 5 + [8, 8, 8] + [0] * 8 and out['raw_mm'][8] == 5.5 and buffers[1][0, 7] == 3


def test_a_withheld_eye_s_value_changes_no_bit():
    sc = exact_scene()
    spec = exact_spec(baseline_tau_s=D)
    a_buffers, b_buffers = ref.fresh(2, 32), ref.fresh(2, 32)
    a = run_ref(spec, sc, a_buffers)
    other = dict(sc, left=sc['left'].copy(), right=sc['right'].copy())
    for side, e in (('left', 0), ('right', 1)):
        hidden = sc['eye_valid'][..., e] == 0
        other[side][hidden] = np.resize(np.float32([np.nan, 1e30, -5.0, 0.0, np.inf, 4.0]), hidden.sum())
    assert other['left'].tobytes() != sc['left'].tobytes()
    b = run_ref(spec, other, b_buffers)
    for k in ref.KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k
    for x, y in zip(a_buffers, b_buffers):
        assert x.tobytes() == y.tobytes()


def halved(x):
    """What the exact scenes' low pass (a = 1/2) makes of connected samples: y[0] = x[0], y[k] = (x[k] + y[k - 1]) / 2, exact on dyadic data."""
    y = [np.float64(x[0])]
    for v in x[1:]:
        y.append((np.float64(v) + y[-1]) / 2)
    return np.array(y)


def test_a_planted_light_response_is_fitted_exactly_and_flattens_the_trace():
    """size = a0 - g * luminance on integer luminance: both low passes halve (a = al = 1/2) and start together, so the filtered size is
    a0 - g * Lf to the bit, and sixteen frames keep every product inside 53 bits."""
    n, g, a0 = 16, 0.25, 7.0
    spec = exact_spec(max_speed_mm_s=1e6, dilate_mm_s=1e6, constrict_mm_s=1e6)
    lum = np.float32(np.random.RandomState(0).randint(4, 13, n))
    size = np.float32(a0 - g * lum)
    out, buffers = simple(size, size, spec, luminance=lum)
    lf = halved(lum)
    assert (out['mm'] == np.float32(a0 - g * lf)).all() and (np.float64(np.float32(a0 - g * lf)) == a0 - g * lf).all()
    tab = buffers[1][0]
    # fit_pupil_light_response's formula
    gain, ref_l = tab[ref.SXY] / tab[ref.SXX], tab[ref.X0] + tab[ref.SX] / tab[ref.N]
    assert tab[ref.N] == n and gain == -g and ref_l == lf.sum() / n
    out2, _ = simple(size, size, spec, luminance=lum, light=(1.0, gain, 8.0, 0.0))
    assert (out2['mm'] == np.float32(a0 - g * 8.0)).all() and (out2['raw_mm'] == size).all()


def test_marked_baselines_start_anew_with_every_run_of_marks():
    n = 24
    size = np.float32(4.0 + np.arange(n) / 8.0)
    marks = np.zeros(n, np.uint8)
    marks[2:6], marks[12:14] = 1, 1
    spec = exact_spec(dilate_mm_s=1e6, max_speed_mm_s=1e6)
    ev = np.ones((n, 2), np.uint8)
    ev[4] = 0                                            # a marked frame that is no sample: the run goes on (three samples of four marks)
    out, buffers = simple(size, size, spec, ev, baseline_mark=marks)
    idx = np.array([f for f in range(n) if f != 4])
    df = np.full(n, np.nan)
    df[idx[0]] = size[0]
    for i, j in zip(idx[:-1], idx[1:]):                  # the low pass over the samples, the step over frame 4 twice as long
        dt = (j - i) * D
        df[j] = df[i] + dt / (dt + D) * (size[j] - df[i])
    assert np.allclose(out['mm'][idx], df[idx], rtol=0, atol=1e-6)
    assert np.isnan(out['change_mm'][:2]).all() and np.isnan(out['change_mm'][4]) and out['valid'][4] == 0
    mean1, mean2 = df[[2, 3, 5]].sum() / 3, df[[12, 13]].sum() / 2
    assert out['change_mm'][2] == 0 and out['change_mm'][3] == np.float32(df[3] - (df[2] + df[3]) / 2) and out['change_mm'][12] == 0
    tol = dict(rtol=0, atol=1e-5)                        # float32 outputs of sizes up to 8 mm: an ulp is 5e-7
    assert np.allclose(out['change_mm'][6:12], df[6:12] - mean1, **tol) and np.allclose(out['change_mm'][14:], df[14:] - mean2, **tol)
    assert np.allclose(out['change_pct'][20], 100.0 * (df[20] - mean2) / mean2, rtol=0, atol=1e-4)
    assert abs(buffers[0][0, ref.BASE] - mean2) < 1e-12 and buffers[0][0, ref.B_N] == 2 and abs(df[13] - mean2) > 0.01 and abs(mean1 - mean2) > 0.5


def test_the_follower_baseline_trails_the_trace():
    size = np.float32([4.0] * 4 + [5.0] * 8)
    spec = exact_spec(baseline_tau_s=D, dilate_mm_s=1e6, max_speed_mm_s=1e6)      # base += (dc - base) / 2
    out, buffers = simple(size, size, spec)
    df = halved(size)
    base, change = df[0], []
    for v in df:
        base = base + (v - base) / 2
        change.append(v - base)
    assert (out['change_mm'] == np.float32(change)).all() and (out['change_mm'][:4] == 0).all() and out['change_mm'][4:7].tolist() == [0.25, 0.25, 0.1875]
    assert out['change_pct'][4] == np.float32(100.0 * 0.25 / 4.25) and buffers[0][0, ref.BASE] == base and 4.9 < base < 5.0
    none, _ = simple(size, size, exact_spec())
    assert np.isnan(none['change_mm']).all() and np.isnan(none['change_pct']).all()


def test_a_ramp_up_and_down_gives_two_episodes_and_a_full_store_drops_the_second():
    up, hold, down = 4.0 + np.arange(9) / 8.0, [5.0] * 6, 5.0 - np.arange(1, 9) / 4.0
    size = np.float32(np.concatenate([[4.0] * 3, up, hold, down, [3.0] * 6]))
    spec = exact_spec(max_speed_mm_s=1e6)                # a sample dilates above 1 mm/s and constricts below -1 mm/s
    out, buffers = simple(size, size, spec)
    df = halved(size)
    vel = np.concatenate([[np.nan], np.diff(df) / D])
    rising, falling = np.flatnonzero(vel > 1.0), np.flatnonzero(vel < -1.0)
    assert (np.diff(rising) == 1).all() and (np.diff(falling) == 1).all() and rising[0] == 4 and rising[-1] < falling[0] - 3
    assert out['event'].tolist() == np.where(vel > 1.0, 1, np.where(vel < -1.0, 2, 0)).tolist()
    assert buffers[4][0] == 2 and buffers[5][0] == 0 and buffers[0][0, ref.EP_COUNT] == 2
    for row, run, phase in ((buffers[3][0, 0], rising, 1.0), (buffers[3][0, 1], falling, -1.0)):    # each begins at the sample before its first
        assert row.tolist() == [phase, (run[0] - 1) * D, run[-1] * D, df[run[0] - 1], df[run[-1]], np.abs(vel[run]).max(), len(run), 0.0]
    assert 0.9 < buffers[3][0, 0, 4] - buffers[3][0, 0, 3] < 1.0 and -2.0 < buffers[3][0, 1, 4] - buffers[3][0, 1, 3] < -1.9
    out1, one = simple(size, size, spec, capacity=1)
    assert one[4][0] == 1 and one[5][0] == 1 and one[3][0, 0].tolist() == buffers[3][0, 0].tolist() and one[0][0, ref.EP_COUNT] == 2
    assert out1['event'].tobytes() == out['event'].tobytes() and one[1].tobytes() == buffers[1].tobytes()
    # an amplitude below min_amplitude_mm is no episode
    _, small = simple(size, size, exact_spec(max_speed_mm_s=1e6, min_amplitude_mm=1.5))
    assert small[4][0] == 1 and small[3][0, 0, 0] == -1.0 and small[0][0, ref.EP_COUNT] == 1


# ---------------------------------------------------------------------------------------------------------------- chunk splits
@pytest.mark.parametrize('sizes', [(48,), (1,) * 48, (7, 5, 20, 16), (3, 13, 17, 15), (31, 1, 16)])
def test_any_split_into_chunks_equals_one_pass(sizes):
    """The cuts fall inside episodes, inside a run of baseline marks (frames 4 .. 8), inside the holes and inside the rejected stretch."""
    sc = exact_scene()
    sc['baseline_mark'] = np.zeros((2, 48), np.uint8)
    sc['baseline_mark'][:, 4:9], sc['baseline_mark'][:, 30:34] = 1, 1
    spec = exact_spec(max_speed_mm_s=31.0)
    whole = ref.fresh(2, 32)
    want = run_ref(spec, sc, whole)
    assert whole[4].min() >= 3 and np.isfinite(want['change_mm']).sum() > 40
    for variant in (dict(use=FRAME_INPUTS), dict(use=('eye_valid', 'luminance'))):      # ... and on the counted clock
        spec_v = spec if 'frame_time' in variant['use'] else exact_spec(max_speed_mm_s=31.0, fps=32.0, baseline_tau_s=0.5)
        whole = ref.fresh(2, 32)
        want = run_ref(spec_v, sc, whole, **variant)
        parts, outs, t0 = ref.fresh(2, 32), [], 0
        for n in sizes:
            outs.append(run_ref(spec_v, sc, parts, cut=(t0, t0 + n), flush=t0 + n == 48, **variant))
            t0 += n
        for k in ref.KEYS:
            assert np.concatenate([o[k] for o in outs], axis=1).tobytes() == want[k].tobytes(), k
        for a, b in zip(parts, whole):
            assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------------------------- the spec
def test_the_spec_compares_by_value_and_refuses_nonsense():
    a, b = PupilSpec(fps=30, min_mm=1, max_mm=9), PupilSpec('pupil', 30.0, 1.0, 9.0)
    assert a == b and hash(a) == hash(b) and a.key() == b.key() and len({a, b}) == 1 and 'PupilSpec(' in repr(a)
    fields = ('fps', 'min_mm', 'max_mm', 'max_speed_mm_s', 'max_gap_s', 'offset_rate', 'cutoff_hz', 'light_tau_s', 'baseline_tau_s', 'dilate_mm_s',
              'constrict_mm_s', 'min_amplitude_mm')
    good = dict(fps=30.0, min_mm=1.0, max_mm=9.0, max_speed_mm_s=12.0, max_gap_s=0.2, offset_rate=0.25, cutoff_hz=5.0, light_tau_s=0.3,
                baseline_tau_s=4.0, dilate_mm_s=0.2, constrict_mm_s=0.4, min_amplitude_mm=0.05)
    base = PupilSpec(**good)
    assert [getattr(base, f) for f in fields] == [good[f] for f in fields]
    for f in fields:
        other = PupilSpec(**dict(good, **{f: good[f] * 0.5}))
        assert other != base and other.key() != base.key(), f
    assert PupilSpec('other', **good) != base and PupilSpec(**dict(good, fps=None, baseline_tau_s=None)).baseline_tau_s is None
    assert PupilSpec(**dict(good, offset_rate=1)).offset_rate == 1.0 and PupilSpec(**dict(good, min_amplitude_mm=0)).min_amplitude_mm == 0.0
    bad = [dict(name=''), dict(name=3), dict(min_mm=9.0), dict(min_mm=10.0), dict(offset_rate=0.0), dict(offset_rate=1.5), dict(min_amplitude_mm=-1.0)]
    for f in fields:
        bad += [{f: v} for v in (float('nan'), float('inf'), -1.0, '1', True)]
        if f not in ('min_amplitude_mm',):
            bad.append({f: 0.0})
    for kw in bad:
        with pytest.raises(ValueError, match='PupilSpec'):
            PupilSpec(**dict(good, **kw))


# ---------------------------------------------------------------------------------------------------------------- EVEStream
class PupilFakes(EventOverlayFakes):
    """The events' and the overlay's stand-ins plus pupil_track, evaluated by tests/pupil_ref.py."""

    def pupil_track(self, size, spec, state, table, light, store, count, dropped, eye_valid=None, frame_time=None, lengths=None, reset=None,
                    flush=None, luminance=None, baseline_mark=None):
        self.calls.append('pupil_track')
        n = lambda t: None if t is None else t.detach().numpy()
        carried = [n(t) for t in (state, table, light, store, count, dropped)]
        if size is None:
            B = state.shape[0]
            ref.run(spec, np.zeros((B, 0), np.float32), np.zeros((B, 0), np.float32), *carried, reset=n(reset), flush=n(flush))
            return {}
        assert size.dtype == torch.float32 and size.shape[0] == 2
        out = ref.run(spec, n(size[0]), n(size[1]), *carried, eye_valid=n(eye_valid), frame_time=n(frame_time), lengths=n(lengths), reset=n(reset),
                      flush=n(flush), luminance=n(luminance), baseline_mark=n(baseline_mark))
        return {k: torch.from_numpy(v) for k, v in out.items()}


@pytest.fixture()
def fake():
    k = PupilFakes()
    kernels.set_default_kernels(k)
    yield k
    kernels.set_default_kernels(None)
    eve_amd.reset_standalone_config()


B, T = 2, 3
NEW = ['pupil_' + k for k in ref.KEYS]


@pytest.fixture()
def scene(fake):
    """The model, two chunks, and a spec laid around the stand-in EyeNet's own pupil sizes (a probe stream's): a range that holds them
    all, and a speed bound they keep."""
    model, _ = make_model(dict(refine_net_rnn_type='CGRU'))
    with torch.no_grad():
        model.eye_net.fc_to_pupil[2].bias.add_(3.0)      # an untrained head ends in a ReLU: lift it off zero
    batch = clip(B, 2 * T, size=32)
    c0, c1 = chunk_of(batch, 0, T), chunk_of(batch, T, 2 * T)
    probe = eve_amd.EVEStream(model, B, use_graph=False)
    p = torch.cat([torch.stack([o['left_pupil_size'], o['right_pupil_size']], dim=-1).clone() for o in (probe.step(c0), probe.step(c1))], dim=1).numpy()
    assert np.isfinite(p).all() and p.min() > 0.5
    del fake.calls[:]
    spec = PupilSpec(fps=32, min_mm=float(p.min()) / 2, max_mm=float(p.max()) * 2, max_speed_mm_s=1e4, max_gap_s=0.25, offset_rate=0.5, cutoff_hz=4.0,
                     dilate_mm_s=1e-4, constrict_mm_s=1e-4, min_amplitude_mm=0.0)
    return model, c0, c1, spec


def run(stream, chunk, **kw):
    return {k: v.clone() for k, v in stream.step(chunk, **kw).items()}


def reference_on(out, spec, buffers, **kw):
    n = lambda t: None if t is None else (t.numpy() if torch.is_tensor(t) else t)
    return ref.run(spec, out['left_pupil_size'].numpy(), out['right_pupil_size'].numpy(), *buffers, **{k: n(v) for k, v in kw.items()})


def carried(stream, name='pupil'):
    st = stream.get_pupil_state()[name]
    return [st[k] for k in ('state', 'table', 'light', 'episodes', 'count', 'dropped')]


def test_a_step_with_pupil_adds_nine_keys_and_one_launch(fake, scene):
    model, c0, c1, spec = scene
    plain = run(eve_amd.EVEStream(model, B, use_graph=False), c0)
    assert 'pupil_track' not in fake.calls and not [k for k in plain if k.startswith('pupil_')]
    calls_plain = list(fake.calls)
    del fake.calls[:]
    s = eve_amd.EVEStream(model, B, use_graph=False, episode_capacity=8)
    out = run(s, c0, pupil=spec)
    assert fake.calls == calls_plain + ['pupil_track']                    # the plain step's launches, then one more
    assert sorted(out) == sorted(list(plain) + NEW)
    for k in plain:
        assert torch.equal(out[k], plain[k]), k
    for k in ref.KEYS:
        assert tuple(out['pupil_' + k].shape) == ((B, T, 2) if k.startswith('eye_') else (B, T)), k
        assert out['pupil_' + k].dtype == (torch.float32 if k in FLOATS else torch.uint8), k
    buffers = ref.fresh(B, 8)
    want = reference_on(out, spec, buffers)
    out1 = run(s, c1, pupil=spec)
    want1 = reference_on(out1, spec, buffers)
    for o, w in ((out, want), (out1, want1)):
        for k in ref.KEYS:
            assert o['pupil_' + k].numpy().tobytes() == w[k].tobytes(), k
    for got, want_ in zip(carried(s), buffers):
        assert got.numpy().tobytes() == want_.tobytes()
    assert out['pupil_valid'].all() and s.pupil_table()[:, 2].tolist() == [6.0, 6.0] and buffers[0][:, ref.TICKS].tolist() == [6.0, 6.0]
    assert torch.isnan(out['pupil_change_mm']).all()                      # no marks, no follower
    # explicit times win over fps; the two chunk keys reach the launch; a name of the caller's
    s2 = eve_amd.EVEStream(model, B, use_graph=False)
    ft = torch.tensor([[0.0, 0.011, 0.5], [5.0, 5.01, 5.02]], dtype=torch.float64)
    lum = torch.tensor([[3.0, 4.0, 5.0], [9.0, float('nan'), 7.0]])
    marks = torch.tensor([[1, 1, 0], [0, 1, 1]], dtype=torch.bool)
    spec2 = PupilSpec('size', None, *spec.key()[2:])
    assert spec2.fps is None and spec2.key()[2:] == spec.key()[2:]
    out2 = run(s2, dict(c0, frame_time=ft, pupil_luminance=lum, pupil_baseline=marks), pupil=spec2)
    b2 = ref.fresh(B, 256)
    want2 = reference_on(out2, spec2, b2, frame_time=ft, luminance=lum, baseline_mark=marks.numpy().astype(np.uint8))
    for k in ref.KEYS:
        assert out2['size_' + k].numpy().tobytes() == want2[k].tobytes(), k
    assert s2.pupil_table('size').numpy().tobytes() == b2[1].tobytes() and b2[1][:, ref.N].tolist() == [3.0, 3.0] and 'pupil_mm' not in out2
    assert torch.isnan(out2['size_change_mm']).tolist() == [[False] * 3, [True, False, False]] and np.isnan(want2['velocity'][0, 2])      # 0.489 s: past max_gap_s


def test_pupil_follows_lengths_and_masks(fake, scene):
    model, c0, _, spec = scene
    s = eve_amd.EVEStream(model, B, use_graph=False)
    out = run(s, c0, pupil=spec, lengths=[2, 0])
    buffers = ref.fresh(B, 256)
    want = reference_on(out, spec, buffers, lengths=np.array([2, 0]))
    for k in ref.KEYS:
        assert out['pupil_' + k][0, :2].numpy().tobytes() == want[k][0, :2].tobytes(), k
    assert not out['pupil_valid'][1].any() and not out['pupil_valid'][0, 2] and carried(s)[0][:, 0].tolist() == [2.0, 0.0]
    mask = torch.ones(B, T, 2, dtype=torch.bool)
    mask[0, 1, 0], mask[1, 2] = False, False
    s = eve_amd.EVEStream(model, B, use_graph=False)
    out = run(s, c0, pupil=spec, eye_mask=mask)
    buffers = ref.fresh(B, 256)
    want = reference_on(out, spec, buffers, eye_valid=out['eye_valid'].numpy().astype(np.uint8))
    for k in ref.KEYS:
        assert out['pupil_' + k].numpy().tobytes() == want[k].tobytes(), k
    assert out['pupil_eye_reason'][0, 1].tolist() == [1, 0] and out['pupil_eye_used'][0, 1].tolist() == [0, 1] and not out['pupil_valid'][1, 2]
    assert out['pupil_eye_reason'][1, 2].tolist() == [1, 1] and s.pupil_table()[:, 2:5].tolist() == [[2, 0, 1], [2, 0, 0]]


def test_refusals_come_before_any_launch(fake, scene):
    model, c0, _, spec = scene
    s = eve_amd.EVEStream(model, B, use_graph=False)
    with pytest.raises(ValueError, match='PupilSpec'):
        s.step(c0, pupil=dict(fps=30))
    with pytest.raises(ValueError, match='PupilSpec'):
        s.step(c0, pupil=data.AoiSpec(num_aois=2, fps=30))
    with pytest.raises(ValueError, match='name'):
        s.step(dict(c0, pupil_mm=torch.zeros(B, T)), pupil=spec)
    with pytest.raises(ValueError, match='name'):
        s.step(c0, pupil=PupilSpec('eye', fps=30), eye_mask=torch.ones(B, T, 2, dtype=torch.bool))      # eye_valid is the masked step's key
    lum, marks = torch.zeros(B, T), torch.zeros(B, T, dtype=torch.bool)
    for bad in (lum.double(), lum[:, :2].contiguous(), lum[:1].contiguous(), lum.numpy(), lum[..., None], marks):
        with pytest.raises(ValueError, match='pupil_luminance'):
            s.step(dict(c0, pupil_luminance=bad), pupil=spec)
    for bad in (marks.float(), marks[:, :2].contiguous(), marks[:1].contiguous(), marks.numpy(), marks[..., None], marks.to(torch.int32)):
        with pytest.raises(ValueError, match='pupil_baseline'):
            s.step(dict(c0, pupil_baseline=bad), pupil=spec)
    nofps = PupilSpec(min_mm=spec.min_mm, max_mm=spec.max_mm)
    with pytest.raises(ValueError, match='frame_time'):
        s.step(c0, pupil=nofps)
    with pytest.raises(ValueError, match='frame_time'):
        s.step(dict(c0, frame_time=torch.zeros(B, T)), pupil=spec)
    with pytest.raises(ValueError, match='episode_capacity'):
        eve_amd.EVEStream(model, B, use_graph=False, episode_capacity=0)
    for call in (s.pupil_table, s.pupil_episodes, s.pupil_episode_counts, s.get_pupil_light_response, s.fit_pupil_light_response,
                 lambda: s.set_pupil_light_response(1.0, 0.0), s.clear_pupil_light_response):
        with pytest.raises(ValueError, match='no pupillometry'):
            call()
    assert fake.calls == [] and s._pupil == {}
    # the tallies are tied to their spec
    s.step(c0, pupil=spec)
    other = PupilSpec(**dict(zip(('name', 'fps', 'min_mm', 'max_mm'), spec.key()[:4]), cutoff_hz=2.0))
    del fake.calls[:]
    with pytest.raises(ValueError, match='another spec'):
        s.step(c0, pupil=other)
    assert fake.calls == []
    s.clear_pupil('pupil')
    s.step(c0, pupil=other)
    assert s.get_pupil_state()['pupil']['spec'].cutoff_hz == 2.0
    with pytest.raises(ValueError, match='min_samples'):
        s.fit_pupil_light_response(min_samples=1)
    with pytest.raises(ValueError, match='gain'):
        s.set_pupil_light_response(float('nan'), 0.0)


def test_the_graph_key_holds_the_spec_and_the_two_chunk_keys(fake, scene):
    model, c0, _, spec = scene
    s = eve_amd.EVEStream(model, B, use_graph=False)
    plan = lambda spec_, ch=c0: s._check_pupil(ch, spec_, None, None, None, None, B, T)
    bare = s._graph_key(c0, False)
    a = s._graph_key(c0, False, pupil=plan(spec))
    same = PupilSpec(*spec.key())
    assert a != bare and a == s._graph_key(dict(c0), False, pupil=plan(same))
    assert a != s._graph_key(c0, False, pupil=plan(PupilSpec(*(spec.key()[:7] + (6.0,) + spec.key()[8:]))))
    lit = dict(c0, pupil_luminance=torch.zeros(B, T))
    marked = dict(c0, pupil_baseline=torch.zeros(B, T, dtype=torch.bool))
    keys = {a, s._graph_key(lit, False, pupil=plan(spec, lit)), s._graph_key(marked, False, pupil=plan(spec, marked)),
            s._graph_key(dict(lit, **marked), False, pupil=plan(spec, dict(lit, **marked)))}
    assert len(keys) == 4
    captured = []
    s._capture = lambda chunk, *a_, **k_: captured.append((a_, k_)) or {'n': len(captured)}
    first = s._graph_for(c0, False, pupil=plan(spec))
    assert s._graph_for(c0, False, pupil=plan(same)) is first and len(captured) == 1 and 'pupil' in captured[0][1]
    assert s._graph_for(c0, False) is not first and len(captured) == 2 and len(captured[1][0]) == 4 and captured[1][1] == {}
    # the buffers exist before a capture could run, and _carried() returns them: a capture's warm-up steps are put back
    s._pupil_entry(spec)
    ids = {id(t) for t in s._carried()}
    assert all(id(t) in ids for t in s._pupil['pupil']['buffers'])


def test_reset_closes_the_episode_and_keeps_the_table(fake, scene):
    model, c0, c1, spec = scene
    s = eve_amd.EVEStream(model, B, use_graph=False, episode_capacity=4)
    out = run(s, c0, pupil=spec)
    # the rig's thresholds (1e-4 mm/s) make every connected sample dilate or constrict: something is open unless the size stood still
    state = carried(s)[0]
    assert state[0, ref.EP_OPEN] == 1 or (out['pupil_event'][0, 1:] == 0).all()
    table, before = s.pupil_table(), s.pupil_episode_counts()[0].clone()
    open0 = float(state[0, ref.EP_OPEN])
    s.set_pupil_light_response(0.5, 2.0, streams=[1])
    s.reset([0])
    run(s, c1, pupil=spec)
    after = carried(s)[0]
    assert after[:, ref.TICKS].tolist() == [T, 2 * T] and after[0, ref.EP_COUNT] >= open0
    count, _ = s.pupil_episode_counts()
    assert count[0] >= before[0] + open0
    now = s.pupil_table()
    assert now[0, 2] == table[0, 2] + T and now[0, 11] == table[0, 11] and now[0, 0] == table[0, 0] + 2 / 32.0      # the table ran on; the reset cut the time
    assert s.get_pupil_light_response().tolist() == [[0, 0, 0, 0], [1, 0.5, 2.0, 0]]
    # a reset before a step WITHOUT pupil= still ends the episode: one launch with no frames, then the plain step
    s.reset([1])
    del fake.calls[:]
    plain = run(s, c0)
    assert fake.calls.count('pupil_track') == 1 and fake.calls[0] == 'pupil_track' and not [k for k in plain if k.startswith('pupil_')]
    state = carried(s)[0]
    assert not state[1, :ref.EP_COUNT].any() and state[0, ref.HAS_PREV] == 1 and torch.equal(s.pupil_table(), now)
    s.flush_pupil_episodes([0])
    assert carried(s)[0][0, ref.EP_OPEN] == 0
    assert [len(e) for e in s.pupil_episodes()] == s.pupil_episode_counts()[0].tolist() and s.pupil_episodes([1])[0].shape[1] == 8
    # the state round-trips, and get_state() does not hold it
    saved = s.get_pupil_state()
    s.clear_pupil(streams=[0])
    assert not s.pupil_table()[0].any() and s.pupil_table()[1].any()
    s.clear_pupil()
    s.clear_pupil_light_response()
    assert not s.pupil_table().any() and not s.get_pupil_light_response().any()
    s.set_pupil_state(saved)
    again = s.get_pupil_state()['pupil']
    for k, v in saved['pupil'].items():
        assert (again[k] == v) if k == 'spec' else torch.equal(again[k], v), k
    assert not any('pupil' in k for k in s.get_state())
    with pytest.raises(ValueError, match='spec'):
        s.set_pupil_state({'pupil': {k: v for k, v in saved['pupil'].items() if k != 'spec'}})
    with pytest.raises(ValueError, match='table'):
        s.set_pupil_state({'pupil': dict(saved['pupil'], table=torch.zeros(B, 23))})
    fresh = eve_amd.EVEStream(model, B, use_graph=False, episode_capacity=4)
    fresh.set_pupil_state(saved)
    assert torch.equal(fresh.pupil_table(), s.pupil_table())


def test_the_light_response_is_fitted_from_the_table_on_the_device(fake, scene):
    model, c0, c1, spec = scene
    s = eve_amd.EVEStream(model, B, use_graph=False)
    lum0, lum1 = torch.tensor([[3.0, 5.0, 4.0], [7.0, 7.0, 7.0]]), torch.tensor([[9.0, 2.0, 6.0], [7.0, 7.0, 7.0]])
    run(s, dict(c0, pupil_luminance=lum0), pupil=spec)
    run(s, dict(c1, pupil_luminance=lum1), pupil=spec)
    tab = s.pupil_table().numpy()
    assert tab[:, ref.N].tolist() == [6.0, 6.0] and tab[0, ref.SXX] > 0 and tab[1, ref.SXX] == 0      # stream 1's luminance never moved
    s.fit_pupil_light_response(min_samples=7)
    assert not s.get_pupil_light_response().any()                          # too few pairs: nothing is set
    s.set_pupil_light_response(9.0, 9.0, streams=[1])
    s.fit_pupil_light_response(min_samples=6)
    light = s.get_pupil_light_response().numpy()
    assert light[0].tolist() == [1.0, tab[0, ref.SXY] / tab[0, ref.SXX], tab[0, ref.X0] + tab[0, ref.SX] / tab[0, ref.N], 0.0]
    assert light[1].tolist() == [1.0, 9.0, 9.0, 0.0]                        # Sxx == 0: stream 1 keeps what it had
    # the next step applies it: mm = the filtered size - gain * (Lf - ref), by the reference on the same buffers
    buffers = [t.numpy().copy() for t in carried(s)]
    out = run(s, dict(c0, pupil_luminance=lum0), pupil=spec)
    want = reference_on(out, spec, buffers, luminance=lum0)
    assert out['pupil_mm'].numpy().tobytes() == want['mm'].tobytes() and not torch.equal(out['pupil_mm'], out['pupil_raw_mm'])
