"""CPU: smooth pursuit as the third gaze class -- the numpy contract (tests/pursuit_ref.py) on the scan path of
test_gaze_events_host.py (no pursuit there), on ramps (one episode each), on one small path per rule and under chunk splits with
ragged lengths and resets; eve_amd.PursuitSpec; data.pursuit_summary; and the EVEStream plumbing (step(events=..., pursuits=...), the
refusals, the graph key, the launches, reset, the resynchronising launch, the accessors, the state round trip) over a stand-in whose
gaze_events_ex, gaze_saccades and gaze_pursuits are the references themselves.  The GPU suite (test_gpu_pursuits.py) checks the HIP
kernel."""
import math

import numpy as np
import pytest
import torch

import eve_amd
import gaze_events_ref as eref
import pursuit_ref as ref
import saccade_ref as sref
from eve_amd import kernels
from eve_amd.data import GAZE_EVENT_KEYS, PURSUIT_COLUMNS, PURSUIT_KEYS, PURSUIT_TABLE, SACCADE_KEYS, GazeEventSpec, PursuitSpec, SaccadeSpec, \
    pursuit_summary
from test_gaze_events_host import DEG_PX, EYE, JITTER_PX, POINTS, PPM, scan_path
from test_saccades_host import SaccadeFakes
from test_stream_host import chunk_of, clip, make_model

TALLIES = [ref.ACCEPTED, ref.ABORTED, ref.SMALL, ref.SHORT, ref.INTERRUPTED]


# ---------------------------------------------------------------------------------------------------------------- the contract
def geometry(T, B=1):
    return (np.tile(EYE.astype(np.float32), (B, T, 1)), np.tile(np.eye(4, dtype=np.float32), (B, T, 1, 1)), np.full((B, T, 2), PPM, dtype=np.float32))


def path(fps, pieces, angle_deg=0.0, seed=5, jitter=True):
    """A point that moves along a line from A: pieces are (seconds, degrees / second) in turn -> (pog [1, T, 2] float32 with
    scan_path's bounded 0.1 degree jitter, target [1, T, 2] float32 without it); frame i at i / fps."""
    rng = np.random.RandomState(seed)
    d = np.array([math.cos(math.radians(angle_deg)), math.sin(math.radians(angle_deg))])
    T = int(round(sum(p[0] for p in pieces) * fps)) + 1
    pog, target = np.zeros((1, T, 2), dtype=np.float32), np.zeros((1, T, 2), dtype=np.float32)
    for i in range(T):
        t, s, t0 = i / fps, 0.0, 0.0
        for seconds, deg_s in pieces:
            s += deg_s * min(max(t - t0, 0.0), seconds)
            t0 += seconds
        p = np.array(POINTS['A']) + s * DEG_PX * d
        target[0, i] = p
        pog[0, i] = p + rng.uniform(-1, 1, 2) * JITTER_PX / math.sqrt(2.0) if jitter else p
    return pog, target


def ramp(fps, deg_s, angle_deg=0.0):
    """0.5 s fixation, 1 s at constant velocity, 0.5 s fixation."""
    return path(fps, [(0.5, 0.0), (1.0, deg_s), (0.5, 0.0)], angle_deg)


def both(spec, pspec, pog, valid=None, target=None, capacity=8, log=None):
    """The events and the pursuit of one clip [1, T, 2], from fresh state -> (ex, out, (state, table, store, count, dropped))."""
    o, inv_cam, ppm = geometry(pog.shape[1])
    ex = sref.events_ex(spec, pog, o, inv_cam, ppm, *eref.fresh(1, 64), valid=valid)
    carried = ref.fresh(1, capacity)
    out = ref.run(pspec, ex['sample'], ex['sample_time'], ex['gaze_vector'], sref.point_of(spec, pog, ex), ex['gaze_event'], ex['gaze_velocity'],
                  ex['fixation_id'], *carried, target=target, log=log)
    return ex, out, carried


def only(table, column, n=1):
    """The table counts n episodes, all under `column`."""
    return all(table[0, c] == (n if c == column else 0) for c in TALLIES)


@pytest.mark.parametrize('velocity_from', ['filtered', 'raw'])
@pytest.mark.parametrize('fps', [30, 60, 120])
def test_the_scan_path_holds_no_pursuit(fps, velocity_from):
    """Fixations, saccades and a hole: not one candidate, an all-zero table, and the events' labels for classes."""
    pog, _, _, _, valid, _ = scan_path(fps)
    ex, out, (state, table, store, count, dropped) = both(GazeEventSpec(fps=fps, velocity_from=velocity_from), PursuitSpec(), pog, valid)
    assert not (out['gaze_class'] == 3).any() and not table.any() and not store.any() and count[0] == 0 and dropped[0] == 0
    assert (out['pursuit_id'] == -1).all() and not out['pursuit_ms'].any() and np.isnan(out['pursuit_gain']).all()
    labelled = ex['sample'][0] == 2
    assert np.array_equal(out['gaze_class'][0, labelled], ex['gaze_event'][0, labelled]) and not out['gaze_class'][0, ~labelled].any()
    w = out['gaze_velocity_windowed'][0]
    assert np.isfinite(w).any() and np.nanmax(w) < 1.5       # (the reference's own: 0.33 .. 0.37 filtered, 1.05 .. 1.21 raw; the threshold is 3)
    assert state[0, ref.OPEN] == 0 and state[0, ref.NEXT_ID] == 0


# the reference's own values at 30 / 60 / 120 fps: amplitude 7.902 / 7.922 / 7.917, direction -0.05 / -0.01 / 0.13, peak 8.51 / 8.34 / 8.40;
# amplitude 14.585 / 14.582 / 14.646, direction 89.91 / 90.01 / 90.00; amplitude 3.696 / 3.797 / 3.814
RAMPS = [(8.0, 0.0, (7.0, 8.5), True, (7.5, 9.5)), (15.0, 90.0, (13.5, 15.5), True, None), (4.0, 0.0, (3.0, 4.3), False, None)]


@pytest.mark.parametrize('deg_s,angle,amp,check_direction,peak', RAMPS)
@pytest.mark.parametrize('fps', [30, 60, 120])
def test_a_ramp_is_one_episode(fps, deg_s, angle, amp, check_direction, peak):
    pog, _ = ramp(fps, deg_s, angle)
    ex, out, (state, table, store, count, dropped) = both(GazeEventSpec(fps=fps), PursuitSpec(), pog)
    assert only(table, ref.ACCEPTED) and count[0] == 1 and dropped[0] == 0 and state[0, ref.OPEN] == 0 and not store[0, 1:].any()
    row = store[0, 0]
    assert amp[0] <= row[ref.R_AMP] <= amp[1]
    if check_direction:
        assert abs(row[ref.R_DIR] - angle) <= 2.0
    if peak is not None:
        assert peak[0] <= row[ref.R_PEAK] <= peak[1]
    inside = out['pursuit_id'][0] == int(row[ref.R_ID])
    t = ex['sample_time'][0]
    assert inside.sum() == row[ref.R_N] and (out['gaze_class'][0, inside] == 3).all() and (out['gaze_class'] == 3).sum() == inside.sum()
    assert (t[inside] >= row[ref.R_T0]).all() and (t[inside] <= row[ref.R_T1]).all() and t[inside].max() == row[ref.R_T1]
    # the ramp runs from 0.5 to 1.5 s: the first candidate lies after its start and its window reaches at most window_s back; the
    # last candidate's window still holds motion, so it lies at most window_s (plus the filter's lag) after the ramp's end
    assert 0.3 <= row[ref.R_T0] <= 0.7 and 1.4 <= row[ref.R_T1] <= 1.8
    assert row[ref.R_MEAN] == row[ref.R_AMP] / (row[ref.R_T1] - row[ref.R_T0]) and row[ref.R_PATH] >= row[ref.R_AMP] * (1 - 1e-9)
    assert row[ref.R_MISSING] == 0 and row[ref.R_GAIN_N] == 0 and np.isnan(row[ref.R_GAIN]) and np.isnan(row[ref.R_ERR])
    assert (ex['gaze_event'][0, inside] == 1).all() and (ex['fixation_id'][0, inside] == row[ref.R_FIX]).all()      # the events' bits stay
    first = np.flatnonzero(inside)[0]
    assert out['pursuit_ms'][0, first] == np.float32(1000.0 * (t[first] - row[ref.R_T0])) and not out['pursuit_ms'][0, ~inside].any()
    assert table[0, ref.SUM_AMP] == row[ref.R_AMP] and table[0, ref.SUM_DUR] == row[ref.R_T1] - row[ref.R_T0] and table[0, ref.MAX_PEAK] == row[ref.R_PEAK]
    summary = pursuit_summary(table[0])
    assert summary['n'] == 1 and summary['pursuit_s'] == table[0, ref.SUM_DUR] and summary['mean_deg_s'] == row[ref.R_MEAN]
    assert np.isnan(summary['mean_gain']) and summary['max_peak_deg_s'] == row[ref.R_PEAK]


FPS = 120
SPEC = GazeEventSpec(fps=FPS)


def test_a_restart_aborts():
    pog, _ = ramp(FPS, 8.0)
    valid = np.ones(pog.shape[:2], dtype=np.uint8)
    valid[0, 120:132] = 0                                 # 12 frames in mid-ramp: 100 ms between samples, above max_gap_s
    ex, out, (state, table, store, count, _) = both(SPEC, PursuitSpec(max_missing=100), pog, valid)
    assert ex['sample'][0, 132] == 1 and table[0, ref.ABORTED] == 1 and out['gaze_class'][0, 132] == 0
    assert (out['pursuit_id'][0, 100:120] == 0).all() and (out['pursuit_id'][0, 120:132] == -1).all()
    # what follows the restart is a second episode of its own, which the first one's frames are no part of
    assert table[0, ref.ACCEPTED] == 1 and count[0] == 1 and store[0, 0, ref.R_ID] == 1 and store[0, 0, ref.R_T0] >= ex['sample_time'][0, 132]


def test_a_saccade_closes_at_the_previous_sample_and_the_settling_samples_stay_out():
    # a 10 degree jump within one frame in the middle of the ramp
    pog, _ = path(FPS, [(0.5, 0.0), (0.5, 8.0), (1.0 / FPS, 10.0 * FPS), (0.6, 8.0), (0.4, 0.0)])
    ex, out, (state, table, store, count, _) = both(SPEC, PursuitSpec(), pog)
    jump = np.flatnonzero(ex['gaze_event'][0] == 2)
    assert len(jump) >= 1 and (np.diff(jump) == 1).all() and only(table, ref.ACCEPTED, 2) and count[0] == 2
    t = ex['sample_time'][0]
    assert (out['gaze_class'][0, jump] == 2).all() and store[0, 0, ref.R_T1] == t[jump[0] - 1] and out['pursuit_id'][0, jump[0] - 1] == 0
    # the fixation samples of the first settle_s after the last saccade frame are in no window, and min_window_s passes before one fills
    after = np.flatnonzero((t > t[jump[-1]]) & (t - t[jump[-1]] < 0.08 + 0.1 - 1e-9))
    assert len(after) >= 20 and np.isnan(out['gaze_velocity_windowed'][0, after]).all() and (out['gaze_class'][0, after] == 1).all()
    assert store[0, 1, ref.R_T0] - t[jump[-1]] >= 0.08 and state[0, ref.SEEN_SACCADE] == 1 and state[0, ref.T_SACCADE] == t[jump[-1]]
    # settle_s = 0 admits them
    _, out0, (_, _, store0, _, _) = both(SPEC, PursuitSpec(settle_s=0.0), pog)
    assert store0[0, 1, ref.R_T0] == t[jump[-1] + 1] and np.isfinite(out0['gaze_velocity_windowed'][0, after]).any()


def test_missing_frames_interrupt_or_are_counted_and_short_and_small_episodes():
    pog, _ = ramp(FPS, 8.0)
    valid = np.ones(pog.shape[:2], dtype=np.uint8)
    valid[0, 120:125] = 0                                 # 5 frames in mid-ramp: 50 ms between samples, the chain holds
    ex, out, (_, table, _, count, _) = both(SPEC, PursuitSpec(), pog, valid)
    assert (ex['sample'][0, 120:125] == 0).all() and ex['sample'][0, 125] == 2 and only(table, ref.INTERRUPTED) and count[0] == 0
    assert (out['pursuit_id'][0, 120:125] == -1).all() and out['pursuit_id'][0, 119] == 0 and out['pursuit_id'][0, 125] == 0
    _, _, (_, table, store, count, _) = both(SPEC, PursuitSpec(max_missing=5), pog, valid)
    assert only(table, ref.ACCEPTED) and count[0] == 1 and store[0, 0, ref.R_MISSING] == 5
    _, _, (_, table, _, count, _) = both(SPEC, PursuitSpec(min_duration_s=2.0), pog)
    assert only(table, ref.SHORT) and count[0] == 0
    _, _, (_, table, _, count, _) = both(SPEC, PursuitSpec(min_amplitude_deg=20.0), pog)
    assert only(table, ref.SMALL) and count[0] == 0
    # the order of the judgement: interrupted before short before small
    _, _, (_, table, _, _, _) = both(SPEC, PursuitSpec(min_duration_s=2.0, min_amplitude_deg=20.0), pog, valid)
    assert only(table, ref.INTERRUPTED)
    _, _, (_, table, _, _, _) = both(SPEC, PursuitSpec(min_duration_s=2.0, min_amplitude_deg=20.0), pog)
    assert only(table, ref.SHORT)


def test_episodes_never_overlap_and_a_full_store_drops():
    """A threshold inside the jitter of the windowed velocity (8.05 on an 8 degrees / second ramp) makes the episode flicker: each
    new one's window reaches back into the one before, and its onset is the first sample after that one's end."""
    pog, _ = ramp(FPS, 8.0)
    flicker = PursuitSpec(pursuit_deg_s=8.05, min_duration_s=0.0, min_amplitude_deg=0.0)
    log = ref.new_log()
    ex, out, (state, table, store, count, dropped) = both(SPEC, flicker, pog, capacity=32, log=log)
    assert ref.thresholds_clear(flicker, log)
    n = int(count[0])
    assert n == 7 and only(table, ref.ACCEPTED, 7) and dropped[0] == 0 and store[0, :n, ref.R_ID].tolist() == list(range(7))
    rows, t = store[0, :n], ex['sample_time'][0]
    assert (rows[1:, ref.R_T0] > rows[:-1, ref.R_T1]).all()
    for a, b_ in zip(rows[:-1], rows[1:]):                # clamped: the very next sample
        assert b_[ref.R_T0] == t[np.flatnonzero(t == a[ref.R_T1])[0] + 1]
    assert (np.diff(np.flatnonzero(out['pursuit_id'][0] >= 0)) >= 1).all() and rows[:, ref.R_N].sum() == (out['gaze_class'] == 3).sum()
    _, _, (_, table4, store4, count4, dropped4) = both(SPEC, flicker, pog, capacity=4)
    assert count4[0] == 4 and dropped4[0] == 3 and np.array_equal(table4, table) and np.array_equal(store4[0], store[0, :4], equal_nan=True)


def frame_args(ex, point, a, b_):
    return [ex[k][:, a:b_] for k in ('sample', 'sample_time', 'gaze_vector')] + [point[:, a:b_]] + \
        [ex[k][:, a:b_] for k in ('gaze_event', 'gaze_velocity', 'fixation_id')]


def test_reset_aborts_and_keeps_next_id_and_the_table():
    pog, _ = ramp(FPS, 8.0)
    o, inv_cam, ppm = geometry(pog.shape[1])
    ex = sref.events_ex(SPEC, pog, o, inv_cam, ppm, *eref.fresh(1, 8))
    point = sref.point_of(SPEC, pog, ex)
    carried = ref.fresh(1, 8)
    ref.run(PursuitSpec(), *frame_args(ex, point, 0, 120), *carried)
    state, table = carried[0], carried[1]
    assert state[0, ref.OPEN] == 1 and state[0, ref.RING_N] == 32 and state[0, ref.NEXT_ID] == 1
    table[0, ref.ACCEPTED], table[0, ref.SUM_AMP] = 3.0, 12.5        # (tallies of an earlier life)
    out = ref.run(PursuitSpec(), None, None, None, None, None, None, None, *carried, reset=np.ones(1, dtype=np.int32))      # T = 0: the reset alone
    assert out['gaze_class'].shape == (1, 0) and table[0, ref.ABORTED] == 1 and table[0, ref.ACCEPTED] == 3 and table[0, ref.SUM_AMP] == 12.5
    assert state[0, ref.NEXT_ID] == 1 and not np.delete(state[0], ref.NEXT_ID).any()
    # the row alone was reset, the chain goes on: the rest of the ramp is a new episode with the next id
    out = ref.run(PursuitSpec(), *frame_args(ex, point, 120, pog.shape[1]), *carried)
    assert table[0, ref.ACCEPTED] == 4 and carried[2][0, 0, ref.R_ID] == 1 and carried[2][0, 0, ref.R_T0] == ex['sample_time'][0, 120]
    assert state[0, ref.NEXT_ID] == 2 and table[0, ref.ABORTED] == 1


def test_a_target_that_moves_with_the_ramp_gives_a_gain_near_one():
    pog, target = ramp(FPS, 8.0)
    ex, out, (_, table, store, count, _) = both(SPEC, PursuitSpec(), pog, target=target)
    row = store[0, 0]
    assert count[0] == 1 and row[ref.R_GAIN_N] == row[ref.R_N] > 0 and 0.9 <= row[ref.R_GAIN] <= 1.1 and 0 < row[ref.R_ERR] < 3 * DEG_PX
    inside = out['pursuit_id'][0] == 0
    gains = out['pursuit_gain'][0, inside]
    assert np.isfinite(gains).all() and abs(gains.astype(np.float64).mean() - row[ref.R_GAIN]) < 1e-6
    assert table[0, ref.TAB_GAIN_N] == row[ref.R_GAIN_N] and table[0, ref.SUM_GAIN] / table[0, ref.TAB_GAIN_N] == row[ref.R_GAIN]
    assert 0.9 <= pursuit_summary(table)['mean_gain'][0] <= 1.1
    # a target at rest has no displacement to project on: no gain; the classes do not look at the target at all
    assert np.isnan(out['pursuit_gain'][0, :int(0.5 * FPS)]).all()
    _, bare, (_, _, store_bare, _, _) = both(SPEC, PursuitSpec(), pog)
    for k in ('gaze_class', 'pursuit_id', 'pursuit_ms', 'gaze_velocity_windowed', 'gaze_straightness'):
        assert out[k].tobytes() == bare[k].tobytes(), k
    assert np.array_equal(store_bare[0, 0, :ref.R_GAIN_N], row[:ref.R_GAIN_N])
    # NaN targets: no gain anywhere
    _, out_nan, (_, table_nan, store_nan, _, _) = both(SPEC, PursuitSpec(), pog, target=np.full_like(target, np.nan))
    assert np.isnan(out_nan['pursuit_gain']).all() and store_nan[0, 0, ref.R_GAIN_N] == 0 and np.isnan(store_nan[0, 0, ref.R_GAIN])
    assert table_nan[0, ref.TAB_GAIN_N] == 0 and table_nan[0, ref.SUM_GAIN] == 0
    # partly NaN: only the windows whose two ends have a target count
    part = target.copy()
    part[0, 150:] = np.nan
    _, out_part, (_, _, store_part, _, _) = both(SPEC, PursuitSpec(), pog, target=part)
    assert np.isnan(out_part['pursuit_gain'][0, 150:]).all() and 0 < store_part[0, 0, ref.R_GAIN_N] < row[ref.R_GAIN_N]


# ---------------------------------------------------------------------------------------------------------------- splits
def two_streams():
    """Stream 0: a ramp with a jump in it and a target; stream 1: the flickering ramp backwards, its target partly missing."""
    a, ta = path(FPS, [(0.3, 0.0), (0.4, 8.0), (1.0 / FPS, 10.0 * FPS), (0.5, 8.0), (0.2, 0.0)])
    b_, tb = path(FPS, [(0.3, 0.0), (0.9, 8.0), (0.2, 0.0)], angle_deg=30.0, seed=9)
    T = min(a.shape[1], b_.shape[1])
    pog, target = np.concatenate([a[:, :T], b_[:, T - 1::-1]]), np.concatenate([ta[:, :T], tb[:, T - 1::-1]])
    target[1, 60:90] = np.nan
    valid = np.ones((2, T), dtype=np.uint8)
    valid[0, 50:53] = 0
    valid[1, 100:112] = 0
    return (pog,) + geometry(T, 2) + (valid, target)


def step_both(spec, pspec, ecarried, carried, pog, o, inv_cam, ppm, valid, target, lengths=None, reset=None, log=None):
    ex = sref.events_ex(spec, pog, o, inv_cam, ppm, *ecarried, valid=valid, lengths=lengths, reset=reset)
    return ref.run(pspec, ex['sample'], ex['sample_time'], ex['gaze_vector'], sref.point_of(spec, pog, ex), ex['gaze_event'],
                   ex['gaze_velocity'], ex['fixation_id'], *carried, target=target, lengths=lengths, reset=reset, log=log)


SCHEDULES = {
    'ones': [((1, 1), (0, 0))] * 170,
    'twos': [((2, 2), (0, 0))] * 85,
    'sevens': [((7, 7), (0, 0))] * 25,
    '64': [((64, 64), (0, 0))] * 3,
    '65': [((65, 65), (0, 0))] * 3,
    'mixed': [((64, 6), (0, 0)), ((0, 33), (0, 0)), ((9, 70), (0, 0)), ((65, 19), (0, 0)), ((1, 2), (0, 0)), ((30, 40), (0, 0))],
    'resets': [((33, 12), (0, 0)), ((52, 40), (1, 0)), ((5, 0), (0, 1)), ((70, 70), (0, 1)), ((8, 6), (1, 0)), ((0, 20), (1, 1))],
}
FLICKER = PursuitSpec(pursuit_deg_s=8.05, min_duration_s=0.0, min_amplitude_deg=0.0)


@pytest.mark.parametrize('name', list(SCHEDULES))
@pytest.mark.parametrize('pspec', [FLICKER, PursuitSpec()], ids=['flicker', 'default'])
def test_any_split_into_chunks_equals_one_pass(name, pspec):
    """Every stream consumes its frames in order; a schedule cuts them into chunks with ragged lengths and reset flags.  One pass: per
    stream, one call per stretch between two resets.  Outputs, state, table, store and counters, bit for bit."""
    spec = SPEC
    inputs = two_streams()
    T = inputs[0].shape[1]
    ecarried, carried, cursor = eref.fresh(2, 16), ref.fresh(2, 16), [0, 0]
    got = [{k: [] for k in PURSUIT_KEYS} for _ in range(2)]
    stretches = [[[0, 0, 0]], [[0, 0, 0]]]                 # per stream: [first frame, end, reset before it]
    padding = {'gaze_class': 0, 'pursuit_id': -1, 'pursuit_ms': 0.0}
    for lengths, reset in SCHEDULES[name]:
        lengths = [min(n, T - c) for n, c in zip(lengths, cursor)]
        W = max(max(lengths), 1)
        chunk = [np.zeros((2, W) + a.shape[2:], dtype=a.dtype) for a in inputs]
        for b in range(2):
            for dst, src in zip(chunk, inputs):
                dst[b, :lengths[b]] = src[b, cursor[b]:cursor[b] + lengths[b]]
        out = step_both(spec, pspec, ecarried, carried, *chunk, lengths=np.array(lengths), reset=np.array(reset))
        for b in range(2):
            for k in PURSUIT_KEYS:
                got[b][k].append(out[k][b, :lengths[b]])
                rest = out[k][b, lengths[b]:]
                assert (rest == padding[k]).all() if k in padding else np.isnan(rest).all(), k
            if reset[b]:
                stretches[b].append([cursor[b], cursor[b], 1])
            cursor[b] += lengths[b]
            stretches[b][-1][1] = cursor[b]
    assert min(cursor) > 100
    for b in range(2):
        ewhole, whole, want = eref.fresh(1, 16), ref.fresh(1, 16), {k: [] for k in PURSUIT_KEYS}
        for t0, t1, flag in stretches[b]:
            cut = [a[b:b + 1, t0:max(t1, t0 + 1)] for a in inputs]
            out = step_both(spec, pspec, ewhole, whole, *cut, lengths=np.array([t1 - t0]), reset=np.array([flag]))
            for k in PURSUIT_KEYS:
                want[k].append(out[k][0, :t1 - t0])
        for k in PURSUIT_KEYS:
            assert np.concatenate(got[b][k]).tobytes() == np.concatenate(want[k]).tobytes(), (b, k)
        for a, w in zip(carried, whole):
            assert a[b].tobytes() == w[0].tobytes(), b
    assert carried[1][:, [ref.ACCEPTED, ref.ABORTED]].sum() >= 2 and (np.concatenate(got[0]['gaze_class']) == 3).sum() > 5      # (episodes open across chunk borders)


# ---------------------------------------------------------------------------------------------------------------- the spec
def test_the_spec_compares_by_value_and_refuses_nonsense():
    a, b_ = PursuitSpec(pursuit_deg_s=2), PursuitSpec(pursuit_deg_s=2.0)
    assert a == b_ and hash(a) == hash(b_) and a.key() == b_.key() and a != PursuitSpec() and a != PursuitSpec(pursuit_deg_s=2, max_missing=2)
    assert a != 1 and len({a, b_, PursuitSpec()}) == 2 and eve_amd.PursuitSpec is PursuitSpec and 'PursuitSpec' in eve_amd.__all__
    d = PursuitSpec()
    assert (d.window_s, d.min_window_s, d.pursuit_deg_s, d.min_straightness, d.settle_s, d.min_duration_s, d.min_amplitude_deg,
            d.max_missing) == (0.2, 0.1, 3.0, 0.7, 0.08, 0.15, 1.0, 3) == d.key()
    assert eval(repr(a)) == a and repr(d).startswith('PursuitSpec(window_s=0.2, min_window_s=0.1, pursuit_deg_s=3.0, min_straightness=0.7')
    for name in ('window_s', 'min_window_s', 'pursuit_deg_s', 'min_straightness', 'settle_s', 'min_duration_s', 'min_amplitude_deg'):
        for bad in (-1.0, float('nan'), float('inf'), '1', True, None):
            with pytest.raises(ValueError, match=name):
                PursuitSpec(**{name: bad})
    for name in ('window_s', 'min_window_s', 'pursuit_deg_s', 'min_straightness'):
        with pytest.raises(ValueError, match=name):
            PursuitSpec(**{name: 0})
    with pytest.raises(ValueError, match='min_window_s'):
        PursuitSpec(window_s=0.1, min_window_s=0.2)
    with pytest.raises(ValueError, match='min_straightness'):
        PursuitSpec(min_straightness=1.01)
    assert PursuitSpec(settle_s=0, min_duration_s=0, min_amplitude_deg=0, min_straightness=1, min_window_s=0.2).key()[1:7] == (0.2, 3.0, 1.0, 0.0, 0.0, 0.0)
    for bad in (-1, 1.5, float('nan'), '1', True, None):
        with pytest.raises(ValueError, match='max_missing'):
            PursuitSpec(max_missing=bad)
    assert len(PURSUIT_COLUMNS) == 18 and len(PURSUIT_TABLE) == 12 and PURSUIT_COLUMNS[ref.R_DIR] == 'direction_deg' and PURSUIT_TABLE[ref.SHORT] == 'short'
    with pytest.raises(ValueError, match='16'):
        pursuit_summary(np.zeros((2, 8)))
    many = pursuit_summary(torch.zeros(3, 16, dtype=torch.float64))
    assert many['n'].shape == (3,) and np.isnan(many['mean_deg_s']).all() and np.isnan(many['mean_gain']).all()


# ---------------------------------------------------------------------------------------------------------------- EVEStream
class PursuitFakes(SaccadeFakes):
    """SaccadeFakes plus gaze_pursuits, evaluated by tests/pursuit_ref.py."""

    def gaze_pursuits(self, sample, sample_time, gaze_vector, point, event, velocity, fixation_id, spec, state, table, store, count, dropped,
                      target=None, lengths=None, reset=None):
        self.calls.append('gaze_pursuits' if sample is not None else 'gaze_pursuits[0]')
        n = lambda t: None if t is None else t.detach().numpy()
        out = ref.run(spec, n(sample), n(sample_time), n(gaze_vector), n(point), n(event), n(velocity), n(fixation_id), n(state), n(table),
                      n(store), n(count), n(dropped), target=n(target), lengths=n(lengths), reset=n(reset))
        return {k: torch.from_numpy(v) for k, v in out.items()} if sample is not None else {}


@pytest.fixture()
def fake():
    k = PursuitFakes()
    kernels.set_default_kernels(k)
    yield k
    kernels.set_default_kernels(None)
    eve_amd.reset_standalone_config()


B, T, CHUNKS = 2, 3, 4
EVENTS = GazeEventSpec(fps=30, saccade_deg_s=1e9)          # every chained frame is a fixation frame
# ... and every one with a window (two samples do) is a candidate
ALWAYS = PursuitSpec(window_s=0.1, min_window_s=0.03, pursuit_deg_s=1e-9, min_straightness=1e-9, settle_s=0.0, min_duration_s=0.0,
                     min_amplitude_deg=0.0)


@pytest.fixture()
def scene(fake):
    model, _ = make_model(dict(refine_net_rnn_type='CGRU'))
    batch = clip(B, CHUNKS * T, size=32)
    return model, [chunk_of(batch, i * T, (i + 1) * T) for i in range(CHUNKS)]


def run(stream, chunk, **kw):
    return {k: v.clone() for k, v in stream.step(chunk, **kw).items()}


def reference_step(out, chunk, spec, pspec, ecarried, carried, lengths=None, reset=None, valid=None, target=None):
    """The reference on the step's own results: the source PoG and the binocular origin."""
    o = torch.stack([chunk['left_o'], chunk['right_o']], dim=-1).mean(dim=-1)
    n = lambda t: t.numpy()
    return step_both(spec, pspec, ecarried, carried, n(out['PoG_px_final']), n(o), n(chunk['inv_camera_transformation']),
                     n(chunk['pixels_per_millimeter']), valid, target, lengths=lengths, reset=reset)


def test_a_step_without_pursuits_is_the_step_it_always_was_and_one_with_them_adds_six_keys_and_one_launch(fake, scene):
    model, chunks = scene
    s0 = eve_amd.EVEStream(model, B, use_graph=False)
    bare = run(s0, chunks[0])
    calls_bare = list(fake.calls)
    del fake.calls[:]
    with_events = run(eve_amd.EVEStream(model, B, use_graph=False), chunks[0], events=EVENTS)
    calls_events = list(fake.calls)
    assert calls_events == calls_bare + ['gaze_events'] and sorted(with_events) == sorted(list(bare) + list(GAZE_EVENT_KEYS))
    del fake.calls[:]
    s1 = eve_amd.EVEStream(model, B, use_graph=False)
    with_saccades = run(s1, chunks[0], events=EVENTS, saccades=SaccadeSpec())
    assert fake.calls == calls_bare + ['gaze_events_ex', 'gaze_saccades'] and sorted(with_saccades) == sorted(list(with_events) + list(SACCADE_KEYS))
    assert s0._pursuits is None and s1._pursuits is None and not any('pursuit' in c or c == 'gaze_class' for c in with_saccades)      # nothing allocated
    # pursuits alone, and after the saccade launch
    s = eve_amd.EVEStream(model, B, use_graph=False, pursuit_capacity=8)
    s2 = eve_amd.EVEStream(model, B, use_graph=False)
    ecarried, carried = eref.fresh(B, 256), ref.fresh(B, 8)
    for i, c in enumerate(chunks):
        del fake.calls[:]
        out = run(s, c, events=EVENTS, pursuits=ALWAYS)
        assert fake.calls == calls_bare + ['gaze_events_ex', 'gaze_pursuits']
        del fake.calls[:]
        out2 = run(s2, c, events=EVENTS, saccades=SaccadeSpec(), pursuits=ALWAYS)
        assert fake.calls == calls_bare + ['gaze_events_ex', 'gaze_saccades', 'gaze_pursuits']
        if i == 0:
            assert sorted(out) == sorted(list(with_events) + list(PURSUIT_KEYS))      # the three _ex arrays stay internal
            assert sorted(out2) == sorted(list(with_saccades) + list(PURSUIT_KEYS))
            for k in with_events:
                assert out[k].numpy().tobytes() == with_events[k].numpy().tobytes(), k
            for k in with_saccades:
                assert out2[k].numpy().tobytes() == with_saccades[k].numpy().tobytes(), k
            assert [out[k].dtype for k in PURSUIT_KEYS] == [torch.uint8, torch.int32] + [torch.float32] * 4
            assert all(tuple(out[k].shape) == (B, T) for k in PURSUIT_KEYS)
        want = reference_step(out, c, EVENTS, ALWAYS, ecarried, carried)
        for k in PURSUIT_KEYS:
            assert out[k].numpy().tobytes() == want[k].tobytes() == out2[k].numpy().tobytes(), (i, k)
    state, table, store, count, dropped = carried
    assert (state[:, ref.OPEN] == 1).all() and (out['gaze_class'] == 3).all() and (out['pursuit_id'] == 0).all()      # one episode, open across the chunks
    # the accessors
    assert np.array_equal(s.get_pursuit_state().numpy(), state, equal_nan=True) and np.array_equal(s.pursuit_table().numpy(), table)
    assert s.pursuit_counts()[0].tolist() == count.tolist() and s.pursuit_counts()[1].tolist() == dropped.tolist()
    # a step whose every frame is a saccade frame closes the episodes: rows
    closing = GazeEventSpec(fps=30, saccade_deg_s=1e-9)
    out = run(s, chunks[0], events=closing, pursuits=ALWAYS)
    want = reference_step(out, chunks[0], closing, ALWAYS, ecarried, carried)
    assert (out['gaze_class'] == 2).all() and out['gaze_class'].numpy().tobytes() == want['gaze_class'].tobytes()
    assert count.tolist() == [1, 1] and s.pursuit_counts()[0].tolist() == [1, 1] and np.array_equal(s.pursuit_table().numpy(), table)
    rows = s.pursuits()
    assert [r.shape for r in rows] == [(1, 20), (1, 20)] and all(np.array_equal(r, store[b, :1], equal_nan=True) for b, r in enumerate(rows))
    assert len(s.pursuits([1])) == 1 and s.pursuit_table() is not s.pursuit_table()
    assert pursuit_summary(s.pursuit_table())['n'].tolist() == [1, 1]
    # the state round trip; get_state() does not hold the row
    saved = s.get_pursuit_state()
    s.set_pursuit_state(torch.zeros(B, 320))
    assert not s.get_pursuit_state().any()
    s.set_pursuit_state(saved.numpy())
    assert s.get_pursuit_state().numpy().tobytes() == saved.numpy().tobytes() and not any('pursuit' in k for k in s.get_state())
    # clear_pursuits: the store and the counters; the table only on request
    s.clear_pursuits([0])
    assert s.pursuit_counts()[0].tolist() == [0, 1] and np.array_equal(s.pursuit_table().numpy(), table)
    s.clear_pursuits(table=True)
    assert s.pursuit_counts()[0].tolist() == [0, 0] and not s.pursuit_table().any() and s.get_pursuit_state().numpy().tobytes() == saved.numpy().tobytes()
    # the carried buffers are the step's to put back
    assert all(any(t is c_ for c_ in s._carried()) for t in s._pursuit_buffers())


def test_the_chunks_pursuit_target_reaches_the_launch(fake, scene):
    model, chunks = scene
    s = eve_amd.EVEStream(model, B, use_graph=False)
    ecarried, carried = eref.fresh(B, 256), ref.fresh(B, 256)
    gains = []
    for i, c in enumerate(chunks[:3]):
        c = dict(c)
        c['pursuit_target'] = torch.arange(B * T * 2, dtype=torch.float32).reshape(B, T, 2) * 7.0 + 100.0 * i
        out = run(s, c, events=EVENTS, pursuits=ALWAYS)
        want = reference_step(out, c, EVENTS, ALWAYS, ecarried, carried, target=c['pursuit_target'].numpy())
        for k in PURSUIT_KEYS:
            assert out[k].numpy().tobytes() == want[k].tobytes(), (i, k)
        gains.append(out['pursuit_gain'])
    assert torch.isfinite(torch.cat(gains, dim=1)[:, 1:]).all() and (s.get_pursuit_state()[:, ref.GAIN_N] > 0).all()


def test_refusals_come_before_any_launch(fake, scene):
    model, chunks = scene
    s = eve_amd.EVEStream(model, B, use_graph=False)
    with pytest.raises(ValueError, match='events='):
        s.step(chunks[0], pursuits=PursuitSpec())
    with pytest.raises(ValueError, match='PursuitSpec'):
        s.step(chunks[0], events=EVENTS, pursuits=dict(window_s=1))
    with pytest.raises(ValueError, match='PursuitSpec'):
        s.step(chunks[0], events=EVENTS, pursuits=SaccadeSpec())
    with pytest.raises(ValueError, match='frame_time'):
        s.step(chunks[0], events=GazeEventSpec(), pursuits=PursuitSpec())
    for bad in (torch.zeros(B, T, 2, dtype=torch.float64), torch.zeros(B, T, 3), torch.zeros(B, T + 1, 2), np.zeros((B, T, 2), dtype=np.float32)):
        with pytest.raises(ValueError, match='pursuit_target'):
            s.step(dict(chunks[0], pursuit_target=bad), events=EVENTS, pursuits=PursuitSpec())
    with pytest.raises(ValueError, match='pursuit_capacity'):
        eve_amd.EVEStream(model, B, use_graph=False, pursuit_capacity=0)
    with pytest.raises(ValueError, match='state'):
        s.set_pursuit_state(np.zeros((B, 32)))
    assert fake.calls == []


def test_the_graph_key_holds_the_spec_and_the_targets_presence(fake, scene):
    model, chunks = scene
    c0 = chunks[0]
    s = eve_amd.EVEStream(model, B, use_graph=False)
    events = s._check_events(c0, EVENTS, B, T)
    plan = lambda pspec, chunk=c0: s._check_pursuits(chunk, pspec, events, B, T)
    bare = s._graph_key(c0, False, False, False, None, events)
    a = s._graph_key(c0, False, False, False, None, events, pursuits=plan(PursuitSpec()))
    assert a != bare and a == s._graph_key(dict(c0), False, False, False, None, events, pursuits=plan(PursuitSpec(window_s=0.2)))
    assert a != s._graph_key(c0, False, False, False, None, events, pursuits=plan(PursuitSpec(max_missing=1)))
    assert a != s._graph_key(c0, False, False, False, None, events, saccades=s._check_saccades(SaccadeSpec(), events))
    ct = dict(c0, pursuit_target=torch.zeros(B, T, 2))
    with_target = plan(PursuitSpec(), ct)
    assert with_target['target'] and not plan(PursuitSpec())['target']
    assert s._graph_key(ct, False, False, False, None, events, pursuits=with_target) != a
    captured = []
    s._capture = lambda chunk, *a_, **k_: captured.append((a_, k_)) or {'n': len(captured)}
    first = s._graph_for(c0, False, False, False, None, events, pursuits=plan(PursuitSpec()))
    assert s._graph_for(c0, False, False, False, None, events, pursuits=plan(PursuitSpec())) is first and len(captured) == 1
    assert captured[0][1]['pursuits']['spec'] == PursuitSpec()
    assert s._graph_for(c0, False, False, False, None, events) is not first and captured[1][1] == {}      # (no pursuits: _capture's old call)


def test_reset_aborts_and_an_events_only_step_is_followed_by_a_resynchronising_launch(fake, scene):
    model, chunks = scene
    s = eve_amd.EVEStream(model, B, use_graph=False)
    out = run(s, chunks[0], events=EVENTS, pursuits=ALWAYS)
    assert out['pursuit_id'].tolist() == [[-1, 0, 0]] * B and out['gaze_class'].tolist() == [[0, 3, 3]] * B
    assert (s.get_pursuit_state()[:, ref.OPEN] == 1).all() and np.allclose(out['pursuit_ms'].numpy(), [[0, 1000 / 30.0, 2000 / 30.0]] * B)
    # reset(): the flagged stream's open episode is aborted inside the step's own launch, its ids run on
    s.reset([1])
    del fake.calls[:]
    out = run(s, chunks[1], events=EVENTS, pursuits=ALWAYS)
    assert 'gaze_pursuits[0]' not in fake.calls and out['pursuit_id'].tolist() == [[0, 0, 0], [-1, 1, 1]]
    assert s.pursuit_table()[:, ref.ABORTED].tolist() == [0, 1] and s.get_pursuit_state()[:, ref.NEXT_ID].tolist() == [1, 2]
    # a reset before a step WITHOUT the stage still reaches its row: one launch with no frames
    s.reset([0])
    del fake.calls[:]
    run(s, chunks[2])
    assert fake.calls[0] == 'gaze_pursuits[0]' and fake.calls.count('gaze_pursuits[0]') == 1 and 'gaze_saccades[0]' not in fake.calls
    assert s.pursuit_table()[:, ref.ABORTED].tolist() == [1, 1] and s.get_pursuit_state()[:, ref.OPEN].tolist() == [0, 1]
    assert s.get_pursuit_state()[:, ref.RING_N].tolist() == [0, 3] and not s._pursuits_stale      # (neither chain moved)
    # an events-only step moves the chain on without the stage; the next pursuits step first starts every row afresh, eagerly
    del fake.calls[:]
    run(s, chunks[2], events=EVENTS)
    assert not any(c.startswith('gaze_pursuits') for c in fake.calls) and fake.calls[-1] == 'gaze_events' and s._pursuits_stale
    del fake.calls[:]
    out = run(s, chunks[3], events=EVENTS, pursuits=ALWAYS)
    assert fake.calls[0] == 'gaze_pursuits[0]' and fake.calls[-2:] == ['gaze_events_ex', 'gaze_pursuits'] and not s._pursuits_stale
    assert s.pursuit_table()[:, ref.ABORTED].tolist() == [1, 2]
    # the run starts afresh with this chunk's first frame: a window needs a second sample
    assert out['gaze_class'].tolist() == [[1, 3, 3]] * B and (s.get_pursuit_state()[:, ref.RING_N] == 3).all()
    del fake.calls[:]
    run(s, chunks[0], events=EVENTS, pursuits=ALWAYS)
    assert 'gaze_pursuits[0]' not in fake.calls
    # a saccades-only step stales the pursuit row and not the saccade row; set_event_state() cuts both ties
    run(s, chunks[1], events=EVENTS, saccades=SaccadeSpec())
    assert s._pursuits_stale and not s._saccades_stale
    run(s, chunks[2], events=EVENTS, saccades=SaccadeSpec(), pursuits=ALWAYS)
    assert not s._pursuits_stale
    s.set_event_state(s.get_event_state())
    assert s._pursuits_stale and s._saccades_stale


def test_pursuits_on_ragged_and_masked_steps(fake, scene):
    model, chunks = scene
    s = eve_amd.EVEStream(model, B, use_graph=False)
    ecarried, carried = eref.fresh(B, 256), ref.fresh(B, 256)
    out = run(s, chunks[0], events=EVENTS, pursuits=ALWAYS, lengths=[2, 0])
    want = reference_step(out, chunks[0], EVENTS, ALWAYS, ecarried, carried, lengths=np.array([2, 0]))
    for k in PURSUIT_KEYS:
        assert out[k][0, :2].numpy().tobytes() == want[k][0, :2].tobytes(), k
    assert out['gaze_class'].tolist() == [[0, 3, 0], [0, 0, 0]] and (out['pursuit_id'][1] == -1).all() and torch.isnan(out['pursuit_gain']).all()
    assert np.array_equal(s.get_pursuit_state().numpy(), carried[0], equal_nan=True) and not carried[0][1].any()
    mask = torch.ones(B, T, 2, dtype=torch.bool)
    mask[0, 1] = False                                    # stream 0, frame 1: no usable eye
    s = eve_amd.EVEStream(model, B, use_graph=False)
    out = run(s, chunks[0], events=EVENTS, pursuits=ALWAYS, eye_mask=mask)
    assert out['pursuit_id'].tolist() == [[-1, -1, 0], [-1, 0, 0]] and s.get_pursuit_state()[:, ref.MISSING].tolist() == [0, 0]
    out = run(s, dict(chunks[1]), events=EVENTS, pursuits=ALWAYS, eye_mask=mask)
    assert out['pursuit_id'].tolist() == [[0, -1, 0], [0, 0, 0]] and s.get_pursuit_state()[:, ref.MISSING].tolist() == [1, 0]


def test_the_stand_alone_entry_returns_events_pursuits_and_tallies(fake):
    from eve_amd import data
    pog, target = ramp(FPS, 8.0)
    o, inv_cam, ppm = geometry(pog.shape[1])
    t = torch.from_numpy
    res = data.gaze_pursuits(t(pog), t(o), t(inv_cam), t(ppm), SPEC, PursuitSpec(), target=t(target), pursuit_capacity=4)
    assert fake.calls == ['gaze_events_ex', 'gaze_pursuits']
    assert sorted(res) == sorted(list(GAZE_EVENT_KEYS) + list(PURSUIT_KEYS) + ['pursuits', 'pursuit_count', 'pursuit_dropped', 'pursuit_table'])
    _, out, (_, table, store, count, dropped) = both(SPEC, PursuitSpec(), pog, target=target, capacity=4)
    assert np.array_equal(res['pursuits'].numpy(), store, equal_nan=True) and np.array_equal(res['pursuit_table'].numpy(), table)
    assert res['pursuit_count'].tolist() == [1] and res['pursuit_dropped'].tolist() == [0]
    for k in PURSUIT_KEYS:
        assert res[k].numpy().tobytes() == out[k].tobytes(), k
    assert 0.9 <= data.pursuit_summary(res['pursuit_table'])['mean_gain'][0] <= 1.1
    with pytest.raises(ValueError, match='PursuitSpec'):
        data.gaze_pursuits(t(pog), t(o), t(inv_cam), t(ppm), SPEC, SPEC)
    with pytest.raises(ValueError, match='GazeEventSpec'):
        data.gaze_pursuits(t(pog), t(o), t(inv_cam), t(ppm), PursuitSpec(), PursuitSpec())
    with pytest.raises(ValueError, match='pursuit_capacity'):
        data.gaze_pursuits(t(pog), t(o), t(inv_cam), t(ppm), SPEC, PursuitSpec(), pursuit_capacity=0)
    with pytest.raises(TypeError, match='target'):
        data.gaze_pursuits(t(pog), t(o), t(inv_cam), t(ppm), SPEC, PursuitSpec(), target=t(target[:, :5]))
    with pytest.raises(ValueError, match='frame_time'):
        data.gaze_pursuits(t(pog), t(o), t(inv_cam), t(ppm), GazeEventSpec(), PursuitSpec())
