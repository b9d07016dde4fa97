"""CPU: saccades as events -- the numpy contract (tests/saccade_ref.py) on the scan path of test_gaze_events_host.py, on one small path
per rule and under chunk splits with ragged lengths and resets; eve_amd.SaccadeSpec; data.main_sequence against numpy.polyfit; and the
EVEStream plumbing (step(events=..., saccades=...), the refusals, the graph key, reset, the resynchronising launch, the accessors, the
state round trip) over a stand-in whose gaze_events_ex and gaze_saccades are the reference itself.  The GPU suite
(test_gpu_saccades.py) checks the HIP kernels."""
import numpy as np
import pytest
import torch

import eve_amd
import gaze_events_ref as eref
import saccade_ref as ref
from eve_amd import kernels
from eve_amd.data import GAZE_EVENT_KEYS, SACCADE_KEYS, GazeEventSpec, SaccadeSpec, main_sequence
from test_gaze_events_host import DEG_PX, EYE, POINTS, PPM, EventFakes, scan_path
from test_stream_host import chunk_of, clip, make_model

FPS = 120


# ---------------------------------------------------------------------------------------------------------------- the contract
def geometry(T):
    return (np.tile(EYE.astype(np.float32), (1, T, 1)), np.tile(np.eye(4, dtype=np.float32), (1, T, 1, 1)), np.full((1, T, 2), PPM, dtype=np.float32))


def both(spec, sspec, pog, valid=None, capacity=8, log=None, elog=None):
    """The events and the saccades of one clip [1, T, 2], from fresh state -> (ex, out, (state, table, store, count, dropped))."""
    o, inv_cam, ppm = geometry(pog.shape[1])
    ex = ref.events_ex(spec, pog, o, inv_cam, ppm, *eref.fresh(1, 64), valid=valid, log=elog)
    carried = ref.fresh(1, capacity)
    out = ref.run(sspec, ex['sample'], ex['sample_time'], ex['gaze_vector'], ref.point_of(spec, pog, ex), ex['gaze_event'], ex['gaze_velocity'],
                  ex['fixation_id'], *carried, log=log)
    return ex, out, carried


def test_the_scan_path_gives_its_two_saccades_raw():
    spec = GazeEventSpec(fps=FPS, velocity_from='raw')
    pog, _, _, _, valid, seg = scan_path(FPS)
    ex, out, (state, table, store, count, dropped) = both(spec, SaccadeSpec(), pog, valid)
    assert count[0] == 2 and dropped[0] == 0 and table[0, ref.ACCEPTED] == 2 and not table[0, ref.ABORTED:].any()
    rows = store[0, :2]
    assert (9.9 <= rows[:, ref.R_AMP]).all() and (rows[:, ref.R_AMP] <= 10.0 + 1e-2).all()
    assert rows[:, [ref.R_PREV_FIX, ref.R_NEXT_FIX]].tolist() == [[0, 1], [2, 3]] and rows[:, ref.R_ID].tolist() == [0, 1]
    assert (rows[:, ref.R_MISSING] == 0).all() and not store[0, 2:].any()
    # nothing comes out of the 150 ms hole: no id inside it, and the restart after it aborted nothing
    hole = valid[0] == 0
    assert (out['saccade_id'][0, hole] == -1).all() and (ex['sample'][0, hole] == 0).all() and ex['sample'][0, np.flatnonzero(seg == 4)[0]] == 1
    # the third saccade is still open at the clip's end: it has an id, and no row
    assert state[0, ref.OPEN] == 1 and state[0, ref.ID] == 2 and state[0, ref.NEXT_ID] == 3 and out['saccade_id'][0, -1] == 2
    # per frame: the ids mark exactly the counted frames, ms runs from the onset sample
    for row in rows:
        inside = out['saccade_id'][0] == int(row[ref.R_ID])
        assert inside.sum() == row[ref.R_N] and (ex['gaze_event'][0, inside] == 2).all()
        first = np.flatnonzero(inside)[0]
        assert ex['sample_time'][0, first - 1] == row[ref.R_T0] and ex['sample_time'][0, np.flatnonzero(inside)[-1]] == row[ref.R_T1]
        assert out['saccade_ms'][0, first] == np.float32(1000.0 * (ex['sample_time'][0, first] - row[ref.R_T0]))
        assert row[ref.R_MEAN] == row[ref.R_AMP] / (row[ref.R_T1] - row[ref.R_T0])
        assert row[ref.R_PEAK] == ex['gaze_velocity'][0, inside].astype(np.float64).max()
    assert (out['saccade_ms'][0][out['saccade_id'][0] < 0] == 0).all()


def test_the_scan_path_gives_two_shorter_saccades_filtered():
    """The amplitude is that of the point the velocity is from: the one-euro filter's lag shortens it."""
    spec = GazeEventSpec(fps=FPS)
    pog, _, _, _, valid, _ = scan_path(FPS)
    _, _, (state, table, store, count, _) = both(spec, SaccadeSpec(), pog, valid)
    assert count[0] == 2 and table[0, ref.ACCEPTED] == 2 and state[0, ref.OPEN] == 1
    assert (9.3 < store[0, :2, ref.R_AMP]).all() and (store[0, :2, ref.R_AMP] < 9.6).all()
    assert store[0, :2, [ref.R_PREV_FIX, ref.R_NEXT_FIX]].T.tolist() == [[0, 1], [2, 3]]


@pytest.mark.parametrize('fps,lo,hi', [(30, 8.85, 8.95), (60, 9.15, 9.25), (120, 9.45, 9.55)])
def test_the_documented_amplitudes_of_the_filtered_point(fps, lo, hi):
    pog, _, _, _, valid, _ = scan_path(fps)
    _, _, (_, _, store, count, _) = both(GazeEventSpec(fps=fps), SaccadeSpec(), pog, valid)
    assert count[0] >= 1 and lo < store[0, 0, ref.R_AMP] < hi
    _, _, (_, _, store, count, _) = both(GazeEventSpec(fps=fps, velocity_from='raw'), SaccadeSpec(), pog, valid)
    assert count[0] >= 1 and 9.85 < store[0, 0, ref.R_AMP] < 10.05


def small_path(steps_deg, tail=10):
    """10 fixation frames at A, then one frame per entry of steps_deg at A + that many degrees to the right, then `tail` frames at the
    last position: [1, T, 2] float32 at 120 fps, no jitter."""
    x = [0.0] * 10 + list(steps_deg) + [steps_deg[-1]] * tail
    pog = np.zeros((1, len(x), 2), dtype=np.float32)
    pog[0, :, 0] = POINTS['A'][0] + np.array(x) * DEG_PX
    pog[0, :, 1] = POINTS['A'][1]
    return pog


RAW = GazeEventSpec(fps=FPS, velocity_from='raw')
RAMP = [2.0, 4.0, 6.0, 8.0, 10.0]


def judged(pog, sspec, valid=None):
    log, elog = ref.new_log(), eref.new_log()
    ex, out, carried = both(RAW, sspec, pog, valid, log=log, elog=elog)
    assert ref.thresholds_clear(sspec, log) and eref.thresholds_clear(RAW, elog)      # every path runs clear of every threshold
    return ex, out, carried


def only(table, column):
    """The table counts one saccade, under `column`."""
    tallies = [ref.ACCEPTED, ref.ABORTED, ref.SMALL, ref.SHORT, ref.LONG, ref.INTERRUPTED]
    return all(table[0, c] == (1 if c == column else 0) for c in tallies)


def test_a_ramp_is_accepted():
    ex, out, (state, table, store, count, _) = judged(small_path(RAMP), SaccadeSpec())
    assert only(table, ref.ACCEPTED) and count[0] == 1 and state[0, ref.OPEN] == 0
    row = store[0, 0]
    assert row[ref.R_N] == 5 and 9.8 < row[ref.R_AMP] < 10.1 and row[ref.R_MISSING] == 0
    assert row[ref.R_T0] == 9 / FPS and row[ref.R_T1] == 14 / FPS and out['saccade_id'][0].tolist() == [-1] * 10 + [0] * 5 + [-1] * 10
    assert (row[ref.R_X0], row[ref.R_Y0]) == (POINTS['A'][0], POINTS['A'][1]) and row[ref.R_X1] == small_path(RAMP)[0, 14, 0]
    assert [row[ref.R_PREV_FIX], row[ref.R_NEXT_FIX]] == [0, 1] and 230 < row[ref.R_PEAK] < 250
    assert table[0, ref.SUM_A] == row[ref.R_AMP] and table[0, ref.SUM_AP] == row[ref.R_AMP] * row[ref.R_PEAK] and table[0, ref.MAX_P] == row[ref.R_PEAK]
    assert table[0, ref.SUM_D] == row[ref.R_T1] - row[ref.R_T0] and table[0, ref.SUM_AD] == row[ref.R_AMP] * (row[ref.R_T1] - row[ref.R_T0])


def test_a_missing_frame_interrupts_or_is_counted():
    pog = small_path(RAMP)
    valid = np.ones(pog.shape[:2], dtype=np.uint8)
    valid[0, 12] = 0                                      # the ramp's third frame
    _, out, (_, table, _, count, _) = judged(pog, SaccadeSpec(max_missing=0), valid)
    assert only(table, ref.INTERRUPTED) and count[0] == 0 and out['saccade_id'][0, 10:15].tolist() == [0, 0, -1, 0, 0]
    _, _, (_, table, store, count, _) = judged(pog, SaccadeSpec(max_missing=1), valid)
    assert only(table, ref.ACCEPTED) and count[0] == 1 and store[0, 0, ref.R_N] == 4 and store[0, 0, ref.R_MISSING] == 1


def test_a_hole_aborts():
    pog = small_path(RAMP, tail=20)
    valid = np.ones(pog.shape[:2], dtype=np.uint8)
    valid[0, 12:22] = 0                                   # 10 frames from mid-ramp on: 92 ms between samples, above max_gap_s
    ex, out, (state, table, _, count, _) = judged(pog, SaccadeSpec(max_missing=100), valid)
    assert ex['sample'][0, 22] == 1 and only(table, ref.ABORTED) and count[0] == 0 and state[0, ref.OPEN] == 0
    assert out['saccade_id'][0, 10:12].tolist() == [0, 0] and (out['saccade_id'][0, 12:] == -1).all() and state[0, ref.NEXT_ID] == 1


def test_a_small_a_long_and_a_short_saccade():
    _, _, (_, table, _, count, _) = judged(small_path([0.3]), SaccadeSpec())
    assert only(table, ref.SMALL) and count[0] == 0
    _, _, (_, table, _, count, _) = judged(small_path([10.0 * (i + 1) / 30 for i in range(30)]), SaccadeSpec())
    assert only(table, ref.LONG) and count[0] == 0
    _, _, (_, table, _, count, _) = judged(small_path([2.0]), SaccadeSpec(min_duration_s=0.02))
    assert only(table, ref.SHORT) and count[0] == 0
    _, _, (_, table, store, count, _) = judged(small_path([2.0]), SaccadeSpec(min_duration_s=0.0))
    assert only(table, ref.ACCEPTED) and count[0] == 1 and store[0, 0, ref.R_N] == 1 and store[0, 0, ref.R_T1] - store[0, 0, ref.R_T0] == 10 / FPS - 9 / FPS


def test_a_full_store_drops_and_nothing_opens_in_the_middle_of_a_run():
    pog = np.concatenate([small_path(RAMP), small_path(RAMP), small_path(RAMP)], axis=1)
    _, _, (_, table, store, count, dropped) = both(RAW, SaccadeSpec(), pog, capacity=2)
    # (the jumps back to A between the parts are saccades too: five in all)
    assert table[0, ref.ACCEPTED] == 5 and count[0] == 2 and dropped[0] == 3 and store[0, :, ref.R_ID].tolist() == [0, 1]
    # a row reset on its own in the middle of a saccade: the rest of that run opens nothing
    o, inv_cam, ppm = geometry(pog.shape[1])
    ex = ref.events_ex(RAW, pog, o, inv_cam, ppm, *eref.fresh(1, 8))
    carried = ref.fresh(1, 8)
    args = lambda a, b_: [ex[k][:, a:b_] for k in ('sample', 'sample_time', 'gaze_vector')] + [pog[:, a:b_]] + \
        [ex[k][:, a:b_] for k in ('gaze_event', 'gaze_velocity', 'fixation_id')]
    ref.run(SaccadeSpec(), *args(0, 12), *carried)
    assert carried[0][0, ref.OPEN] == 1
    out = ref.run(SaccadeSpec(), *args(12, 30), *carried, reset=np.ones(1, dtype=np.int32))
    assert carried[1][0, ref.ABORTED] == 1 and (out['saccade_id'][0, :3] == -1).all() and carried[1][0, ref.ACCEPTED] == 1
    assert carried[2][0, 0, ref.R_ID] == 1 and carried[0][0, ref.NEXT_ID] == 2        # the jump back to A: the next id


# ---------------------------------------------------------------------------------------------------------------- splits
def two_streams():
    a, _, _, _, va, _ = scan_path(FPS)
    b_, _, _, _, vb, _ = scan_path(FPS, seed=9)
    pog, valid = np.concatenate([a, b_[:, ::-1]]), np.concatenate([va, vb[:, ::-1]])      # (stream 1: the path backwards)
    o, inv_cam, ppm = geometry(pog.shape[1])
    return pog, np.tile(o, (2, 1, 1)), np.tile(inv_cam, (2, 1, 1, 1)), np.tile(ppm, (2, 1, 1)), valid


def step_both(spec, sspec, ecarried, carried, pog, o, inv_cam, ppm, valid, lengths=None, reset=None):
    ex = ref.events_ex(spec, pog, o, inv_cam, ppm, *ecarried, valid=valid, lengths=lengths, reset=reset)
    return ref.run(sspec, ex['sample'], ex['sample_time'], ex['gaze_vector'], ref.point_of(spec, pog, ex), ex['gaze_event'],
                   ex['gaze_velocity'], ex['fixation_id'], *carried, lengths=lengths, reset=reset)


SCHEDULES = {
    'ones': [((1, 1), (0, 0))] * 128,
    'sevens': [((7, 7), (0, 0))] * 19,
    'ragged': [((64, 6), (0, 0)), ((0, 33), (0, 0)), ((9, 70), (0, 0)), ((55, 19), (0, 0))],
    'resets': [((33, 12), (0, 0)), ((12, 40), (1, 0)), ((5, 0), (0, 1)), ((70, 70), (0, 1)), ((8, 6), (1, 0))],
}


@pytest.mark.parametrize('name', list(SCHEDULES))
@pytest.mark.parametrize('velocity_from', ['raw', 'filtered'])
def test_any_split_into_chunks_equals_one_pass(name, velocity_from):
    """Every stream consumes its frames in order; a schedule cuts them into chunks with ragged lengths and reset flags.  One pass: per
    stream, one call per stretch between two resets."""
    spec, sspec = GazeEventSpec(fps=FPS, velocity_from=velocity_from), SaccadeSpec()
    inputs = two_streams()
    T = inputs[0].shape[1]
    ecarried, carried, cursor = eref.fresh(2, 16), ref.fresh(2, 16), [0, 0]
    got = [{k: [] for k in SACCADE_KEYS} for _ in range(2)]
    stretches = [[[0, 0, 0]], [[0, 0, 0]]]                 # per stream: [first frame, end, reset before it]
    for lengths, reset in SCHEDULES[name]:
        lengths = [min(n, T - c) for n, c in zip(lengths, cursor)]
        W = max(max(lengths), 1)
        chunk = [np.zeros((2, W) + a.shape[2:], dtype=a.dtype) for a in inputs]
        for b in range(2):
            for dst, src in zip(chunk, inputs):
                dst[b, :lengths[b]] = src[b, cursor[b]:cursor[b] + lengths[b]]
        out = step_both(spec, sspec, ecarried, carried, *chunk, lengths=np.array(lengths), reset=np.array(reset))
        for b in range(2):
            for k in SACCADE_KEYS:
                got[b][k].append(out[k][b, :lengths[b]])
                assert (out[k][b, lengths[b]:] == (-1 if k == 'saccade_id' else 0)).all()
            if reset[b]:
                stretches[b].append([cursor[b], cursor[b], 1])
            cursor[b] += lengths[b]
            stretches[b][-1][1] = cursor[b]
    assert min(cursor) > 100
    for b in range(2):
        ewhole, whole, want = eref.fresh(1, 16), ref.fresh(1, 16), {k: [] for k in SACCADE_KEYS}
        for t0, t1, flag in stretches[b]:
            cut = [a[b:b + 1, t0:max(t1, t0 + 1)] for a in inputs]
            out = step_both(spec, sspec, ewhole, whole, *cut, lengths=np.array([t1 - t0]), reset=np.array([flag]))
            for k in SACCADE_KEYS:
                want[k].append(out[k][0, :t1 - t0])
        for k in SACCADE_KEYS:
            assert np.concatenate(got[b][k]).tobytes() == np.concatenate(want[k]).tobytes(), (b, k)
        for a, w in zip(carried, whole):
            assert a[b].tobytes() == w[0].tobytes(), b
    assert carried[1][:, ref.ACCEPTED].sum() >= 2         # (saccades open across several chunk borders)


# ---------------------------------------------------------------------------------------------------------------- the spec
def test_the_spec_compares_by_value_and_refuses_nonsense():
    a, b_ = SaccadeSpec(min_amplitude_deg=1), SaccadeSpec(min_amplitude_deg=1.0)
    assert a == b_ and hash(a) == hash(b_) and a.key() == b_.key() and a != SaccadeSpec() and a != SaccadeSpec(min_amplitude_deg=1, max_missing=2)
    assert a != 1 and len({a, b_, SaccadeSpec()}) == 2 and eve_amd.SaccadeSpec is SaccadeSpec and 'SaccadeSpec' in eve_amd.__all__
    d = SaccadeSpec()
    assert (d.min_amplitude_deg, d.min_duration_s, d.max_duration_s, d.max_missing) == (0.5, 0.0, 0.2, 0) == d.key()
    assert repr(d) == 'SaccadeSpec(min_amplitude_deg=0.5, min_duration_s=0.0, max_duration_s=0.2, max_missing=0)' and eval(repr(a)) == a
    for name in ('min_amplitude_deg', 'min_duration_s', 'max_duration_s'):
        for bad in (-1.0, float('nan'), float('inf'), '1', True, None):
            with pytest.raises(ValueError, match=name):
                SaccadeSpec(**{name: bad})
    with pytest.raises(ValueError, match='max_duration_s'):
        SaccadeSpec(max_duration_s=0)
    assert SaccadeSpec(min_amplitude_deg=0, min_duration_s=0).key()[:2] == (0.0, 0.0)
    for bad in (-1, 1.5, float('nan'), '1', True, None):
        with pytest.raises(ValueError, match='max_missing'):
            SaccadeSpec(max_missing=bad)


# ---------------------------------------------------------------------------------------------------------------- the main sequence
def test_the_main_sequence_equals_polyfit_on_the_stored_rows():
    steps = []
    for amp, frames in ((2.0, 2), (4.0, 3), (6.0, 3), (8.0, 4), (10.0, 5), (3.0, 2)):      # out and back, every amplitude its own duration
        ramp = [amp * (i + 1) / frames for i in range(frames)]
        steps += ramp + [amp] * 10 + ramp[-2::-1] + [0.0] + [0.0] * 10
    _, _, (_, table, store, count, _) = both(RAW, SaccadeSpec(), small_path(steps), capacity=32)
    assert count[0] == 12 and table[0, ref.ACCEPTED] == 12
    rows = store[0, :12]
    amp, dur, peak = rows[:, ref.R_AMP], rows[:, ref.R_T1] - rows[:, ref.R_T0], rows[:, ref.R_PEAK]
    fit = main_sequence(table[0])
    close = lambda a, b_: abs(a - b_) <= 1e-9 * max(1.0, abs(b_))
    d_slope, d_icpt = np.polyfit(amp, dur, 1)
    p_slope, p_icpt = np.polyfit(amp, peak, 1)
    assert close(fit['duration_slope'], d_slope) and close(fit['duration_intercept'], d_icpt)
    assert close(fit['peak_slope'], p_slope) and close(fit['peak_intercept'], p_icpt)
    assert fit['n'] == 12 and close(fit['mean_amplitude_deg'], amp.mean()) and fit['max_amplitude_deg'] == amp.max() and fit['max_peak_deg_s'] == peak.max()
    assert d_slope > 0                                    # longer saccades for larger amplitudes: the path was built that way
    # a tensor [S, 16]: per stream; fewer than 2 saccades or no spread in amplitude: NaN
    one = ref.fresh(1, 4)
    ref_rows = np.stack([table[0], np.zeros(16), one[1][0]])
    ref_rows[2, :7] = [3, 3 * 5.0, 3 * 25.0, 3 * 100.0, 3 * 500.0, 3 * 0.04, 3 * 0.2]      # three equal saccades
    many = main_sequence(torch.from_numpy(ref_rows))
    assert many['duration_slope'].shape == (3,) and close(many['duration_slope'][0], d_slope)
    for k in ('duration_slope', 'duration_intercept', 'peak_slope', 'peak_intercept'):
        assert np.isnan(many[k][1:]).all(), k
    assert np.isnan(many['mean_amplitude_deg'][1]) and many['mean_amplitude_deg'][2] == 5.0
    single = np.zeros(16)
    single[:7] = [1, 5.0, 25.0, 100.0, 500.0, 0.04, 0.2]
    assert np.isnan(main_sequence(single)['peak_slope'])
    with pytest.raises(ValueError, match='16'):
        main_sequence(np.zeros((2, 8)))


# ---------------------------------------------------------------------------------------------------------------- EVEStream
class SaccadeFakes(EventFakes):
    """EventFakes plus gaze_events_ex and gaze_saccades, evaluated by tests/saccade_ref.py."""

    def gaze_events_ex(self, pog, origin, inv_cam, ppm, spec, state, store, count, dropped, frame_time=None, valid=None, lengths=None,
                       reset=None, flush=None):
        self.calls.append('gaze_events_ex')
        n = lambda t: None if t is None else t.detach().numpy()
        out = ref.events_ex(spec, n(pog), n(origin), n(inv_cam), n(ppm), n(state), n(store), n(count), n(dropped), frame_time=n(frame_time),
                            valid=n(valid), lengths=n(lengths), reset=n(reset), flush=n(flush))
        return {k: torch.from_numpy(v) for k, v in out.items()}

    def gaze_saccades(self, sample, sample_time, gaze_vector, point, event, velocity, fixation_id, spec, state, table, store, count, dropped,
                      lengths=None, reset=None):
        self.calls.append('gaze_saccades' if sample is not None else 'gaze_saccades[0]')
        n = lambda t: None if t is None else t.detach().numpy()
        out = ref.run(spec, n(sample), n(sample_time), n(gaze_vector), n(point), n(event), n(velocity), n(fixation_id), n(state), n(table),
                      n(store), n(count), n(dropped), lengths=n(lengths), reset=n(reset))
        return {k: torch.from_numpy(v) for k, v in out.items()} if sample is not None else {}


@pytest.fixture()
def fake():
    k = SaccadeFakes()
    kernels.set_default_kernels(k)
    yield k
    kernels.set_default_kernels(None)
    eve_amd.reset_standalone_config()


B, T, CHUNKS = 2, 3, 4
SACCADES = SaccadeSpec(min_amplitude_deg=0.0, max_duration_s=10.0)


@pytest.fixture()
def scene(fake):
    model, _ = make_model(dict(refine_net_rnn_type='CGRU'))
    batch = clip(B, CHUNKS * T, size=32)
    chunks = [chunk_of(batch, i * T, (i + 1) * T) for i in range(CHUNKS)]
    # a threshold in the middle of the clip's own velocities: some frames of either kind
    s = eve_amd.EVEStream(model, B, use_graph=False)
    v = torch.cat([s.step(c, events=GazeEventSpec(fps=30, saccade_deg_s=1e9))['gaze_velocity'].clone() for c in chunks], dim=1)
    del fake.calls[:]
    return model, chunks, GazeEventSpec(fps=30, saccade_deg_s=float(v[torch.isfinite(v)].median()))


def run(stream, chunk, **kw):
    return {k: v.clone() for k, v in stream.step(chunk, **kw).items()}


def reference_step(out, chunk, spec, sspec, ecarried, carried, lengths=None, reset=None, valid=None):
    """The reference on the step's own results: the source PoG and the binocular origin."""
    o = torch.stack([chunk['left_o'], chunk['right_o']], dim=-1).mean(dim=-1)
    n = lambda t: t.numpy()
    return step_both(spec, sspec, ecarried, carried, n(out['PoG_px_final']), n(o), n(chunk['inv_camera_transformation']),
                     n(chunk['pixels_per_millimeter']), valid, lengths=lengths, reset=reset)


def test_a_step_with_saccades_adds_two_keys_and_one_launch(fake, scene):
    model, chunks, spec = scene
    s0 = eve_amd.EVEStream(model, B, use_graph=False)
    with_events = run(s0, chunks[0], events=spec)
    calls_events = list(fake.calls)
    assert calls_events[-1] == 'gaze_events' and 'gaze_events_ex' not in calls_events and s0._saccades is None      # nothing new, nothing allocated
    del fake.calls[:]
    s = eve_amd.EVEStream(model, B, use_graph=False, saccade_capacity=8)
    ecarried, carried = eref.fresh(B, 256), ref.fresh(B, 8)
    for i, c in enumerate(chunks):
        del fake.calls[:]
        out = run(s, c, events=spec, saccades=SACCADES)
        assert fake.calls == calls_events[:-1] + ['gaze_events_ex', 'gaze_saccades']      # _ex in place of the events launch, then one more
        if i == 0:
            assert sorted(out) == sorted(list(with_events) + list(SACCADE_KEYS))      # the three _ex arrays stay internal
            for k in with_events:
                assert out[k].numpy().tobytes() == with_events[k].numpy().tobytes(), k
            assert out['saccade_id'].dtype == torch.int32 and out['saccade_ms'].dtype == torch.float32 and tuple(out['saccade_ms'].shape) == (B, T)
        want = reference_step(out, c, spec, SACCADES, ecarried, carried)
        for k in SACCADE_KEYS:
            assert out[k].numpy().tobytes() == want[k].tobytes(), (i, k)
    state, table, store, count, dropped = carried
    assert count.sum() >= 1 and table[:, ref.ACCEPTED].sum() == count.sum()      # (the clip does hold completed saccades)
    # the accessors
    assert np.array_equal(s.get_saccade_state().numpy(), state) and np.array_equal(s.saccade_table().numpy(), table)
    assert s.saccade_counts()[0].tolist() == count.tolist() and s.saccade_counts()[1].tolist() == dropped.tolist()
    rows = s.saccades()
    assert [r.shape for r in rows] == [(int(c_), 16) for c_ in count] and all(np.array_equal(r, store[b, :count[b]]) for b, r in enumerate(rows))
    assert len(s.saccades([1])) == 1 and s.saccade_table() is not s.saccade_table()
    assert np.array_equal(s.get_event_state().numpy(), ecarried[0])
    fit = main_sequence(s.saccade_table())
    assert fit['n'].tolist() == count.tolist()
    # the state round trip; get_state() does not hold the row
    saved = s.get_saccade_state()
    s.set_saccade_state(torch.zeros(B, 32))
    assert not s.get_saccade_state().any()
    s.set_saccade_state(saved.numpy())
    assert torch.equal(s.get_saccade_state(), saved) and not any('saccade' in k for k in s.get_state())
    # clear_saccades: the store and the counters; the table only on request
    s.clear_saccades([0])
    assert s.saccade_counts()[0].tolist() == [0, int(count[1])] and np.array_equal(s.saccade_table().numpy(), table)
    s.clear_saccades(table=True)
    assert s.saccade_counts()[0].tolist() == [0, 0] and not s.saccade_table().any() and torch.equal(s.get_saccade_state(), saved)
    # the carried buffers are the step's to put back
    assert all(any(t is c_ for c_ in s._carried()) for t in s._saccade_buffers())


def test_refusals_come_before_any_launch(fake, scene):
    model, chunks, spec = scene
    s = eve_amd.EVEStream(model, B, use_graph=False)
    with pytest.raises(ValueError, match='events='):
        s.step(chunks[0], saccades=SaccadeSpec())
    with pytest.raises(ValueError, match='SaccadeSpec'):
        s.step(chunks[0], events=spec, saccades=dict(min_amplitude_deg=1))
    with pytest.raises(ValueError, match='SaccadeSpec'):
        s.step(chunks[0], events=spec, saccades=spec)
    with pytest.raises(ValueError, match='frame_time'):
        s.step(chunks[0], events=GazeEventSpec(), saccades=SaccadeSpec())
    with pytest.raises(ValueError, match='saccade_capacity'):
        eve_amd.EVEStream(model, B, use_graph=False, saccade_capacity=0)
    with pytest.raises(ValueError, match='state'):
        s.set_saccade_state(np.zeros((B, 31)))
    assert fake.calls == []


def test_the_graph_key_holds_the_spec(fake, scene):
    model, chunks, spec = scene
    c0 = chunks[0]
    s = eve_amd.EVEStream(model, B, use_graph=False)
    events = s._check_events(c0, spec, B, T)
    plan = lambda sspec: s._check_saccades(sspec, events)
    bare = s._graph_key(c0, False, False, False, None, events)
    a = s._graph_key(c0, False, False, False, None, events, saccades=plan(SaccadeSpec()))
    assert a != bare and a == s._graph_key(dict(c0), False, False, False, None, events, saccades=plan(SaccadeSpec(min_amplitude_deg=0.5)))
    assert a != s._graph_key(c0, False, False, False, None, events, saccades=plan(SaccadeSpec(max_missing=1)))
    captured = []
    s._capture = lambda chunk, *a_, **k_: captured.append((a_, k_)) or {'n': len(captured)}
    first = s._graph_for(c0, False, False, False, None, events, saccades=plan(SaccadeSpec()))
    assert s._graph_for(c0, False, False, False, None, events, saccades=plan(SaccadeSpec())) is first and len(captured) == 1
    assert captured[0][1]['saccades']['spec'] == SaccadeSpec()
    assert s._graph_for(c0, False, False, False, None, events) is not first and captured[1][1] == {}      # (no saccades: _capture's old call)


def test_reset_aborts_and_an_events_only_step_is_followed_by_a_resynchronising_launch(fake, scene):
    model, chunks, spec = scene
    always = GazeEventSpec(fps=30, saccade_deg_s=1e-9)    # every chained frame is a saccade frame
    s = eve_amd.EVEStream(model, B, use_graph=False)
    out = run(s, chunks[0], events=always, saccades=SACCADES)
    assert out['saccade_id'].tolist() == [[-1, 0, 0]] * B and (s.get_saccade_state()[:, ref.OPEN] == 1).all()
    assert np.allclose(out['saccade_ms'].numpy(), [[0, 1000 / 30.0, 2000 / 30.0]] * B)
    # reset(): the flagged stream's open saccade is aborted inside the step's own launch, its ids run on
    s.reset([1])
    del fake.calls[:]
    out = run(s, chunks[1], events=always, saccades=SACCADES)
    assert 'gaze_saccades[0]' not in fake.calls and out['saccade_id'].tolist() == [[0, 0, 0], [-1, 1, 1]]
    assert s.saccade_table()[:, ref.ABORTED].tolist() == [0, 1] and s.get_saccade_state()[:, ref.NEXT_ID].tolist() == [1, 2]
    # a reset before a step WITHOUT the stage still reaches its row: one launch with no frames
    s.reset([0])
    del fake.calls[:]
    run(s, chunks[2])
    assert fake.calls[:2] == ['gaze_saccades[0]', 'gaze_events'] and fake.calls.count('gaze_saccades[0]') == 1
    assert s.saccade_table()[:, ref.ABORTED].tolist() == [1, 1] and s.get_saccade_state()[:, ref.OPEN].tolist() == [0, 1]
    assert not s._saccades_stale                          # (neither chain moved)
    # an events-only step moves the chain on without the stage; the next saccades step first starts every row afresh, eagerly
    del fake.calls[:]
    run(s, chunks[2], events=always)
    assert 'gaze_saccades' not in fake.calls and 'gaze_saccades[0]' not in fake.calls and fake.calls[-1] == 'gaze_events' and s._saccades_stale
    del fake.calls[:]
    out = run(s, chunks[3], events=always, saccades=SACCADES)
    assert fake.calls[0] == 'gaze_saccades[0]' and fake.calls[-2:] == ['gaze_events_ex', 'gaze_saccades'] and not s._saccades_stale
    assert s.saccade_table()[:, ref.ABORTED].tolist() == [1, 2]
    # the run under way is not reported (nothing opens in the middle of a run), and the stage is in step again
    assert (out['saccade_id'] == -1).all() and (s.get_saccade_state()[:, ref.HAS_PREV] == 1).all()
    del fake.calls[:]
    run(s, chunks[0], events=always, saccades=SACCADES)
    assert 'gaze_saccades[0]' not in fake.calls
    # set_event_state() cuts the tie as well
    s.set_event_state(s.get_event_state())
    assert s._saccades_stale


def test_saccades_on_ragged_and_masked_steps(fake, scene):
    model, chunks, spec = scene
    s = eve_amd.EVEStream(model, B, use_graph=False)
    ecarried, carried = eref.fresh(B, 256), ref.fresh(B, 256)
    out = run(s, chunks[0], events=spec, saccades=SACCADES, lengths=[2, 0])
    want = reference_step(out, chunks[0], spec, SACCADES, ecarried, carried, lengths=np.array([2, 0]))
    for k in SACCADE_KEYS:
        assert out[k][0, :2].numpy().tobytes() == want[k][0, :2].tobytes(), k
    assert (out['saccade_id'][:, 2:] == -1).all() and (out['saccade_id'][1] == -1).all()
    assert np.array_equal(s.get_saccade_state().numpy(), carried[0]) and not carried[0][1].any()
    mask = torch.ones(B, T, 2, dtype=torch.bool)
    mask[0, 1] = False                                    # stream 0, frame 1: no usable eye
    s = eve_amd.EVEStream(model, B, use_graph=False)
    always = GazeEventSpec(fps=30, saccade_deg_s=1e-9)
    out = run(s, chunks[0], events=always, saccades=SaccadeSpec(min_amplitude_deg=0, max_missing=0))
    assert out['saccade_id'].tolist() == [[-1, 0, 0]] * B
    s = eve_amd.EVEStream(model, B, use_graph=False)
    out = run(s, chunks[0], events=always, saccades=SACCADES, eye_mask=mask)
    assert out['saccade_id'].tolist() == [[-1, -1, 0], [-1, 0, 0]] and s.get_saccade_state()[:, ref.MISSING].tolist() == [0, 0]
    out = run(s, dict(chunks[1]), events=always, saccades=SACCADES, eye_mask=mask)
    assert out['saccade_id'].tolist() == [[0, -1, 0], [0, 0, 0]] and s.get_saccade_state()[:, ref.MISSING].tolist() == [1, 0]


def test_the_stand_alone_entry_returns_events_saccades_and_tallies(fake):
    from eve_amd import data
    pog, o, inv_cam, ppm, valid, _ = scan_path(FPS)
    t = torch.from_numpy
    res = data.gaze_saccades(t(pog), t(o), t(inv_cam), t(ppm), RAW, SaccadeSpec(), valid=t(valid), saccade_capacity=4)
    assert fake.calls == ['gaze_events_ex', 'gaze_saccades']
    assert sorted(res) == sorted(list(GAZE_EVENT_KEYS) + list(SACCADE_KEYS) + ['saccades', 'saccade_count', 'saccade_dropped', 'saccade_table'])
    _, out, (_, table, store, count, dropped) = both(RAW, SaccadeSpec(), pog, valid, capacity=4)
    assert np.array_equal(res['saccades'].numpy(), store) and np.array_equal(res['saccade_table'].numpy(), table)
    assert res['saccade_count'].tolist() == [2] and res['saccade_dropped'].tolist() == [0]
    for k in SACCADE_KEYS:
        assert res[k].numpy().tobytes() == out[k].tobytes(), k
    with pytest.raises(ValueError, match='SaccadeSpec'):
        data.gaze_saccades(t(pog), t(o), t(inv_cam), t(ppm), RAW, RAW)
    with pytest.raises(ValueError, match='GazeEventSpec'):
        data.gaze_saccades(t(pog), t(o), t(inv_cam), t(ppm), SaccadeSpec(), SaccadeSpec())
    with pytest.raises(ValueError, match='saccade_capacity'):
        data.gaze_saccades(t(pog), t(o), t(inv_cam), t(ppm), RAW, SaccadeSpec(), saccade_capacity=0)
    with pytest.raises(ValueError, match='frame_time'):
        data.gaze_saccades(t(pog), t(o), t(inv_cam), t(ppm), GazeEventSpec(), SaccadeSpec())
