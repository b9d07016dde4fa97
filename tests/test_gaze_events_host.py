"""CPU: the gaze filter and the fixation / saccade events -- the numpy contract (tests/gaze_events_ref.py) on a synthetic scan path
and under chunk splits, eve_amd.GazeEventSpec, and the EVEStream plumbing (step(events=...), the refusals, the graph key, reset, the
fixation store, the overlay's marker keys) over a stand-in whose gaze_events is the reference itself.  The GPU suite
(test_gpu_gaze_events.py) checks the HIP kernel."""
import math

import numpy as np
import pytest
import torch

import eve_amd
import gaze_events_ref as ref
from eve_amd import kernels
from eve_amd.data import GAZE_EVENT_KEYS, GazeEventSpec, OverlaySpec
from test_overlay_host import OverlayFakes, stream_chunk
from test_stream_host import chunk_of, clip, make_model
from test_stream_mask_host import MaskFakes

# ---------------------------------------------------------------------------------------------------------------- the scan path
PPM = 3.6                                                # pixels per millimetre
EYE = np.array([265.0, 150.0, 600.0])                    # the eye in screen millimetres: 600 mm in front of the screen
DEG_PX = 600.0 * math.tan(math.radians(1.0)) * PPM       # one degree on the screen under the eye, in pixels
JITTER_PX = 0.1 * DEG_PX                                 # 0.1 degrees: the bound of the jitter's length
POINTS = {'A': (700.0, 500.0), 'B': (700.0 + 10 * DEG_PX, 500.0), 'C': (700.0 + 10 * DEG_PX, 500.0 + 5 * DEG_PX),
          'D': (700.0, 500.0 + 5 * DEG_PX), 'E': (700.0, 500.0)}
# (start, end, from, to, kind): fixation 300 ms, a 10 degree saccade over 40 ms, fixation 200 ms, a 150 ms hole, fixation 250 ms, a
# saccade, a 33 ms fixation, a saccade
SEGMENTS = [(0.000, 0.300, 'A', 'A', 'fix'), (0.300, 0.340, 'A', 'B', 'sac'), (0.340, 0.540, 'B', 'B', 'fix'), (0.540, 0.690, 'B', 'C', 'hole'),
            (0.690, 0.940, 'C', 'C', 'fix'), (0.940, 0.980, 'C', 'D', 'sac'), (0.980, 1.013, 'D', 'D', 'fix'), (1.013, 1.053, 'D', 'E', 'sac')]
LONG = ('A', 'B', 'C')


def scan_path(fps, jitter=True, seed=5):
    """-> (pog [1, T, 2] float32, o, inv_cam, ppm, valid uint8 [1, T], segment index per frame); frame i at i / fps."""
    rng = np.random.RandomState(seed)
    T = int(math.floor(1.06 * fps)) + 1
    pog, valid, seg = np.zeros((1, T, 2), dtype=np.float32), np.ones((1, T), dtype=np.uint8), np.full(T, len(SEGMENTS) - 1)
    for i in range(T):
        t = i / fps
        for s, (t0, t1, a, b_, kind) in enumerate(SEGMENTS):
            if t0 <= t < t1 or s == len(SEGMENTS) - 1:
                w = min(max((t - t0) / (t1 - t0), 0.0), 1.0)
                p = (1 - w) * np.array(POINTS[a]) + w * np.array(POINTS[b_])
                seg[i] = s
                if kind == 'hole':
                    valid[0, i] = 0
                if kind == 'fix' and jitter:
                    p = p + rng.uniform(-1, 1, 2) * JITTER_PX / math.sqrt(2.0)
                pog[0, i] = p
                break
    o = np.tile(EYE.astype(np.float32), (1, T, 1))
    inv_cam = np.tile(np.eye(4, dtype=np.float32), (1, T, 1, 1))
    ppm = np.full((1, T, 2), PPM, dtype=np.float32)
    return pog, o, inv_cam, ppm, valid, seg


def one_pass(spec, inputs, capacity=8, flush=True):
    pog, o, inv_cam, ppm, valid, _ = inputs
    state, store, count, dropped = ref.fresh(1, capacity)
    out = ref.run(spec, pog, o, inv_cam, ppm, state, store, count, dropped, valid=valid, flush=np.ones(1, dtype=np.int32) if flush else None)
    return out, state, store, count, dropped


@pytest.mark.parametrize('fps', [30, 120])
def test_the_scan_path_gives_its_three_long_fixations(fps):
    inputs = scan_path(fps)
    out, state, store, count, dropped = one_pass(GazeEventSpec(fps=fps), inputs)
    seg = inputs[5]
    assert count[0] == 3 and dropped[0] == 0          # the three long ones: not the 33 ms one, nothing out of the hole
    rows = store[0, :3]
    assert (np.diff(rows[:, 0]) > 0).all()             # ids increase
    for row, name in zip(rows, LONG):
        s = [i for i, sg in enumerate(SEGMENTS) if sg[2] == name and sg[4] == 'fix'][0]
        t0, t1 = SEGMENTS[s][:2]
        # (the frame in which a saccade sets out has moved for less than a frame's time, and the filter behind the velocity has not
        # followed it yet: it may still belong to the fixation)
        assert t0 - 1e-9 <= row[1] and row[2] < t1 + 1.0 / fps + 1e-9 and row[2] - row[1] >= 0.06
        # every sample of the fixation lies within the jitter of the truth, so does their mean (+ the float32 rounding of a pixel)
        assert np.hypot(row[4] - POINTS[name][0], row[5] - POINTS[name][1]) <= JITTER_PX + 1e-3
        assert row[6] <= JITTER_PX + 1e-3 and row[3] == np.sum((out['fixation_id'][0] == int(row[0])))
    ev = out['gaze_event'][0]
    assert (ev[inputs[4][0] == 0] == 0).all()          # the hole has no events
    hole_end = np.flatnonzero(seg == 4)[0]
    assert ev[hole_end] == 0 and np.isnan(out['gaze_velocity'][0, hole_end])      # the first sample after the gap: no velocity
    assert (out['PoG_px_filtered'][0, hole_end] == inputs[0][0, hole_end]).all()
    for s_, sg in enumerate(SEGMENTS):                 # every saccade is seen (the filter behind the velocity may miss its onset frame)
        assert sg[4] != 'sac' or (ev[seg == s_] == 2).any(), s_
    assert (out['fixation_id'][0][ev != 1] == -1).all() and (out['fixating'][0][ev != 1] == 0).all()
    assert state[0, ref.FIX_OPEN] == 0


@pytest.mark.parametrize('fps', [30, 120])
def test_the_filter_follows_a_step_as_fast_as_its_formulas_say(fps):
    """A step of A = 10 degrees, no jitter.  From the filter's formulas: at the step's sample the derivative estimate is ad * A / dt
    (it was 0), so that sample's alpha is a1 = alpha(min_cutoff + beta * ad * A / dt) and the error left is (1 - a1) * A; every later
    sample multiplies the error by 1 - alpha_k <= 1 - alpha(min_cutoff), the cutoff never being below min_cutoff.  So the error k
    samples after the step is at most (1 - a1) * (1 - a_min)^k * A, and the filtered point is within the raw jitter (0.1 degree) of
    the target after K = ceil(log(J / ((1 - a1) * A)) / log(1 - a_min)) samples at the latest."""
    spec = GazeEventSpec(fps=fps)
    T, A = 200, 10 * DEG_PX
    pog = np.zeros((1, T, 2), dtype=np.float32)
    pog[0, :, 0], pog[0, :, 1] = 700.0, 500.0
    pog[0, 10:, 0] += np.float32(A)
    A = float(pog[0, 10, 0]) - 700.0
    o, inv_cam, ppm = np.tile(EYE.astype(np.float32), (1, T, 1)), np.tile(np.eye(4, dtype=np.float32), (1, T, 1, 1)), np.full((1, T, 2), PPM, np.float32)
    state, store, count, dropped = ref.fresh(1, 4)
    out = ref.run(spec, pog, o, inv_cam, ppm, state, store, count, dropped)
    dt = 1.0 / fps
    alpha = lambda fc: 1.0 / (1.0 + (1.0 / (2 * math.pi * fc)) / dt)
    a1, a_min = alpha(spec.min_cutoff_hz + spec.beta * alpha(spec.d_cutoff_hz) * A / dt), alpha(spec.min_cutoff_hz)
    err = np.abs(out['PoG_px_filtered'][0, 10:, 0].astype(np.float64) - (700.0 + A))
    bound = (1 - a1) * (1 - a_min) ** np.arange(T - 10) * A
    assert (err <= bound * (1 + 1e-9) + 1e-3).all()   # (+ the float32 rounding of the output)
    K = int(math.ceil(math.log(JITTER_PX / ((1 - a1) * A)) / math.log(1 - a_min)))
    assert 0 < K < T - 10 and (err[K:] <= JITTER_PX).all()
    assert (out['PoG_px_filtered'][0, :10, 0] == 700.0).all() and (out['PoG_px_filtered'][0, :, 1] == 500.0).all()


def test_raw_and_filtered_velocities_differ_where_expected():
    """120 fps, inside the first fixation (every sample within J of the truth).  Raw: consecutive points are at most 2 J apart.
    Filtered: the filtered point is a convex combination of earlier samples, so the next raw sample is at most 2 J from it per
    axis pair and the filter moves by alpha times that, alpha <= alpha(min_cutoff + beta * 2 J / dt) because the derivative
    estimate is a convex combination of raw derivatives of at most 2 J / dt.  A segment of length L seen from at least d = 600 mm
    subtends at most L / d radians."""
    fps, dt = 120, 1.0 / 120
    inputs = scan_path(fps)
    seg = inputs[5]
    raw, *_ = one_pass(GazeEventSpec(fps=fps, velocity_from='raw'), inputs)
    fil, *_ = one_pass(GazeEventSpec(fps=fps), inputs)
    inside = np.flatnonzero(seg == 0)[1:]
    alpha = lambda fc: 1.0 / (1.0 + (1.0 / (2 * math.pi * fc)) / dt)
    deg_s = lambda px: math.degrees(px / PPM / 600.0) / dt
    raw_bound = deg_s(2 * JITTER_PX)
    fil_bound = deg_s(math.sqrt(2.0) * alpha(1.0 + 0.007 * 2 * JITTER_PX / dt) * 2 * JITTER_PX)
    assert fil_bound < 0.5 * raw_bound < 0.5 * 30.0
    assert (raw['gaze_velocity'][0, inside] <= raw_bound * (1 + 1e-6)).all() and (fil['gaze_velocity'][0, inside] <= fil_bound * (1 + 1e-6)).all()
    assert raw['gaze_velocity'][0, inside].max() > fil_bound          # the jitter the filter takes out is there in the raw signal
    moving = [i for i in range(1, len(seg)) if SEGMENTS[seg[i]][4] == 'sac' and SEGMENTS[seg[i - 1]][4] == 'sac' and i / fps < 1.053]
    assert moving and (raw['gaze_event'][0, moving] == 2).all()       # the raw point moves at 125 or 250 deg/s in every such frame
    # the filter lags behind a saccade: after the landing it is still moving, so it labels no fewer frames a saccade
    assert (fil['gaze_event'] == 2).sum() >= (raw['gaze_event'] == 2).sum() > 0
    assert np.array_equal(raw['PoG_px_filtered'], fil['PoG_px_filtered'])      # the filter itself does not depend on the choice


@pytest.mark.parametrize('sizes', [[1, None], [None, 1], [7] * 40, [64, 6, None], [33, None]], ids=['1+rest', 'rest+1', 'sevens', '64+6', '33'])
@pytest.mark.parametrize('timed', [False, True])
def test_any_split_into_chunks_equals_one_pass(sizes, timed):
    fps = 120
    pog, o, inv_cam, ppm, valid, _ = scan_path(fps)
    T = pog.shape[1]
    ft = None
    if timed:                                             # explicit times: a jittered clock
        ft = (np.arange(T) / fps + np.random.RandomState(1).uniform(0, 2e-3, T))[None]
    spec = GazeEventSpec(fps=None if timed else fps)
    whole = ref.fresh(1, 8)
    want = ref.run(spec, pog, o, inv_cam, ppm, *whole, frame_time=ft, valid=valid)
    parts, got, t0 = ref.fresh(1, 8), [], 0
    for n in sizes:
        n = T - t0 - (1 if sizes[-1] == 1 and n is None else 0) if n is None else min(n, T - t0)
        if n <= 0:
            break
        cut = lambda a: None if a is None else a[:, t0:t0 + n]
        got.append(ref.run(spec, cut(pog), cut(o), cut(inv_cam), cut(ppm), *parts, frame_time=cut(ft), valid=cut(valid)))
        t0 += n
    assert t0 == T
    for k in GAZE_EVENT_KEYS:
        joined = np.concatenate([g[k] for g in got], axis=1)
        assert joined.tobytes() == want[k].tobytes(), k
    for a, b_ in zip(whole, parts):
        assert a.tobytes() == b_.tobytes()
    assert whole[2][0] == 3                               # (the three long fixations, each open across several chunk borders)


def test_reset_flush_and_a_full_store_in_the_reference():
    fps = 120
    pog, o, inv_cam, ppm, valid, _ = scan_path(fps)
    spec = GazeEventSpec(fps=fps)
    state, store, count, dropped = ref.fresh(1, 1)
    ref.run(spec, pog, o, inv_cam, ppm, state, store, count, dropped, valid=valid, flush=np.ones(1, dtype=np.int32))
    assert count[0] == 1 and dropped[0] == 2 and store[0, 0, 0] == 0
    # a reset closes the open fixation, clears the row and leaves the id counter alone
    state, store, count, dropped = ref.fresh(1, 8)
    cut = lambda a: a[:, :30]
    ref.run(spec, cut(pog), cut(o), cut(inv_cam), cut(ppm), state, store, count, dropped)
    assert state[0, ref.FIX_OPEN] == 1 and count[0] == 0 and state[0, ref.TICKS] == 30
    open_row = ref.open_fixation(state[0])
    nxt = state[0, ref.NEXT_ID]
    out = ref.run(spec, cut(pog), cut(o), cut(inv_cam), cut(ppm), state, store, count, dropped, reset=np.ones(1, dtype=np.int32))
    assert count[0] == 1 and np.array_equal(store[0, 0], open_row)
    assert state[0, ref.TICKS] == 30 and out['gaze_event'][0, 0] == 0 and out['fixation_id'][0, 1] == nxt


# ---------------------------------------------------------------------------------------------------------------- the spec
def test_the_spec_compares_by_value_and_refuses_nonsense():
    a, b_ = GazeEventSpec(fps=30), GazeEventSpec(fps=30.0)
    assert a == b_ and hash(a) == hash(b_) and a != GazeEventSpec(fps=60) and a != GazeEventSpec(fps=30, beta=0.01)
    assert a != GazeEventSpec(fps=30, velocity_from='raw') and a != GazeEventSpec(fps=30, source='PoG_px_initial') and a != 30
    assert len({a, b_, GazeEventSpec(fps=30, max_gap_s=0.1)}) == 2 and eve_amd.GazeEventSpec is GazeEventSpec
    d = GazeEventSpec()
    assert (d.source, d.fps, d.min_cutoff_hz, d.beta, d.d_cutoff_hz, d.velocity_from, d.saccade_deg_s, d.min_fixation_s, d.max_gap_s) == \
        (None, None, 1.0, 0.007, 1.0, 'filtered', 30.0, 0.06, 0.075)
    for name in ('fps', 'min_cutoff_hz', 'd_cutoff_hz', 'saccade_deg_s', 'min_fixation_s', 'max_gap_s'):
        for bad in (0, -1.0, float('nan'), float('inf'), '30', True):
            with pytest.raises(ValueError, match=name):
                GazeEventSpec(**{name: bad})
    for bad in (-0.1, float('nan'), float('inf'), None):
        with pytest.raises(ValueError, match='beta'):
            GazeEventSpec(beta=bad)
    assert GazeEventSpec(beta=0).beta == 0.0
    with pytest.raises(ValueError, match='source'):
        GazeEventSpec(source='PoG_cm_final')
    with pytest.raises(ValueError, match='velocity_from'):
        GazeEventSpec(velocity_from='both')


# ---------------------------------------------------------------------------------------------------------------- EVEStream
class EventFakes(MaskFakes):
    """MaskFakes (the ragged and masked steps' stand-ins) plus gaze_events, evaluated by tests/gaze_events_ref.py."""

    def gaze_events(self, pog, origin, inv_cam, ppm, spec, state, store, count, dropped, frame_time=None, valid=None, lengths=None,
                    reset=None, flush=None):
        self.calls.append('gaze_events')
        n = lambda t: None if t is None else t.detach().numpy()
        if pog is None:
            B = state.shape[0]
            ref.run(spec, np.zeros((B, 0, 2)), np.zeros((B, 0, 3)), np.zeros((B, 0, 4, 4)), np.zeros((B, 0, 2)), n(state), n(store), n(count),
                    n(dropped), reset=n(reset), flush=n(flush))
            return {}
        out = ref.run(spec, n(pog), n(origin), n(inv_cam), n(ppm), n(state), n(store), n(count), n(dropped), frame_time=n(frame_time),
                      valid=n(valid), lengths=n(lengths), reset=n(reset), flush=n(flush))
        return {k: torch.from_numpy(v) for k, v in out.items()}


class EventOverlayFakes(EventFakes, OverlayFakes):
    pass


@pytest.fixture()
def fake():
    k = EventOverlayFakes()
    kernels.set_default_kernels(k)
    yield k
    kernels.set_default_kernels(None)
    eve_amd.reset_standalone_config()


B, T = 2, 3
EVERYTHING_FIXATES = dict(fps=30, saccade_deg_s=1e9, min_fixation_s=0.02)     # each stream: one fixation from its second sample on


@pytest.fixture()
def scene(fake):
    model, _ = make_model(dict(refine_net_rnn_type='CGRU'))
    batch = clip(B, 2 * T, size=32)
    return model, chunk_of(batch, 0, T), chunk_of(batch, T, 2 * T)


def run(stream, chunk, **kw):
    return {k: v.clone() for k, v in stream.step(chunk, **kw).items()}


def reference_on(out, chunk, spec, source, state, frame_time=None, valid=None, lengths=None, capacity=256):
    """The reference on the step's own results: the source PoG and the binocular origin (the mean of the usable origins)."""
    o = torch.stack([chunk['left_o'], chunk['right_o']], dim=-1).mean(dim=-1)
    n = lambda t: t.numpy()
    _, store, count, dropped = ref.fresh(B, capacity)
    res = ref.run(spec, n(out[source]), n(o), n(chunk['inv_camera_transformation']), n(chunk['pixels_per_millimeter']), state, store, count,
                  dropped, frame_time=frame_time, valid=valid, lengths=lengths)
    return res, store, count


def test_a_step_with_events_adds_the_seven_keys_and_one_launch(fake, scene):
    model, c0, c1 = scene
    plain = run(eve_amd.EVEStream(model, B, use_graph=False), c0)
    assert 'gaze_events' not in fake.calls and not set(GAZE_EVENT_KEYS) & set(plain)
    calls_plain = list(fake.calls)
    del fake.calls[:]
    s = eve_amd.EVEStream(model, B, use_graph=False)
    spec = GazeEventSpec(fps=30)
    out = run(s, c0, events=spec)
    assert fake.calls == calls_plain + ['gaze_events']                   # the plain step's launches, then one more
    assert sorted(out) == sorted(list(plain) + list(GAZE_EVENT_KEYS))
    for k in plain:
        assert torch.equal(out[k], plain[k]), k
    shapes = {'PoG_px_filtered': ((B, T, 2), torch.float32), 'gaze_velocity': ((B, T), torch.float32), 'gaze_event': ((B, T), torch.uint8),
              'fixation_id': ((B, T), torch.int32), 'fixation_px': ((B, T, 2), torch.float32), 'fixation_ms': ((B, T), torch.float32),
              'fixating': ((B, T), torch.uint8)}
    for k, (shape, dtype) in shapes.items():
        assert tuple(out[k].shape) == shape and out[k].dtype == dtype, k
    # PoG_px_final with a RefineNet; the state carries into the second step
    state = np.zeros((B, 32))
    want, _, _ = reference_on(out, c0, spec, 'PoG_px_final', state)
    for k in GAZE_EVENT_KEYS:
        assert out[k].numpy().tobytes() == want[k].tobytes(), k
    assert torch.isfinite(out['gaze_velocity'][:, 1:]).all() and (out['gaze_event'][:, 1:] != 0).all()
    out1 = run(s, c1, events=spec)
    want1, _, _ = reference_on(out1, c1, spec, 'PoG_px_final', state)
    for k in GAZE_EVENT_KEYS:
        assert out1[k].numpy().tobytes() == want1[k].tobytes(), k
    assert np.array_equal(s.get_event_state().numpy(), state) and state[0, ref.TICKS] == 2 * T
    # a step without events afterwards: the plain step's launches and bits, the events' state untouched
    del fake.calls[:]
    fresh = eve_amd.EVEStream(model, B, use_graph=False)
    run(fresh, c0), run(fresh, c1)
    again = run(fresh, c0)
    del fake.calls[:]
    back = run(s, c0)
    assert 'gaze_events' not in fake.calls and sorted(back) == sorted(again)
    for k in again:
        assert torch.equal(back[k], again[k]), k
    assert np.array_equal(s.get_event_state().numpy(), state)
    # an explicit source, and the chunk's frame_time wins over fps
    s2 = eve_amd.EVEStream(model, B, use_graph=False)
    ft = torch.tensor([[0.0, 0.011, 0.019], [5.0, 5.5, 5.51]], dtype=torch.float64)
    spec2 = GazeEventSpec(source='PoG_px_initial', fps=30)
    out2 = run(s2, dict(c0, frame_time=ft), events=spec2)
    want2, _, _ = reference_on(out2, c0, spec2, 'PoG_px_initial', np.zeros((B, 32)), frame_time=ft.numpy())
    for k in GAZE_EVENT_KEYS:
        assert out2[k].numpy().tobytes() == want2[k].tobytes(), k
    assert torch.isnan(out2['gaze_velocity'][1, 1]) and not torch.isnan(out2['gaze_velocity'][0, 1])     # a 0.5 s gap against 11 ms


def test_events_on_ragged_and_masked_steps(fake, scene):
    model, c0, _ = scene
    spec = GazeEventSpec(fps=30)
    s = eve_amd.EVEStream(model, B, use_graph=False)
    out = run(s, c0, events=spec, lengths=[2, 0])
    want, _, _ = reference_on(out, c0, spec, 'PoG_px_final', np.zeros((B, 32)), lengths=np.array([2, 0]))
    for k in GAZE_EVENT_KEYS:
        assert out[k][0, :2].numpy().tobytes() == want[k][0, :2].tobytes(), k
    assert (out['gaze_event'][1] == 0).all() and s.get_event_state()[:, 0].tolist() == [2.0, 0.0]
    mask = torch.ones(B, T, 2, dtype=torch.bool)
    mask[0, 1] = False                                   # stream 0, frame 1: no usable eye
    mask[1, :, 0] = False                                # stream 1: the right eye alone
    s = eve_amd.EVEStream(model, B, use_graph=False)
    out = run(s, c0, events=spec, eye_mask=mask)
    assert out['valid'].tolist() == [[True, False, True], [True, True, True]]
    o = torch.stack([torch.stack([c0['left_o'], c0['right_o']], dim=-1).mean(dim=-1)[0], c0['right_o'][1]])
    state, store, count, dropped = ref.fresh(B, 256)
    want = ref.run(spec, out['PoG_px_final'].numpy(), o.numpy(), c0['inv_camera_transformation'].numpy(), c0['pixels_per_millimeter'].numpy(),
                   state, store, count, dropped, valid=out['valid'].numpy())
    for k in GAZE_EVENT_KEYS:
        assert out[k].numpy().tobytes() == want[k].tobytes(), k
    assert out['gaze_event'][0].tolist()[1] == 0 and state[0, ref.TICKS] == T      # masked frames are delivered frames: they tick


def test_refusals_come_before_any_launch(fake, scene):
    model, c0, _ = scene
    s = eve_amd.EVEStream(model, B, use_graph=False)
    spec = GazeEventSpec(fps=30)
    without = lambda key: {k: v for k, v in c0.items() if k != key}
    with pytest.raises(ValueError, match='GazeEventSpec'):
        s.step(c0, events=dict(fps=30))
    with pytest.raises(ValueError, match='inv_camera_transformation'):
        s.step(without('inv_camera_transformation'), events=spec)
    with pytest.raises(ValueError, match='pixels_per_millimeter'):
        s.step(without('pixels_per_millimeter'), events=spec)
    with pytest.raises(ValueError, match='frame_time'):
        s.step(c0, events=GazeEventSpec())
    for bad in (torch.zeros(B, T), torch.zeros(B, T + 1, dtype=torch.float64), np.zeros((B, T))):
        with pytest.raises(ValueError, match='frame_time'):
            s.step(dict(c0, frame_time=bad), events=spec)
    with pytest.raises(ValueError, match='fixation_capacity'):
        eve_amd.EVEStream(model, B, use_graph=False, fixation_capacity=0)
    with pytest.raises(ValueError, match='state'):
        s.set_event_state(np.zeros((B, 31)))
    assert fake.calls == []
    eye_only, _ = make_model(dict(refine_net_enabled=False))
    s = eve_amd.EVEStream(eye_only, B, use_graph=False)
    with pytest.raises(ValueError, match='RefineNet'):
        s.step(c0, events=GazeEventSpec(fps=30, source='PoG_px_final'))
    assert fake.calls == []
    out = s.step(without('screen_frame'), events=spec)   # source None without a RefineNet: PoG_px_initial
    want, _, _ = reference_on(out, c0, spec, 'PoG_px_initial', np.zeros((B, 32)))
    assert out['PoG_px_filtered'].numpy().tobytes() == want['PoG_px_filtered'].tobytes() and 'PoG_px_final' not in out


def test_the_graph_key_holds_the_spec_and_frame_time(fake, scene):
    model, c0, _ = scene
    s = eve_amd.EVEStream(model, B, use_graph=False)
    plan = lambda spec, ch=c0: s._check_events(ch, spec, B, T)
    bare = s._graph_key(c0, False)
    a = s._graph_key(c0, False, False, False, None, plan(GazeEventSpec(fps=30)))
    assert a != bare and a == s._graph_key(dict(c0), False, False, False, None, plan(GazeEventSpec(fps=30.0)))
    assert a != s._graph_key(c0, False, False, False, None, plan(GazeEventSpec(fps=30, saccade_deg_s=40)))
    assert a != s._graph_key(c0, False, False, False, None, plan(GazeEventSpec(fps=30, source='PoG_px_initial')))
    timed = dict(c0, frame_time=torch.zeros(B, T, dtype=torch.float64))
    assert a != s._graph_key(timed, False, False, False, None, plan(GazeEventSpec(fps=30), timed))
    captured = []
    s._capture = lambda chunk, *a_, **k_: captured.append(a_) or {'n': len(captured)}
    first = s._graph_for(c0, False, False, False, None, plan(GazeEventSpec(fps=30)))
    assert s._graph_for(c0, False, False, False, None, plan(GazeEventSpec(fps=30))) is first and len(captured) == 1
    assert s._graph_for(c0, False) is not first and len(captured) == 2 and len(captured[1]) == 4      # (no events: _capture's old call)


def test_reset_closes_and_clears_and_fixations_reads_the_store(fake, scene):
    model, c0, c1 = scene
    spec = GazeEventSpec(**EVERYTHING_FIXATES)
    s = eve_amd.EVEStream(model, B, use_graph=False, fixation_capacity=4)
    assert [f.shape for f in s.fixations()] == [(0, 8)] * B
    out = run(s, c0, events=spec)
    assert out['gaze_event'].tolist() == [[0, 1, 1]] * B and out['fixation_id'].tolist() == [[-1, 0, 0]] * B
    assert out['fixating'].tolist() == [[0, 0, 1]] * B                  # 0 and 33 ms against 20
    assert np.allclose(out['fixation_ms'].numpy(), [[0, 0, 1000 / 30.0]] * B)
    state = s.get_event_state().numpy()
    assert [f.shape for f in s.fixations()] == [(0, 8)] * B and s.fixation_counts()[0].tolist() == [0, 0]
    opened = s.fixations(include_open=True)
    for b in range(B):
        assert np.array_equal(opened[b], ref.open_fixation(state[b])[None])
        assert opened[b][0, 3] == 2 and opened[b][0, 1] == 1 / 30.0 and opened[b][0, 2] == 2 / 30.0
    assert len(s.fixations([1], include_open=True)) == 1
    s.reset([1])
    out = run(s, c1, events=spec)
    count, dropped = s.fixation_counts()
    assert count.tolist() == [0, 1] and dropped.tolist() == [0, 0]
    assert np.array_equal(s.fixations()[1], opened[1])                   # closed as it stood
    assert out['gaze_event'].tolist() == [[1, 1, 1], [0, 1, 1]] and out['fixation_id'].tolist() == [[0, 0, 0], [-1, 1, 1]]
    after = s.get_event_state().numpy()
    assert after[:, ref.TICKS].tolist() == [2 * T, T] and after[:, ref.NEXT_ID].tolist() == [1, 2]
    # a reset before a step WITHOUT events still reaches the events' state: one launch with no frames, and the plain step
    s.reset([0])
    del fake.calls[:]
    run(s, c0)
    assert fake.calls.count('gaze_events') == 1 and fake.calls[0] == 'gaze_events'
    assert s.fixation_counts()[0].tolist() == [1, 1] and s.get_event_state()[0, ref.TICKS] == 0
    assert s.fixations()[0][0, 3] == 5 and s.get_event_state()[1, ref.FIX_OPEN] == 1
    s.flush_fixations([1])
    assert s.fixation_counts()[0].tolist() == [1, 2] and s.get_event_state()[1, ref.FIX_OPEN] == 0
    s.clear_fixations([1])
    assert s.fixation_counts()[0].tolist() == [1, 0]
    # set_event_state round-trips, get_state() does not hold the row
    saved = s.get_event_state()
    s.set_event_state(torch.zeros(B, 32))
    assert not s.get_event_state().any()
    s.set_event_state(saved)
    assert torch.equal(s.get_event_state(), saved) and not any('event' in k for k in s.get_state())


def test_overlay_markers_may_name_the_event_keys_only_with_events(fake):
    from test_stream_ragged_host import CONFIGS, make_model as ragged_model
    model = ragged_model(*CONFIGS['gru-cgru'])
    Bc, Tc = 2, 2
    ch = stream_chunk(Bc, Tc)
    s = eve_amd.EVEStream(model, Bc, use_graph=False)
    overlay = OverlaySpec(markers=[dict(key='fixation_px', valid='fixating', r_fill=3, r_outline=5), dict(key='PoG_px_filtered', r_fill=2, r_outline=3)],
                          inset=None, out_format='rgb')
    with pytest.raises(ValueError, match='fixation_px'):
        s.step(ch, render=overlay)
    assert fake.calls == []
    spec = GazeEventSpec(**EVERYTHING_FIXATES)
    out = s.step(ch, render=overlay, events=spec)
    assert fake.calls[-2:] == ['gaze_events', 'overlay_render'] and 'rendered' in out
    # the launch got the step's own fixation_px, gated by fixating
    import overlay_ref as oref
    cap = ch['screen_frame_nv12']
    N = Bc * Tc
    IH, IW = cap.shape[2] * 2 // 3, cap.shape[3]
    markers = dict(centres=np.stack([out['fixation_px'].reshape(N, 2).numpy(), out['PoG_px_filtered'].reshape(N, 2).numpy()], axis=1),
                   table=np.array(overlay.marker_table(), dtype=np.int32).reshape(-1, 4),
                   valid=np.stack([out['fixating'].reshape(N).numpy(), np.ones(N, dtype=np.uint8)], axis=1),
                   sx=np.float32(IW / 1920.0), sy=np.float32(IH / 1080.0))
    want = oref.render(cap.reshape((N,) + tuple(cap.shape[2:])).numpy(), 'nv12', 'rgb', 'bt601', markers, None, None, None)
    assert np.array_equal(out['rendered'].reshape(want.shape).numpy(), want)
