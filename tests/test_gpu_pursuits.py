"""GPU: eve_gaze_pursuits against the numpy contract of tests/pursuit_ref.py, and EVEStream's step(events=..., pursuits=...) around it
(eager and captured).  Every test here needs the new entry point, PursuitSpec or the pursuits argument, so every one fails without
them.

What must be equal.  The kernel is fed the REFERENCE's events arrays (saccade_ref.events_ex), so everything that does not pass through
an atan2 is bit for bit: gaze_class, pursuit_id, pursuit_ms, pursuit_gain (+ - * / only), the state row but its peak entry -- the ring
with its running path length included --, the counters, and every store and table column of times, points, counts, gain and error
(whose sqrt is correctly rounded on both sides).  The window angle's descendants -- gaze_velocity_windowed and gaze_straightness after
their float32 rounding: the same or the adjacent float32; the state's and the rows' peak -- and the closings' amplitude, direction,
mean velocity and path: within 1e-12 * max(1, |reference|), the bound of a double sqrt / atan2 chain (test_gpu_calibration.py,
test_gpu_saccades.py); a table column that sums k such terms within 2 k times that bound.  Labels depend on thresholded atan2 values,
so each comparison first asserts ON THE REFERENCE ALONE that thresholds_clear holds: no frame's windowed velocity or straightness and
no closing's amplitude within 1e-9 (relative) of its threshold.  No frame is exempt from the comparison."""
import numpy as np
import pytest
import torch

import eve_amd
import gaze_events_ref as eref
import pursuit_ref as ref
import saccade_ref as sref
from eve_amd import data
from eve_amd.data import GAZE_EVENT_KEYS, PURSUIT_KEYS, SACCADE_KEYS, GazeEventSpec, PursuitSpec, SaccadeSpec
from eve_amd.eve import _mean2
from eve_amd.kernels import default_kernels
from test_gpu_calibration import cuda, guarded, guards_hold
from test_gpu_gaze_events import same_or_adjacent_float32
from test_gpu_stream import gpu_clip, make_model
from test_pursuits_host import FLICKER, geometry, path, ramp

pytestmark = pytest.mark.gpu
FPS = 120
FILTERED = GazeEventSpec(fps=FPS)
# windows of 12 frames that decide from 6 on, so that 70 frames hold closings of every kind
SHORT_WINDOWS = PursuitSpec(window_s=0.1, min_window_s=0.05, settle_s=0.03, min_duration_s=0.05, min_amplitude_deg=0.5, max_missing=1)
BOUND = 1e-12
EXACT_OUT = ('gaze_class', 'pursuit_id', 'pursuit_ms', 'pursuit_gain')
ROUNDED_OUT = ('gaze_velocity_windowed', 'gaze_straightness')
OUT_DTYPES = (torch.uint8, torch.int32, torch.float32, torch.float32, torch.float32, torch.float32)


def close(got, want, k=1):
    both_nan = np.isnan(got) & np.isnan(want)
    return bool((both_nan | (np.abs(got - want) <= k * BOUND * np.maximum(1.0, np.abs(want)))).all())


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=got.dtype.kind == 'f')


# ---------------------------------------------------------------------------------------------------------------- the clip
def the_clip(fps=FPS, T=80):
    """B = 3, T = 80 (the one-pass test takes the first 70: across the 64-frame pass).
    stream 0: 8 frames at rest, then 8 degrees / second to the end: one episode, open across the pass boundary and at the end; its
              target has no position in frames 30 .. 39;
    stream 1: 10 degrees / second with a 10 degree jump at frame 30 (the episode before it closes and is stored; the settling samples
              stay out), frames 55 and 56 invalid inside the second episode (2 > max_missing: interrupted when it ends), at rest from
              frame 64 on;
    stream 2: stop and go at 15 degrees / second, 30 degrees off the x axis; no target (NaN)."""
    fr = lambda n: n / float(fps)
    a, ta = path(fps, [(fr(8), 0.0), (fr(T), 8.0)])
    b_, tb = path(fps, [(fr(30), 10.0), (fr(1), 10.0 * fps), (fr(33), 10.0), (fr(T), 0.0)], seed=6)
    c, tc = path(fps, [(fr(14), 15.0), (fr(16), 0.0), (fr(14), 15.0), (fr(T), 0.0)], angle_deg=30.0, seed=7)
    pog, target = np.concatenate([a[:, :T], b_[:, :T], c[:, :T]]), np.concatenate([ta[:, :T], tb[:, :T], tc[:, :T]])
    target[0, 30:40] = np.nan
    target[2] = np.nan
    valid = np.ones((3, T), dtype=np.uint8)
    valid[1, 55:57] = 0
    return (pog,) + geometry(T, 3) + (valid, target)


def reference(spec, pspec, inputs, T=None, lengths=None, capacity=4, target=True):
    """The reference's events and pursuit of the first T frames in one pass from fresh state, its thresholds asserted clear."""
    pog, o, inv_cam, ppm, valid, tgt = [a[:, :T] for a in inputs]
    elog, log = eref.new_log(), ref.new_log()
    ex = sref.events_ex(spec, pog, o, inv_cam, ppm, *eref.fresh(pog.shape[0], 8), valid=valid, lengths=lengths, log=elog)
    carried = ref.fresh(pog.shape[0], capacity)
    frames = frame_inputs(spec, ex, pog)
    out = ref.run(pspec, *frames, *carried, target=tgt if target is True else target, lengths=lengths, log=log)
    assert eref.thresholds_clear(spec, elog) and ref.thresholds_clear(pspec, log, margin=1e-9) and log['velocities']
    return dict(ex=ex, frames=frames, out=out, carried=carried, target=tgt, lengths=lengths)


def frame_inputs(spec, ex, pog):
    return [ex['sample'], ex['sample_time'], ex['gaze_vector'], np.nan_to_num(sref.point_of(spec, pog, ex)), ex['gaze_event'], ex['gaze_velocity'],
            ex['fixation_id']]


@pytest.fixture(scope='module')
def clip():
    """The clip and the reference on its first 70 frames and on all 80: computed once, shared, never modified."""
    inputs = the_clip()
    lengths = np.array([70, 70, 40], dtype=np.int32)
    seventy = reference(FILTERED, SHORT_WINDOWS, inputs, T=70, lengths=lengths)
    eighty = reference(FILTERED, SHORT_WINDOWS, inputs)
    state, table, store, count, dropped = seventy['carried']
    out = seventy['out']
    assert state[0, ref.OPEN] == 1 and (out['pursuit_id'][0, 56:70] == 0).all() and state[0, ref.RING_N] == 32      # open across the pass
    assert table[1, ref.ACCEPTED] == 1 and count[1] == 1 and (out['gaze_class'][1] == 2).any() and (out['gaze_class'][1, 60:68] == 3).any()
    assert not out['gaze_class'][2, 40:].any() and np.isnan(out['gaze_velocity_windowed'][2, 40:]).all() and state[2, ref.OPEN] == 1
    assert np.isfinite(out['pursuit_gain'][0, 20:30]).all() and np.isnan(out['pursuit_gain'][0, 30:40]).all() and np.isnan(out['pursuit_gain'][2]).all()
    assert eighty['carried'][1][1, ref.INTERRUPTED] == 1 and eighty['carried'][1][:, ref.ACCEPTED].tolist() == [0, 1, 1]
    return dict(inputs=inputs, seventy=seventy, eighty=eighty)


def device_buffers(B, capacity):
    """The five carried buffers of fresh streams between guards -> ((whole, sentinel) pairs, buffers)."""
    SENT = -777.25
    shapes = [((B, 320), torch.float64, SENT), ((B, 16), torch.float64, SENT), ((B, capacity, 20), torch.float64, SENT), ((B,), torch.int32, -7),
              ((B,), torch.int32, -7)]
    pairs = [guarded(shape, dtype, sentinel) for shape, dtype, sentinel in shapes]
    for _, payload in pairs:
        payload.zero_()
    return [(whole, s_[2]) for (whole, _), s_ in zip(pairs, shapes)], [payload for _, payload in pairs]


def assert_outputs(got, want, where=None):
    """got: the device's six per-frame results (tensors); want: the reference's."""
    sel = (lambda a: a) if where is None else (lambda a: a[where])
    for k_ in EXACT_OUT:
        assert same(sel(got[k_].cpu().numpy()), sel(want[k_])), k_
    for k_ in ROUNDED_OUT:
        g = got[k_].cpu().numpy()
        assert g.dtype == np.float32 and same_or_adjacent_float32(np.ascontiguousarray(sel(g)), np.ascontiguousarray(sel(want[k_]))), k_


def assert_carried(got, want, state=True):
    """got: the five device buffers; want: the reference's."""
    g_state, table, store, count, dropped = (t.cpu().numpy() for t in got)
    w_state, w_table, w_store, w_count, w_dropped = want
    assert count.tolist() == w_count.tolist() and dropped.tolist() == w_dropped.tolist()
    if state:
        cols = [c for c in range(ref.STATE_DOUBLES) if c != ref.PEAK]
        assert same(g_state[:, cols], w_state[:, cols])
        assert close(g_state[:, ref.PEAK], w_state[:, ref.PEAK])
    cols = [c for c in range(ref.ROW) if c not in ref.TRANSCENDENTAL_ROW]
    assert same(store[:, :, cols], w_store[:, :, cols])
    for c in ref.TRANSCENDENTAL_ROW:
        assert close(store[:, :, c], w_store[:, :, c]), c
    cols = [c for c in range(ref.TABLE_ROW) if c not in ref.TRANSCENDENTAL_TABLE]
    assert same(table[:, cols], w_table[:, cols])
    k = np.maximum(w_table[:, ref.ACCEPTED], 1.0)
    for c in ref.TRANSCENDENTAL_TABLE:
        assert (np.abs(table[:, c] - w_table[:, c]) <= 2 * k * BOUND * np.maximum(1.0, np.abs(w_table[:, c]))).all(), c


# ---------------------------------------------------------------------------------------------------------------- eve_gaze_pursuits
def pursuits_call(pspec, frames, target, carried, outs, lengths=None, reset=None, T=None, B=None, S=None):
    """The C entry point itself.  frames: the seven frame inputs (device tensors) or Nones; -> its status."""
    k = default_kernels()
    state, table, store, count, dropped = carried
    p = k._p
    T = frames[0].shape[1] if T is None else T
    B = (state.shape[0] if state is not None else 1) if B is None else B
    S = (store.shape[1] if store is not None else 1) if S is None else S
    return k.lib.eve_gaze_pursuits(B, T, *[p(a) for a in frames], p(target), p(lengths), p(reset), pspec.window_s, pspec.min_window_s,
                                   pspec.pursuit_deg_s, pspec.min_straightness, pspec.settle_s, pspec.min_duration_s, pspec.min_amplitude_deg,
                                   pspec.max_missing, p(state), p(table), S, p(store), p(count), p(dropped), *[p(a) for a in outs], k._stream())


def test_seventy_frames_across_the_pass_between_guards(clip):
    want = clip['seventy']
    B, T = want['frames'][0].shape
    frames = [cuda(a) for a in want['frames']]
    wholes, carried = device_buffers(B, 4)
    guarded_outs = [guarded((B, T), dtype, 99 if dtype in (torch.uint8, torch.int32) else -777.25) for dtype in OUT_DTYPES]
    outs = [payload for _, payload in guarded_outs]
    assert pursuits_call(SHORT_WINDOWS, frames, cuda(want['target']), carried, outs, cuda(want['lengths'])) == 0
    torch.cuda.synchronize()
    assert default_kernels().lib.eve_last_kernel().decode() == 'gaze_pursuits_kernel'
    assert_outputs(dict(zip(PURSUIT_KEYS, outs)), want['out'])
    assert_carried(carried, want['carried'])
    assert all(guards_hold(w, 99 if w.dtype in (torch.uint8, torch.int32) else -777.25) for w, _ in guarded_outs)
    assert all(guards_hold(w, s_) for w, s_ in wholes)


def device_run(pspec, want, sizes, capacity=4, resets=None, target=True):
    """A reference's arrays through the wrapper in chunks of `sizes` -> (outputs joined, the five buffers)."""
    arrays = want['frames'] + ([want['target']] if target else [])
    B, T = arrays[0].shape
    lengths = want['lengths'] if want['lengths'] is not None else np.full(B, T, dtype=np.int32)
    k = default_kernels()
    carried = data.pursuit_buffers(B, capacity, 'cuda')
    parts, t0 = [], 0
    for i, n in enumerate(sizes):
        cut = [cuda(a[:, t0:t0 + n]) for a in arrays]
        parts.append(k.gaze_pursuits(*cut[:7], pspec, *carried, target=cut[7] if target else None,
                                     lengths=cuda(np.clip(lengths - t0, 0, n).astype(np.int32)),
                                     reset=None if resets is None else cuda(np.asarray(resets[i], dtype=np.int32))))
        t0 += n
    assert t0 == T
    return {k_: torch.cat([p[k_] for p in parts], dim=1) for k_ in PURSUIT_KEYS}, carried


def test_chunks_of_two_over_eighty_frames_carry_the_ring_and_the_episode(clip):
    want = clip['eighty']
    whole = device_run(SHORT_WINDOWS, want, [80])
    assert_outputs(whole[0], want['out'])
    assert_carried(whole[1], want['carried'])
    for sizes in ([2] * 40, [64, 16], [63, 1, 16]):
        split = device_run(SHORT_WINDOWS, want, sizes)
        for k_ in PURSUIT_KEYS:
            assert same(split[0][k_].cpu().numpy(), whole[0][k_].cpu().numpy()), (sizes[0], k_)
        for a, b_ in zip(whole[1], split[1]):
            assert same(a.cpu().numpy(), b_.cpu().numpy()), sizes[0]      # exactly, in every column: the atan2 is the device's in both


def test_one_frame_no_frames_with_reset_flags_and_ragged_lengths(clip):
    want80 = clip['eighty']
    arrays = want80['frames'] + [want80['target']]
    k = default_kernels()
    pspec = SHORT_WINDOWS
    # 64 frames, then T = 1, then T = 0 with reset flags (streams 0 and 2 in mid-episode), then 5 frames with lengths (0, 1, 5), then
    # the rest with a reset of stream 1 (in mid-episode too) -- against the reference walked the same way
    want, got = ref.fresh(3, 1), data.pursuit_buffers(3, 1, 'cuda')
    steps = [(0, 64, None, None), (64, 65, None, None), (65, 65, [1, 0, 1], None), (65, 70, None, [0, 1, 5]), (70, 80, [0, 1, 0], None)]
    log = ref.new_log()
    for t0, t1, reset, lengths in steps:
        n = t1 - t0
        rs = None if reset is None else np.asarray(reset, dtype=np.int32)
        ln = None if lengths is None else np.asarray(lengths, dtype=np.int32)
        if n:
            w = ref.run(pspec, *[a[:, t0:t1] for a in arrays[:7]], *want, target=arrays[7][:, t0:t1], lengths=ln, reset=rs, log=log)
            cut = [cuda(a[:, t0:t1]) for a in arrays]
            g = k.gaze_pursuits(*cut[:7], pspec, *got, target=cut[7], lengths=None if ln is None else cuda(ln), reset=None if rs is None else cuda(rs))
            assert_outputs(g, w)
        else:
            before = [a.copy() for a in want]
            ref.run(pspec, None, None, None, None, None, None, None, *want, reset=rs)
            assert k.gaze_pursuits(None, None, None, None, None, None, None, pspec, *got, reset=cuda(rs)) == {}
            assert before[0][0, ref.OPEN] == 1 and want[1][0, ref.ABORTED] == before[1][0, ref.ABORTED] + 1 and want[0][0, ref.NEXT_ID] == before[0][0, ref.NEXT_ID]
            assert not np.delete(want[0][0], ref.NEXT_ID).any() and same(want[0][1], before[0][1])
        assert_carried(got, want)
    assert ref.thresholds_clear(pspec, log, margin=1e-9)
    assert want[1][:, ref.ABORTED].tolist() == [1, 1, 0] and want[3].tolist() == [0, 1, 1]


def test_flickering_episodes_on_the_device_never_overlap():
    """The host suite's ramp under a threshold inside the windowed velocity's jitter: seven short episodes, each one's onset clamped to
    the sample after the one before, over four passes; default windows (24 samples); the same ramp at 150 degrees beside it."""
    (a, ta), (b_, tb) = ramp(FPS, 8.0), ramp(FPS, 8.0, 150.0)
    pog, target = np.concatenate([a, b_]), np.concatenate([ta, tb])
    T = pog.shape[1]
    want = reference(FILTERED, FLICKER, (pog,) + geometry(T, 2) + (np.ones((2, T), dtype=np.uint8), target), capacity=1)
    state, table, store, count, dropped = want['carried']
    assert table[:, ref.ACCEPTED].tolist() == [7, 4] and count.tolist() == [1, 1] and dropped.tolist() == [6, 3] and T > 192      # a store of one row
    got, carried = device_run(FLICKER, want, [pog.shape[1]], capacity=1)
    assert_outputs(got, want['out'])
    assert_carried(carried, want['carried'])


def test_the_ring_caps_a_window_at_thirty_two_samples():
    """240 fps and window_s = 0.2: 48 samples would fit the window, the ring holds 32, so every window is 31 steps long."""
    spec, pspec = GazeEventSpec(fps=240), PursuitSpec()
    a, ta = path(240, [(10 / 240.0, 0.0), (1.0, 8.0)])
    b_, tb = path(240, [(1.0, 15.0)], angle_deg=90.0, seed=8)
    T = 70
    inputs = (np.concatenate([a[:, :T], b_[:, :T]]),) + geometry(T, 2) + (np.ones((2, T), dtype=np.uint8), np.concatenate([ta[:, :T], tb[:, :T]]))
    want = reference(spec, pspec, inputs)
    w = want['out']['gaze_velocity_windowed']
    assert np.isnan(w[:, :24]).all() and np.isfinite(w[:, 24:]).all() and (want['out']['gaze_class'][1, 40:] == 3).all()
    assert (want['carried'][0][:, ref.RING_N] == 32).all() and (want['carried'][0][:, ref.OPEN] == 1).all()
    # (a window of 31 steps of 1 / 240 s: 0.129 s, not 0.2 -- the onset of stream 1's episode, whose first frame is 24, is frame 0)
    assert want['carried'][0][1, ref.T_ONSET] == 0.0 and want['out']['pursuit_ms'][1, 69] == np.float32(1000.0 * 69 / 240.0)
    got, carried = device_run(pspec, want, [70])
    assert_outputs(got, want['out'])
    assert_carried(carried, want['carried'])
    got, carried = device_run(pspec, want, [33, 33, 4])
    assert_outputs(got, want['out'])
    assert_carried(carried, want['carried'])


@pytest.mark.parametrize('velocity_from', ['filtered', 'raw'])
def test_targets_absent_and_nan_a_silent_stream_and_either_velocity(clip, velocity_from):
    """target NULL and all NaN; a stream whose every frame is a non-sample; both velocity_from settings (for raw only reference ==
    kernel is claimed)."""
    pog, o, inv_cam, ppm, valid, target = [a[:, :70].copy() for a in clip['inputs']]
    valid[2] = 0
    inputs = (pog, o, inv_cam, ppm, valid, target)
    spec = GazeEventSpec(fps=FPS, velocity_from=velocity_from)
    for tgt in (None, np.full_like(target, np.nan)):
        want = reference(spec, SHORT_WINDOWS, inputs, target=tgt)
        assert not want['ex']['sample'][2].any() and not want['out']['gaze_class'][2].any() and not want['carried'][0][2].any()
        assert np.isnan(want['out']['pursuit_gain']).all() and (want['carried'][1][:, ref.TAB_GAIN_N] == 0).all()
        want['target'] = tgt
        got, carried = device_run(SHORT_WINDOWS, want, [70], target=tgt is not None)
        assert_outputs(got, want['out'])
        assert_carried(carried, want['carried'])


def test_the_library_refuses_without_a_launch(clip):
    k = default_kernels()
    want = clip['seventy']
    frames = [cuda(a[:, :2]) for a in want['frames']]
    carried = list(data.pursuit_buffers(3, 2, 'cuda'))
    outs = [torch.zeros((3, 2), dtype=dtype, device='cuda') for dtype in OUT_DTYPES]
    k.gaze_events(None, None, None, None, FILTERED, torch.zeros((1, 32), dtype=torch.float64, device='cuda'),
                  torch.zeros((1, 1, 8), dtype=torch.float64, device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda'),
                  torch.zeros(1, dtype=torch.int32, device='cuda'))
    before = k.lib.eve_last_kernel()
    assert before == b'gaze_events_kernel'

    class Bad(object):
        def __init__(self, **kw):
            self.__dict__.update(dict(PursuitSpec().__dict__, **kw))

    def refused(status, *words):
        msg = k.lib.eve_last_error().decode()
        assert status != 0 and msg.startswith('gaze_pursuits:') and all(w in msg for w in words), msg
        assert k.lib.eve_last_kernel() == before

    ok = PursuitSpec()
    for i in range(5):
        refused(pursuits_call(ok, frames, None, carried[:i] + [None] + carried[i + 1:], outs, B=3, S=2), 'null carried buffer')
    for i in range(7):
        refused(pursuits_call(ok, frames[:i] + [None] + frames[i + 1:], None, carried, outs, T=2), 'null frame input or output')
    for i in range(6):
        refused(pursuits_call(ok, frames, None, carried, outs[:i] + [None] + outs[i + 1:]), 'null frame input or output')
    refused(pursuits_call(ok, frames, None, carried, outs, T=-1), 'T >= 0')
    refused(pursuits_call(ok, frames, None, carried, outs, B=0), 'B >= 1')
    refused(pursuits_call(ok, frames, None, carried, outs, S=0), 'S >= 1')
    refused(pursuits_call(ok, [None] * 7, None, carried, [None] * 6, T=0, B=1 << 23), '320', '31 bits')
    refused(pursuits_call(ok, [None] * 7, None, carried, [None] * 6, T=0, B=1 << 20, S=1 << 10), 'S * 20', '31 bits')
    refused(pursuits_call(ok, frames, None, carried, outs, T=1 << 10, B=1 << 20), 'T * 3', '31 bits')
    names = ('window_s', 'min_window_s', 'pursuit_deg_s', 'min_straightness', 'settle_s', 'min_duration_s', 'min_amplitude_deg')
    for name in names:
        for bad in (float('nan'), float('inf'), -float('inf')):
            refused(pursuits_call(Bad(**{name: bad}), frames, None, carried, outs), 'finite')
    for name, bad in (('window_s', 0.0), ('min_window_s', 0.0), ('min_window_s', 0.3), ('pursuit_deg_s', 0.0), ('min_straightness', 0.0),
                      ('min_straightness', 1.5), ('settle_s', -1e-9), ('min_duration_s', -1e-9), ('min_amplitude_deg', -0.1), ('max_missing', -1)):
        refused(pursuits_call(Bad(**{name: bad}), frames, None, carried, outs), name)
    # the wrapper's own type and shape checks
    with pytest.raises(TypeError, match='state'):
        k.gaze_pursuits(*frames, ok, carried[0][:, :32].contiguous(), *carried[1:])
    with pytest.raises(TypeError, match='store'):
        k.gaze_pursuits(*frames, ok, carried[0], carried[1], carried[2][:, :, :16].contiguous(), *carried[3:])
    with pytest.raises(TypeError, match='target'):
        k.gaze_pursuits(*frames, ok, *carried, target=torch.zeros((3, 2, 2), dtype=torch.float64, device='cuda'))
    with pytest.raises(TypeError, match='gaze_vector'):
        k.gaze_pursuits(frames[0], frames[1], frames[2].float(), *frames[3:], ok, *carried)
    with pytest.raises(TypeError, match='no frame inputs'):
        k.gaze_pursuits(None, frames[1], None, None, None, None, None, ok, *carried)
    torch.cuda.synchronize()
    assert k.lib.eve_last_kernel() == before and not any(t.any() for t in carried) and not any(t.any() for t in outs)


# ---------------------------------------------------------------------------------------------------------------- EVEStream
S, TC = 3, 5
EVENTS = GazeEventSpec(fps=30, saccade_deg_s=1e9)          # every chained frame is a fixation frame
# ... and every one with a window (two samples do) is a candidate; nothing is near a threshold
ALWAYS = PursuitSpec(window_s=0.1, min_window_s=0.03, pursuit_deg_s=1e-9, min_straightness=1e-9, settle_s=0.0, min_duration_s=0.0,
                     min_amplitude_deg=0.0)
SACCADES = SaccadeSpec(min_amplitude_deg=0.0, max_duration_s=10.0)


@pytest.fixture(scope='module')
def rig():
    """One model and one 3 x 10 clip with a pursuit target: shared and never modified."""
    model, _ = make_model(refine_net_rnn_type='CGRU')
    _, d, _ = gpu_clip(S, 2 * TC, seed=7)
    d = dict(d)
    rng = np.random.RandomState(3)
    target = (np.array([900.0, 500.0]) + np.cumsum(rng.uniform(5.0, 25.0, (S, 2 * TC, 2)), axis=1)).astype(np.float32)
    target[1, 3] = np.nan
    d['pursuit_target'] = cuda(target)
    chunk = lambda t0, t1: {k: v[:, t0:t1].contiguous() for k, v in d.items()}
    return {'model': model, 'chunks': (chunk(0, TC), chunk(TC, 2 * TC))}


def keep_out(out):
    return {k: v.clone() for k, v in out.items()}


def test_stream_pursuits_eager_captured_stand_alone_and_the_reference(rig):
    model, chunks = rig['model'], rig['chunks']
    eager_stream, graph_stream, bare_stream = eve_amd.EVEStream(model, S, use_graph=False), eve_amd.EVEStream(model, S), eve_amd.EVEStream(model, S, use_graph=False)
    step = lambda s_, i, **kw: keep_out(s_.step(chunks[i], events=EVENTS, saccades=SACCADES, **kw))
    eager = [step(eager_stream, i, pursuits=ALWAYS) for i in range(2)]
    graph = [step(graph_stream, i, pursuits=ALWAYS) for i in range(2)]
    bare = [step(bare_stream, i) for i in range(2)]
    assert len(graph_stream._graphs) == 1 and bare_stream._pursuits is None      # the second step replayed the first one's graph
    for e, g, b_ in zip(eager, graph, bare):
        assert sorted(e) == sorted(g) == sorted(list(b_) + list(PURSUIT_KEYS)) and set(SACCADE_KEYS) <= set(b_)
        for k_ in e:                                       # a graph replay equals eager
            assert same(e[k_].cpu().numpy(), g[k_].cpu().numpy()), k_
        for k_ in b_:                                      # a step without pursuits= keeps its bits in every key it had
            assert same(e[k_].cpu().numpy(), b_[k_].cpu().numpy()), k_
    for a, b_ in zip(eager_stream._pursuit_buffers(), graph_stream._pursuit_buffers()):      # (the capture's warm-up steps moved nothing)
        assert same(a.cpu().numpy(), b_.cpu().numpy())
    # the stand-alone entry on the same points: the same launches from fresh state, so the same bits
    cat = lambda key: torch.cat([c[key] for c in chunks], dim=1)
    pog = torch.cat([e['PoG_px_final'] for e in eager], dim=1)
    o = _mean2(cat('left_o'), cat('right_o')).float()
    alone = data.gaze_pursuits(pog, o, cat('inv_camera_transformation').float(), cat('pixels_per_millimeter').float(), EVENTS, ALWAYS,
                               target=cat('pursuit_target'), pursuit_capacity=eager_stream.pursuit_capacity)
    for k_ in PURSUIT_KEYS + GAZE_EVENT_KEYS:
        assert same(alone[k_].cpu().numpy(), torch.cat([e[k_] for e in eager], dim=1).cpu().numpy()), k_
    state, table, store, count, dropped = eager_stream._pursuit_buffers()
    for a, b_ in ((alone['pursuit_table'], table), (alone['pursuits'], store), (alone['pursuit_count'], count), (alone['pursuit_dropped'], dropped)):
        assert same(a.cpu().numpy(), b_.cpu().numpy())
    # ... and the reference on them
    elog, log = eref.new_log(), ref.new_log()
    n = lambda t: t.float().cpu().numpy()
    ex = sref.events_ex(EVENTS, n(pog), n(o), n(cat('inv_camera_transformation')), n(cat('pixels_per_millimeter')), *eref.fresh(S, 8), log=elog)
    want_carried = ref.fresh(S, eager_stream.pursuit_capacity)
    want = ref.run(ALWAYS, *frame_inputs(EVENTS, ex, n(pog)), *want_carried, target=n(cat('pursuit_target')), log=log)
    assert eref.thresholds_clear(EVENTS, elog) and ref.thresholds_clear(ALWAYS, log, margin=1e-9)
    assert (want['gaze_class'][:, 1:] == 3).all() and (want_carried[0][:, ref.OPEN] == 1).all()
    # (stream 1's target is missing in frame 3: no gain there, nor in frame 6, whose window of three steps starts there)
    assert np.isnan(want['pursuit_gain'][1, [3, 6]]).all() and np.isfinite(want['pursuit_gain'][1, [4, 5, 7]]).all()
    assert np.isfinite(want['pursuit_gain'][0, 1:]).all()
    for k_ in ('gaze_class', 'pursuit_id', 'pursuit_ms'):
        assert same(alone[k_].cpu().numpy(), want[k_]), k_
    assert same(eager_stream.get_pursuit_state()[:, [ref.OPEN, ref.ID, ref.NEXT_ID, ref.N, ref.RING_N, ref.GAIN_N]].cpu().numpy(),
                want_carried[0][:, [ref.OPEN, ref.ID, ref.NEXT_ID, ref.N, ref.RING_N, ref.GAIN_N]])
    # reset() in mid-episode: aborted inside the captured step, the ids run on
    graph_stream.reset([1])
    third = graph_stream.step(chunks[0], events=EVENTS, saccades=SACCADES, pursuits=ALWAYS)
    assert third['pursuit_id'].tolist() == [[0] * 5, [-1, 1, 1, 1, 1], [0] * 5] and graph_stream.pursuit_table()[:, ref.ABORTED].tolist() == [0, 1, 0]
    with pytest.raises(ValueError, match='events='):
        graph_stream.step(chunks[0], pursuits=ALWAYS)
