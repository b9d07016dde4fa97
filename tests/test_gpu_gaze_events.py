"""GPU: eve_gaze_events against the numpy contract of tests/gaze_events_ref.py, and EVEStream's step(events=...) around it (eager
and captured).  Every test here needs the entry point, GazeEventSpec or the events argument, so every one fails without them.

What must be equal, in every comparison with the reference: PoG_px_filtered, fixation_px, fixation_ms, fixating, gaze_event,
fixation_id, the state rows, the store rows except rms_px and the counters, bit for bit (nothing but + - * / fabs and comparisons
leads to them); gaze_velocity and rms_px within 1e-12 * max(1, |reference|) in float64 terms (a double sqrt / atan2 chain, the bound
of test_gpu_calibration.py) -- for the float32 velocity output that is the same or an adjacent float32.  Exact labels are fair only
away from the thresholds, so each comparison first asserts ON THE REFERENCE ALONE that no velocity, sample interval or closing
duration is within 1e-9 (relative) of its threshold."""
import numpy as np
import pytest
import torch

import eve_amd
import gaze_events_ref as ref
import overlay_ref as oref
from eve_amd import data
from eve_amd.data import GAZE_EVENT_KEYS, GazeEventSpec, OverlaySpec
from eve_amd.eve import _fuse2, _mean2
from eve_amd.kernels import default_kernels
from test_gpu_calibration import cuda, guarded, guards_hold
from test_gpu_overlay import CAPTURE, nv12_capture
from test_gpu_stream import gpu_clip, make_model

pytestmark = pytest.mark.gpu
EXACT = ('PoG_px_filtered', 'fixation_px', 'fixation_ms', 'fixating', 'gaze_event', 'fixation_id')
OUT_DTYPES = {'PoG_px_filtered': (torch.float32, 2), 'gaze_velocity': (torch.float32, 1), 'gaze_event': (torch.uint8, 1),
              'fixation_id': (torch.int32, 1), 'fixation_px': (torch.float32, 2), 'fixation_ms': (torch.float32, 1), 'fixating': (torch.uint8, 1)}
PPM = 3.6
INV_CAM = np.array([[1.0, 0.01, 0.02, 5.0], [-0.01, 1.0, 0.03, -3.0], [0.02, -0.03, 1.0, 600.0], [0.0, 0.0, 0.0, 1.0]], dtype=np.float32)


def geometry(B, T, seed):
    """An eye some 600 mm in front of the screen: o within 30 mm of (265, 150, 0) per stream, moving by at most 0.2 mm from frame to
    frame (0.02 degrees), one inv_camera_transformation, 3.6 px / mm."""
    rng = np.random.RandomState(seed)
    o = (np.array([265.0, 150.0, 0.0]) + rng.uniform(-30, 30, (B, 1, 3)) + rng.uniform(-0.1, 0.1, (B, T, 3))).astype(np.float32)
    return o, np.tile(INV_CAM, (B, T, 1, 1)), np.full((B, T, 2), PPM, dtype=np.float32)


def path(points, seed):
    """Fixation points [T, 2] plus a jitter of at most 1 px per axis: 0.03 degrees, under 1.5 deg/s at 30 fps."""
    return (np.asarray(points, dtype=np.float64) + np.random.RandomState(seed).uniform(-1, 1, (len(points), 2))).astype(np.float32)


def same_or_adjacent_float32(got, want):
    """Equal bits, or two finite float32 of one sign next to each other; a NaN only against a NaN."""
    g, w = got.view(np.int32).astype(np.int64), want.view(np.int32).astype(np.int64)
    nan = np.isnan(want)
    return bool((np.isnan(got) == nan).all()) and bool((np.abs(g - w)[~nan] <= 1).all())


def assert_outputs(got, want, where=None):
    """got: device results (tensors); want: the reference's (numpy).  where: bool [B, T], the frames that are specified."""
    sel = (lambda a: a) if where is None else (lambda a: a[where])
    for k in EXACT:
        g = got[k].cpu().numpy()
        assert g.dtype == want[k].dtype and sel(g).tobytes() == sel(want[k]).tobytes(), k
    assert same_or_adjacent_float32(sel(got['gaze_velocity'].cpu().numpy()), sel(want['gaze_velocity']))


def assert_store(store, count, dropped, want_store, want_count, want_dropped):
    store, count, dropped = (t.cpu().numpy() for t in (store, count, dropped))
    assert count.tolist() == want_count.tolist() and dropped.tolist() == want_dropped.tolist()
    cols = [0, 1, 2, 3, 4, 5, 7]
    assert store[:, :, cols].tobytes() == want_store[:, :, cols].tobytes()
    assert (np.abs(store[:, :, 6] - want_store[:, :, 6]) <= 1e-12 * np.maximum(1.0, np.abs(want_store[:, :, 6]))).all()


def raw_call(spec, pog, o, inv_cam, ppm, state, store, count, dropped, outs, frame_time=None, valid=None, lengths=None, reset=None, flush=None):
    """The C entry point itself, so that the outputs can lie between guards too."""
    k = default_kernels()
    B, T = pog.shape[:2]
    p = k._p
    k._ck(k.lib.eve_gaze_events(B, T, p(pog), p(o), p(inv_cam), p(ppm), p(frame_time), p(valid), p(lengths), p(reset), p(flush),
                                0.0 if spec.fps is None else spec.fps, spec.min_cutoff_hz, spec.beta, spec.d_cutoff_hz,
                                1 if spec.velocity_from == 'raw' else 0, spec.saccade_deg_s, spec.min_fixation_s, spec.max_gap_s, p(state),
                                store.shape[1], p(store), p(count), p(dropped), *[p(outs[k_]) for k_ in GAZE_EVENT_KEYS], k._stream()))
    assert k.lib.eve_last_kernel().decode() == 'gaze_events_kernel'


def guarded_outputs(B, T):
    whole, outs = {}, {}
    for k_, (dtype, n) in OUT_DTYPES.items():
        sentinel = 99 if dtype in (torch.uint8, torch.int32) else -777.25
        whole[k_], outs[k_] = guarded((B, T, 2) if n == 2 else (B, T), dtype, sentinel)
        whole[k_] = (whole[k_], sentinel)
    return whole, outs


# ---------------------------------------------------------------------------------------------------------------- kernel, test 1
def test_one_chunk_with_every_kind_of_frame():
    """B = 3, T = 5, explicit times at 30 fps, every stream with a carried state that holds an open fixation of 67 ms.
    stream 0: fixation, a saccade (closes the carried fixation: the store's second and last row), a validity hole, two fixation frames
              (chained across the hole: 67 ms < max_gap_s) whose fixation the flush flag closes after 33 ms >= 30 ms: dropped, the store is full;
    stream 1: lengths 0 and a reset flag: the carried fixation goes to the store, the row is cleared but for the id counter;
    stream 2: lengths 4: a fixation frame, a NaN PoG, a NaN in inv_camera_transformation, a frame_time that does not increase, and a
              fifth frame past its length that holds NaNs."""
    B, T, F = 3, 5, 2
    spec = GazeEventSpec(min_fixation_s=0.03)
    fix = [[700.0, 500.0]] * 4
    o_all, cam_all, ppm_all = geometry(B, 4 + T, seed=1)             # the four frames before the chunk, then the chunk
    o_pre, cam_pre, ppm_pre = o_all[:, :4], cam_all[:, :4], ppm_all[:, :4]
    pre_time = np.tile(np.arange(-4, 0) / 30.0, (B, 1))
    state, store, count, dropped = ref.fresh(B, F)
    ref.run(spec, np.stack([path(fix, 10 + b) for b in range(B)]), o_pre, cam_pre, ppm_pre, state, store, count, dropped, frame_time=pre_time)
    assert (state[:, ref.FIX_OPEN] == 1).all() and (count == 0).all()
    store[:, 0] = np.arange(8) + 100.0                   # one row in use already
    count[:] = 1
    store[:, 1] = -5.5
    pog = np.stack([path([[700, 500], [850, 560], [850, 560], [850, 560], [850, 560]], 20), path([[700, 500]] * 5, 21),
                    path([[700, 500]] * 5, 22)])
    o, inv_cam, ppm = o_all[:, 4:].copy(), cam_all[:, 4:].copy(), ppm_all[:, 4:].copy()
    frame_time = np.tile(np.arange(T) / 30.0, (B, 1))
    valid = np.ones((B, T), dtype=np.uint8)
    valid[0, 2] = 0
    pog[2, 1, 0] = np.nan
    inv_cam[2, 2, 1, 2] = np.nan
    frame_time[2, 3] = -0.5
    pog[2, 4], o[2, 4], frame_time[2, 4] = np.nan, np.nan, np.nan      # past stream 2's length
    lengths, reset, flush = (np.array(a, dtype=np.int32) for a in ([5, 0, 4], [0, 1, 0], [1, 0, 0]))
    # the device's copies, every buffer between guards
    SENT = -777.25
    s_whole, d_state = guarded((B, 32), torch.float64, SENT)
    f_whole, d_store = guarded((B, F, 8), torch.float64, SENT)
    c_whole, d_count = guarded((B,), torch.int32, -7)
    x_whole, d_dropped = guarded((B,), torch.int32, -7)
    d_state.copy_(cuda(state)), d_store.copy_(cuda(store)), d_count.copy_(cuda(count)), d_dropped.copy_(cuda(dropped))
    whole, outs = guarded_outputs(B, T)
    log = ref.new_log()
    want = ref.run(spec, pog, o, inv_cam, ppm, state, store, count, dropped, frame_time=frame_time, valid=valid, lengths=lengths, reset=reset,
                   flush=flush, log=log)
    assert ref.thresholds_clear(spec, log) and len(log['closings']) == 3 and len(log['velocities']) == 5
    assert want['gaze_event'].tolist() == [[1, 2, 0, 1, 1], [0] * 5, [1, 0, 0, 0, 0]]
    assert count.tolist() == [2, 2, 1] and dropped.tolist() == [1, 0, 0] and state[1, ref.NEXT_ID] == 1 and not state[1, :ref.NEXT_ID].any()
    raw_call(spec, cuda(pog), cuda(o), cuda(inv_cam), cuda(ppm), d_state, d_store, d_count, d_dropped, outs, cuda(frame_time), cuda(valid),
             cuda(lengths), cuda(reset), cuda(flush))
    torch.cuda.synchronize()
    assert_outputs(outs, want)
    assert d_state.cpu().numpy().tobytes() == state.tobytes()
    assert_store(d_store, d_count, d_dropped, store, count, dropped)
    assert guards_hold(s_whole, SENT) and guards_hold(f_whole, SENT) and guards_hold(c_whole, -7) and guards_hold(x_whole, -7)
    for k_, (buf, sentinel) in whole.items():
        assert guards_hold(buf, sentinel), k_


# ---------------------------------------------------------------------------------------------------------------- kernel, test 2
def long_clip():
    """B = 2, T = 70 at 30 fps, counted time.  Stream 0: a saccade between frames 63 and 64 (frame 64's predecessor is the carried
    vector of the first pass) and one at frame 20.  Stream 1: frames 62 .. 65 invalid -- a gap of 167 ms from frame 61 to 66 that
    straddles the pass boundary -- and a saccade at frame 30."""
    T = 70
    a = [[700.0, 500.0]] * 20 + [[1000.0, 420.0]] * 44 + [[600.0, 700.0]] * 6
    b_ = [[900.0, 300.0]] * 30 + [[500.0, 640.0]] * 40
    pog = np.stack([path(a, 30), path(b_, 31)])
    valid = np.ones((2, T), dtype=np.uint8)
    valid[1, 62:66] = 0
    o, inv_cam, ppm = geometry(2, T, seed=3)
    return pog, o, inv_cam, ppm, valid


def device_run(spec, inputs, sizes, capacity=4, flush_last=True):
    """The clip through the wrapper in chunks of `sizes` -> (outputs joined, state, store, count, dropped)."""
    pog, o, inv_cam, ppm, valid = inputs
    B = pog.shape[0]
    k = default_kernels()
    state = torch.zeros((B, 32), dtype=torch.float64, device='cuda')
    store = torch.zeros((B, capacity, 8), dtype=torch.float64, device='cuda')
    count, dropped = torch.zeros((B,), dtype=torch.int32, device='cuda'), torch.zeros((B,), dtype=torch.int32, device='cuda')
    parts, t0 = [], 0
    for i, n in enumerate(sizes):
        cut = lambda a: cuda(a[:, t0:t0 + n])
        last = flush_last and i == len(sizes) - 1
        parts.append(k.gaze_events(cut(pog), cut(o), cut(inv_cam), cut(ppm), spec, state, store, count, dropped, valid=cut(valid),
                                   flush=torch.ones((B,), dtype=torch.int32, device='cuda') if last else None))
        t0 += n
    assert t0 == pog.shape[1]
    return {k_: torch.cat([p[k_] for p in parts], dim=1) for k_ in GAZE_EVENT_KEYS}, state, store, count, dropped


def test_seventy_frames_cross_the_pass_boundary():
    spec = GazeEventSpec(fps=30)
    inputs = long_clip()
    pog, o, inv_cam, ppm, valid = inputs
    state, store, count, dropped = ref.fresh(2, 4)
    log = ref.new_log()
    want = ref.run(spec, pog, o, inv_cam, ppm, state, store, count, dropped, valid=valid, flush=np.ones(2, dtype=np.int32), log=log)
    assert ref.thresholds_clear(spec, log)
    assert want['gaze_event'][0, 63:67].tolist() == [1, 2, 2, 1] and want['gaze_event'][0, 20] == 2      # (the filter lags one frame)
    assert want['gaze_event'][1, 60:68].tolist() == [1, 1, 0, 0, 0, 0, 0, 1] and np.isnan(want['gaze_velocity'][1, 66])
    assert count.tolist() == [3, 3] and dropped.tolist() == [0, 0]
    got, d_state, d_store, d_count, d_dropped = device_run(spec, inputs, [70])
    assert_outputs(got, want)
    assert d_state.cpu().numpy().tobytes() == state.tobytes()
    assert_store(d_store, d_count, d_dropped, store, count, dropped)


def test_chunks_equal_one_pass_on_the_device():
    spec = GazeEventSpec(fps=30)
    inputs = long_clip()
    whole = device_run(spec, inputs, [70])
    for sizes in ([64, 6], [1, 69], [10] * 7):
        split = device_run(spec, inputs, sizes)
        for k_ in GAZE_EVENT_KEYS:
            assert split[0][k_].cpu().numpy().tobytes() == whole[0][k_].cpu().numpy().tobytes(), (sizes, k_)
        for a, b_ in zip(whole[1:], split[1:]):
            assert a.cpu().numpy().tobytes() == b_.cpu().numpy().tobytes(), sizes


def test_the_stand_alone_call_is_the_kernel_call():
    spec = GazeEventSpec(fps=30)
    inputs = long_clip()
    want, _, store, count, dropped = device_run(spec, inputs, [70], capacity=256)
    pog, o, inv_cam, ppm, valid = (cuda(a) for a in inputs)
    got = data.gaze_events(pog, o, inv_cam, ppm, spec, valid=valid != 0)
    assert sorted(got) == sorted(GAZE_EVENT_KEYS + ('fixations', 'fixation_count', 'fixation_dropped'))
    for k_ in GAZE_EVENT_KEYS:
        assert got[k_].cpu().numpy().tobytes() == want[k_].cpu().numpy().tobytes(), k_
    assert torch.equal(got['fixations'], store) and torch.equal(got['fixation_count'], count) and torch.equal(got['fixation_dropped'], dropped)
    assert count.tolist() == [3, 3]
    timed = data.gaze_events(pog, o, inv_cam, ppm, GazeEventSpec(), frame_time=cuda(np.tile(np.arange(70) / 30.0, (2, 1))), valid=valid)
    for k_ in GAZE_EVENT_KEYS:                           # i / 30 as frame_time: the counted time's own values
        assert timed[k_].cpu().numpy().tobytes() == want[k_].cpu().numpy().tobytes(), k_
    with pytest.raises(ValueError, match='fps'):
        data.gaze_events(pog, o, inv_cam, ppm, GazeEventSpec())
    with pytest.raises(TypeError, match='frame_time'):
        data.gaze_events(pog, o, inv_cam, ppm, spec, frame_time=torch.zeros((2, 70), device='cuda'))


def test_the_library_refuses_without_a_launch():
    k = default_kernels()
    spec = GazeEventSpec(fps=30)
    B, T = 1, 2
    z = lambda *s, dtype=torch.float32: torch.zeros(s, dtype=dtype, device='cuda')
    state, store, count, dropped = z(B, 32, dtype=torch.float64), z(B, 2, 8, dtype=torch.float64), z(B, dtype=torch.int32), z(B, dtype=torch.int32)
    outs = {k_: z(B, T, 2, dtype=d) if n == 2 else z(B, T, dtype=d) for k_, (d, n) in OUT_DTYPES.items()}
    args = dict(pog=z(B, T, 2), o=z(B, T, 3), inv_cam=z(B, T, 4, 4), ppm=z(B, T, 2))

    class Bad(object):
        def __init__(self, **kw):
            self.__dict__.update(dict(spec.__dict__, **kw))
    for bad in (Bad(fps=0.0), Bad(fps=float('nan')), Bad(beta=-1.0), Bad(max_gap_s=0.0), Bad(min_cutoff_hz=float('inf')), Bad(saccade_deg_s=-3.0)):
        with pytest.raises(RuntimeError, match='gaze_events'):
            raw_call(bad, args['pog'], args['o'], args['inv_cam'], args['ppm'], state, store, count, dropped, outs)
    with pytest.raises(RuntimeError, match='gaze_events'):
        raw_call(spec, args['pog'], None, args['inv_cam'], args['ppm'], state, store, count, dropped, outs)
    with pytest.raises(RuntimeError, match='gaze_events'):
        raw_call(spec, args['pog'], args['o'], args['inv_cam'], args['ppm'], None, store, count, dropped, outs)
    with pytest.raises(TypeError, match='state'):
        k.gaze_events(args['pog'], args['o'], args['inv_cam'], args['ppm'], spec, state.float(), store, count, dropped)
    with pytest.raises(TypeError, match='ppm'):
        k.gaze_events(args['pog'], args['o'], args['inv_cam'], z(B, T, 3), spec, state, store, count, dropped)
    torch.cuda.synchronize()
    assert not state.any() and not count.any()


# ---------------------------------------------------------------------------------------------------------------- EVEStream
S, TC = 3, 5


@pytest.fixture(scope='module')
def rig():
    """One model and one 3 x 10 clip, shared and never modified."""
    model, _ = make_model(refine_net_rnn_type='CGRU')
    _, d, _ = gpu_clip(S, 2 * TC, seed=7)
    chunk = lambda t0, t1: {k: v[:, t0:t1].contiguous() for k, v in d.items()}
    return {'model': model, 'chunks': (chunk(0, TC), chunk(TC, 2 * TC))}


def keep(out):
    return {k: v.clone() for k, v in out.items()}


def check_against_reference(outs, chunks, spec, source='PoG_px_final', lengths=None, frame_times=None):
    """Two steps' event outputs == the reference on the steps' OWN source PoG and origin, the state carried between them."""
    state, store, count, dropped = ref.fresh(S, 256)
    for i, (out, chunk) in enumerate(zip(outs, chunks)):
        o = _mean2(chunk['left_o'], chunk['right_o']) if 'eye_valid' not in out else _fuse2(chunk['left_o'], chunk['right_o'], out['eye_valid'])
        valid = out['valid'].cpu().numpy() if 'eye_valid' in out else None
        log = ref.new_log()
        want = ref.run(spec, out[source].cpu().numpy(), o.float().cpu().numpy(), chunk['inv_camera_transformation'].float().cpu().numpy(),
                       chunk['pixels_per_millimeter'].float().cpu().numpy(), state, store, count, dropped, valid=valid,
                       frame_time=None if frame_times is None else frame_times[i].cpu().numpy(),
                       lengths=None if lengths is None else np.asarray(lengths[i]), log=log)
        assert ref.thresholds_clear(spec, log) and log['velocities']
        where = out['valid'].cpu().numpy() if 'valid' in out else None
        assert_outputs(out, want, where)
    return state, store, count, dropped


def two_steps(stream, chunks, lengths=None, frame_time=None, **kw):
    """lengths, frame_time: None or one entry per step."""
    outs = []
    for i, chunk in enumerate(chunks):
        if lengths is not None:
            kw['lengths'] = lengths[i]
        outs.append(keep(stream.step(chunk if frame_time is None else dict(chunk, frame_time=frame_time[i]), **kw)))
    return outs


def specified(a, out):
    """The entries of a result that the step specifies: those at valid frames, where the step reports `valid`."""
    return a[out['valid']] if 'valid' in out and tuple(a.shape[:2]) == tuple(out['valid'].shape) else a


def assert_replay_is_eager(eager, graph):
    for e, g in zip(eager, graph):
        assert sorted(e) == sorted(g)
        for k_ in e:
            assert specified(e[k_], e).cpu().numpy().tobytes() == specified(g[k_], e).cpu().numpy().tobytes(), k_


@pytest.mark.parametrize('mode', ['lengths', 'eye_mask'])
def test_stream_events_eager_and_captured(rig, mode):
    model, chunks = rig['model'], rig['chunks']
    spec = GazeEventSpec(fps=30)
    if mode == 'lengths':
        kw = dict(lengths=[[5, 0, 4], [5, 3, 5]])
    else:
        mask = torch.ones((S, TC, 2), dtype=torch.bool, device='cuda')
        mask[0, 1, 0] = mask[0, 3, 1] = mask[2, 2, 0] = mask[2, 2, 1] = False
        mask[1, :, 1] = False
        kw = dict(eye_mask=mask)
    eager_stream, graph_stream = eve_amd.EVEStream(model, S, use_graph=False), eve_amd.EVEStream(model, S)
    eager = two_steps(eager_stream, chunks, events=spec, **kw)
    graph = two_steps(graph_stream, chunks, events=spec, **kw)
    assert_replay_is_eager(eager, graph)
    assert len(graph_stream._graphs) == 1                                # the second step replayed the first one's graph
    state, store, count, dropped = check_against_reference(eager, chunks, spec, lengths=kw.get('lengths'))
    for s_ in (eager_stream, graph_stream):                              # (the capture's warm-up steps did not tick the filter)
        assert s_.get_event_state().cpu().numpy().tobytes() == state.tobytes()
        assert_store(*s_._events[1:], store, count, dropped)
    ticks = [10, 3, 9] if mode == 'lengths' else [10, 10, 10]
    assert state[:, ref.TICKS].tolist() == ticks
    # without events the same EVEStream returns the plain step's bits, and its events' state stays
    plain = keep(eve_amd.EVEStream(model, S).step(chunks[0], **{k_: (v[0] if k_ == 'lengths' else v) for k_, v in kw.items()}))
    graph_stream.reset()
    back = graph_stream.step(chunks[0], **{k_: (v[0] if k_ == 'lengths' else v) for k_, v in kw.items()})
    assert sorted(back) == sorted(plain)
    for k_ in plain:
        assert specified(back[k_], plain).cpu().numpy().tobytes() == specified(plain[k_], plain).cpu().numpy().tobytes(), k_


def test_stream_events_feed_the_overlay(rig):
    """events with frame_time and render: a fixation marker at fixation_px, drawn where fixating, and the filtered point."""
    model = rig['model']
    cap = nv12_capture(43, B=S, T=2 * TC)
    chunks = [dict({k_: v for k_, v in c.items() if k_ != 'screen_frame'}, screen_frame_nv12=cap[:, i * TC:(i + 1) * TC].contiguous())
              for i, c in enumerate(rig['chunks'])]
    times = [cuda(np.tile(np.arange(i * TC, (i + 1) * TC) / 60.0, (S, 1)) + np.arange(S)[:, None] * 100.0) for i in range(2)]
    spec = GazeEventSpec(saccade_deg_s=400.0, min_fixation_s=0.03)
    overlay = OverlaySpec(markers=[dict(key='fixation_px', valid='fixating', r_fill=3, r_outline=5), dict(key='PoG_px_filtered', r_fill=2, r_outline=3)],
                          inset=None, out_format='rgb')
    eager = two_steps(eve_amd.EVEStream(model, S, use_graph=False), chunks, events=spec, render=overlay, frame_time=times)
    graph = two_steps(eve_amd.EVEStream(model, S), chunks, events=spec, render=overlay, frame_time=times)
    assert_replay_is_eager(eager, graph)
    check_against_reference(eager, chunks, spec, frame_times=times)
    N, (IH, IW) = S * TC, CAPTURE
    drawn = 0
    for out, chunk in zip(eager, chunks):
        markers = dict(centres=np.stack([out['fixation_px'].reshape(N, 2).cpu().numpy(), out['PoG_px_filtered'].reshape(N, 2).cpu().numpy()], axis=1),
                       table=np.array(overlay.marker_table(), dtype=np.int32).reshape(-1, 4),
                       valid=np.stack([out['fixating'].reshape(N).cpu().numpy(), np.ones(N, dtype=np.uint8)], axis=1),
                       sx=np.float32(IW / 1920.0), sy=np.float32(IH / 1080.0))
        flat = chunk['screen_frame_nv12'].reshape((N,) + tuple(chunk['screen_frame_nv12'].shape[2:])).cpu().numpy()
        want = oref.render(flat, 'nv12', 'rgb', 'bt601', markers, None, None, None)
        assert np.array_equal(out['rendered'].reshape(want.shape).cpu().numpy(), want)
        drawn += int(out['fixating'].sum())
    assert drawn > 0
    with pytest.raises(ValueError, match='fixation_px'):
        eve_amd.EVEStream(model, S, use_graph=False).step(chunks[0], render=overlay)


def test_reset_closes_the_fixation_and_restarts_the_ticks(rig):
    model, chunks = rig['model'], rig['chunks']
    spec = GazeEventSpec(fps=30, saccade_deg_s=1e9, min_fixation_s=0.03)     # everything fixates: one fixation per stream from frame 1 on
    stream = eve_amd.EVEStream(model, S, fixation_capacity=4)
    first = keep(stream.step(chunks[0], events=spec))
    assert first['gaze_event'].tolist() == [[0, 1, 1, 1, 1]] * S and stream.fixation_counts()[0].tolist() == [0, 0, 0]
    opened = stream.fixations(include_open=True)
    assert [f.shape for f in opened] == [(1, 8)] * S and [f.shape for f in stream.fixations()] == [(0, 8)] * S
    stream.reset([1])
    second = keep(stream.step(chunks[1], events=spec))
    count, dropped = stream.fixation_counts()
    assert count.tolist() == [0, 1, 0] and dropped.tolist() == [0, 0, 0]
    assert np.array_equal(stream.fixations()[1], opened[1]) and opened[1][0, 3] == 4
    assert second['gaze_event'].tolist() == [[1] * 5, [0, 1, 1, 1, 1], [1] * 5]
    assert second['fixation_id'].tolist() == [[0] * 5, [-1, 1, 1, 1, 1], [0] * 5]
    state = stream.get_event_state().cpu().numpy()
    assert state[:, ref.TICKS].tolist() == [10, 5, 10] and state[:, ref.NEXT_ID].tolist() == [1, 2, 1]
    assert np.allclose(second['fixation_ms'][:, 4].cpu().numpy(), [1000 * 8 / 30.0, 1000 * 3 / 30.0, 1000 * 8 / 30.0])
    stream.flush_fixations()
    assert stream.fixation_counts()[0].tolist() == [1, 2, 1] and not stream.get_event_state()[:, ref.FIX_OPEN].any()
    assert [f[-1, 3] for f in stream.fixations()] == [9, 4, 9]
    stream.clear_fixations([1])
    assert stream.fixation_counts()[0].tolist() == [1, 0, 1]
