"""GPU: eve_gaze_events_ex and eve_gaze_saccades against the numpy contract of tests/saccade_ref.py, and EVEStream's step(events=...,
saccades=...) around them (eager and captured).  Every test here needs the new entry points, SaccadeSpec or the saccades argument, so
every one fails without them.

What must be equal.  eve_gaze_events_ex against eve_gaze_events on the same inputs: everything, bit for bit; its sample, sample_time
and gaze_vector against the reference: bit for bit (nothing but + - * / and comparisons leads to them).  eve_gaze_saccades fed the
REFERENCE's arrays: saccade_id, saccade_ms, the state rows, the counters and every store and table column that holds only + - * /,
max and comparisons, bit for bit; amplitude and mean velocity within 1e-12 * max(1, |reference|) (a double sqrt / atan2 chain, the
bound of test_gpu_calibration.py); a table column that sums k such terms within 2 k times that bound (amp * amp doubles the
relative error of a term, and the k additions add less than k ulp).  Fed the DEVICE's own events -- whose float32 velocity is the
reference's or the float32 next to it (test_gpu_gaze_events.py) -- peak_deg_s is the same or an adjacent float32, the state's peak
entry too, and a column that sums peaks is within the sum of one float32 step per term (times the amplitude for sum amp * peak) on top
of its other bound.  Exact verdicts are fair only away from the thresholds, so each comparison first asserts ON THE REFERENCE ALONE
that both thresholds_clear hold."""
import math

import numpy as np
import pytest
import torch

import eve_amd
import gaze_events_ref as eref
import saccade_ref as ref
from eve_amd import data
from eve_amd.data import GAZE_EVENT_KEYS, SACCADE_KEYS, GazeEventSpec, SaccadeSpec
from eve_amd.eve import _fuse2, _mean2
from eve_amd.kernels import default_kernels
from test_gpu_calibration import cuda, guarded, guards_hold
from test_gpu_gaze_events import INV_CAM, OUT_DTYPES, PPM, same_or_adjacent_float32
from test_gpu_stream import gpu_clip, make_model

pytestmark = pytest.mark.gpu
FPS = 120
DEG_PX = 600.0 * math.tan(math.radians(1.0)) * PPM       # one degree on the screen under the eye, in pixels
RAW = GazeEventSpec(fps=FPS, velocity_from='raw')
EX_KEYS = ('sample', 'sample_time', 'gaze_vector')
EX_DTYPES = {'sample': (torch.uint8, ()), 'sample_time': (torch.float64, ()), 'gaze_vector': (torch.float64, (3,))}
BOUND = 1e-12


def close(got, want, k=1):
    return bool((np.abs(got - want) <= k * BOUND * np.maximum(1.0, np.abs(want))).all())


# ---------------------------------------------------------------------------------------------------------------- the clip
def degrees(x):
    """x: degrees to the right of (700, 500), one entry per frame -> pog [T, 2] float32."""
    pog = np.zeros((len(x), 2), dtype=np.float32)
    pog[:, 0], pog[:, 1] = 700.0 + np.asarray(x) * DEG_PX, 500.0
    return pog


def the_clip():
    """B = 3, T = 70 at 120 fps, the velocity from the raw point.
    stream 0: a 6 degree saccade over frames 20 .. 22 and a 10 degree one over frames 62 .. 66, across the 64-frame pass: two accepted;
    stream 1: a saccade over frames 30 .. 33 whose frame 31 is invalid (interrupted at max_missing 0), a ramp from frame 48 on whose
              frames 50 .. 59 are invalid (92 ms between samples: the restart at frame 60 aborts it), a 0.3 degree step at frame 65 (small);
    stream 2: lengths 40: a saccade over frames 10 .. 12, one that sets out at frame 38 and is open when the frames end; the frames
              past the length hold NaNs."""
    T = 70
    a = [0.0] * 20 + [2.0, 4.0, 6.0] + [6.0] * 39 + [8.0, 10.0, 12.0, 14.0, 16.0] + [16.0] * 3
    b_ = [0.0] * 30 + [2.0, 4.0, 6.0, 8.0] + [8.0] * 14 + [10.0 + 2 * i for i in range(12)] + [32.0] * 5 + [32.3] * 5
    c = [0.0] * 10 + [3.0, 6.0, 9.0] + [9.0] * 25 + [11.0, 13.0] + [13.0] * 30
    pog = np.stack([degrees(a), degrees(b_), degrees(c)])
    valid = np.ones((3, T), dtype=np.uint8)
    valid[1, 31] = 0
    valid[1, 50:60] = 0
    o = np.tile(np.array([265.0, 150.0, 0.0], dtype=np.float32), (3, T, 1)) + np.arange(3, dtype=np.float32)[:, None, None]
    inv_cam, ppm = np.tile(INV_CAM, (3, T, 1, 1)), np.full((3, T, 2), PPM, dtype=np.float32)
    pog[2, 40:], o[2, 40:] = np.nan, np.nan
    return pog, o, inv_cam, ppm, valid, np.array([70, 70, 40], dtype=np.int32)


@pytest.fixture(scope='module')
def clip():
    """The clip, the reference's events and saccades on it in one pass from fresh state: computed once, shared, never modified."""
    pog, o, inv_cam, ppm, valid, lengths = the_clip()
    sspec = SaccadeSpec()
    ecarried, carried = eref.fresh(3, 8), ref.fresh(3, 4)
    elog, log = eref.new_log(), ref.new_log()
    ex = ref.events_ex(RAW, pog, o, inv_cam, ppm, *ecarried, valid=valid, lengths=lengths, log=elog)
    out = ref.run(sspec, *saccade_inputs(ex, pog), *carried, lengths=lengths, log=log)
    assert eref.thresholds_clear(RAW, elog) and ref.thresholds_clear(sspec, log)
    state, table, store, count, dropped = carried
    assert count.tolist() == [2, 0, 1] and table[:, ref.ACCEPTED].tolist() == [2, 0, 1] and state[:, ref.OPEN].tolist() == [0, 0, 1]
    assert table[1, ref.ABORTED:ref.INTERRUPTED + 1].tolist() == [1, 1, 0, 0, 1]
    assert out['saccade_id'][0, 61:68].tolist() == [-1, 1, 1, 1, 1, 1, -1] and store[0, 1, ref.R_N] == 5      # across the pass
    return dict(inputs=(pog, o, inv_cam, ppm, valid, lengths), ex=ex, out=out, ecarried=ecarried, carried=carried, sspec=sspec)


def saccade_inputs(ex, pog):
    return [ex['sample'], ex['sample_time'], ex['gaze_vector'], np.nan_to_num(pog), ex['gaze_event'], ex['gaze_velocity'], ex['fixation_id']]


def device_buffers(B, capacity):
    """The five carried buffers of fresh streams between guards -> ((whole, sentinel) pairs, buffers)."""
    SENT = -777.25
    shapes = [((B, 32), torch.float64, SENT), ((B, 16), torch.float64, SENT), ((B, capacity, 16), torch.float64, SENT), ((B,), torch.int32, -7),
              ((B,), torch.int32, -7)]
    pairs = [guarded(shape, dtype, sentinel) for shape, dtype, sentinel in shapes]
    for _, payload in pairs:
        payload.zero_()
    return [(whole, s_[2]) for (whole, _), s_ in zip(pairs, shapes)], [payload for _, payload in pairs]


def assert_carried(got, want, device_events=False):
    """got: the five device buffers; want: the reference's."""
    state, table, store, count, dropped = (t.cpu().numpy() for t in got)
    w_state, w_table, w_store, w_count, w_dropped = want
    assert count.tolist() == w_count.tolist() and dropped.tolist() == w_dropped.tolist()
    state_cols = [c for c in range(32) if not (device_events and c == ref.PEAK)]
    assert state[:, state_cols].tobytes() == w_state[:, state_cols].tobytes()
    store_cols = [c for c in range(16) if c not in ref.TRANSCENDENTAL_ROW and not (device_events and c in ref.PEAK_ROW)]
    assert store[:, :, store_cols].tobytes() == w_store[:, :, store_cols].tobytes()
    for c in ref.TRANSCENDENTAL_ROW:
        assert close(store[:, :, c], w_store[:, :, c]), c
    table_cols = [c for c in range(16) if c not in ref.TRANSCENDENTAL_TABLE and not (device_events and c in ref.PEAK_TABLE)]
    assert table[:, table_cols].tobytes() == w_table[:, table_cols].tobytes()
    k = np.maximum(w_table[:, ref.ACCEPTED], 1.0)
    step32 = lambda a: np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)
    peak_step = np.zeros((len(w_count), 2))              # per stream: the sums of one float32 step per stored peak, plain and times amp
    if device_events:
        assert same_or_adjacent_float32(state[:, ref.PEAK].astype(np.float32), w_state[:, ref.PEAK].astype(np.float32))
        assert same_or_adjacent_float32(store[:, :, ref.R_PEAK].astype(np.float32), w_store[:, :, ref.R_PEAK].astype(np.float32))
        assert (w_dropped == 0).all()                    # (every accepted saccade is a stored row: the sums below are over the rows)
        for b in range(len(w_count)):
            rows = w_store[b, :w_count[b]]
            peak_step[b] = [step32(rows[:, ref.R_PEAK]).sum(), (rows[:, ref.R_AMP] * step32(rows[:, ref.R_PEAK])).sum()]
    for c in ref.TRANSCENDENTAL_TABLE + (ref.PEAK_TABLE if device_events else ()):
        extra = 0.0 if c not in ref.PEAK_TABLE else peak_step[:, 1] * (1 + 1e-9) if c == ref.SUM_AP else peak_step[:, 0]
        bound = (2 * k * BOUND * np.maximum(1.0, np.abs(w_table[:, c])) if c in ref.TRANSCENDENTAL_TABLE else 0.0) + extra
        assert (np.abs(table[:, c] - w_table[:, c]) <= bound).all(), c


# ---------------------------------------------------------------------------------------------------------------- eve_gaze_events_ex
def events_call(entry, spec, arrays, carried, outs, valid=None, lengths=None, reset=None):
    """One of the two C entry points itself, so that the outputs can lie between guards."""
    k = default_kernels()
    pog, o, inv_cam, ppm = arrays
    state, store, count, dropped = carried
    B, T = pog.shape[:2]
    p = k._p
    keys = GAZE_EVENT_KEYS + (EX_KEYS if entry == 'eve_gaze_events_ex' else ())
    k._ck(getattr(k.lib, entry)(B, T, p(pog), p(o), p(inv_cam), p(ppm), None, p(valid), p(lengths), p(reset), None,
                                0.0 if spec.fps is None else spec.fps, spec.min_cutoff_hz, spec.beta, spec.d_cutoff_hz,
                                1 if spec.velocity_from == 'raw' else 0, spec.saccade_deg_s, spec.min_fixation_s, spec.max_gap_s, p(state),
                                store.shape[1], p(store), p(count), p(dropped), *[p(outs[k_]) for k_ in keys], k._stream()))
    assert k.lib.eve_last_kernel().decode() == 'gaze_events_kernel'      # both entries launch the one kernel


def test_events_ex_is_the_events_launch_and_hands_out_the_reference_s_arrays(clip):
    pog, o, inv_cam, ppm, valid, lengths = clip['inputs']
    B, T = pog.shape[:2]
    arrays = [cuda(a) for a in (pog, o, inv_cam, ppm)]
    z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device='cuda')
    fresh = lambda: (z(B, 32), z(B, 8, 8), z(B, dtype=torch.int32), z(B, dtype=torch.int32))
    plain_carried, ex_carried = fresh(), fresh()
    plain = {k_: torch.zeros((B, T, 2) if n == 2 else (B, T), dtype=d, device='cuda') for k_, (d, n) in OUT_DTYPES.items()}
    whole, outs = {}, {}
    tails = dict({k_: (d, (2,) if n == 2 else ()) for k_, (d, n) in OUT_DTYPES.items()}, **EX_DTYPES)
    for k_, (dtype, tail) in tails.items():
        sentinel = 99 if dtype in (torch.uint8, torch.int32) else -777.25
        buf, outs[k_] = guarded((B, T) + tail, dtype, sentinel)
        whole[k_] = (buf, sentinel)
    events_call('eve_gaze_events', RAW, arrays, plain_carried, plain, cuda(valid), cuda(lengths))
    events_call('eve_gaze_events_ex', RAW, arrays, ex_carried, outs, cuda(valid), cuda(lengths))
    torch.cuda.synchronize()
    for k_ in GAZE_EVENT_KEYS:
        assert outs[k_].cpu().numpy().tobytes() == plain[k_].cpu().numpy().tobytes(), k_
    for a, b_ in zip(plain_carried, ex_carried):
        assert a.cpu().numpy().tobytes() == b_.cpu().numpy().tobytes()
    assert ex_carried[0].cpu().numpy().tobytes() == clip['ecarried'][0].tobytes()      # (and the reference's state row)
    for k_ in EX_KEYS:
        got = outs[k_].cpu().numpy()
        assert got.dtype == clip['ex'][k_].dtype and got.tobytes() == clip['ex'][k_].tobytes(), k_
    assert set(np.unique(clip['ex']['sample'])) == {0, 1, 2} and not clip['ex']['sample'][2, 40:].any()
    for k_, (buf, sentinel) in whole.items():
        assert guards_hold(buf, sentinel), k_
    # the wrapper: the ten keys, the same bits; each of the three outputs may be absent
    res = default_kernels().gaze_events_ex(*arrays, RAW, *fresh(), valid=cuda(valid), lengths=cuda(lengths))
    assert sorted(res) == sorted(GAZE_EVENT_KEYS + EX_KEYS)
    for k_ in res:
        assert res[k_].cpu().numpy().tobytes() == outs[k_].cpu().numpy().tobytes(), k_
    some = dict(outs, sample=None, gaze_vector=None)
    outs['sample_time'].fill_(-1.0)
    events_call('eve_gaze_events_ex', RAW, arrays, fresh(), some, cuda(valid), cuda(lengths))
    assert outs['sample_time'].cpu().numpy().tobytes() == clip['ex']['sample_time'].tobytes()


# ---------------------------------------------------------------------------------------------------------------- eve_gaze_saccades
def saccades_call(sspec, frames, carried, outs, lengths=None, reset=None, T=None):
    """The C entry point itself.  frames: the seven frame inputs (device tensors) or Nones; -> its status."""
    k = default_kernels()
    state, table, store, count, dropped = carried
    p = k._p
    T = frames[0].shape[1] if T is None else T
    return k.lib.eve_gaze_saccades(state.shape[0] if state is not None else 1, T, *[p(a) for a in frames], p(lengths), p(reset),
                                   sspec.min_amplitude_deg, sspec.min_duration_s, sspec.max_duration_s, sspec.max_missing, p(state), p(table),
                                   store.shape[1] if store is not None else 1, p(store), p(count), p(dropped), p(outs[0]), p(outs[1]), k._stream())


def test_seventy_frames_with_every_verdict_between_guards(clip):
    pog, _, _, _, _, lengths = clip['inputs']
    B, T = pog.shape[:2]
    frames = [cuda(a) for a in saccade_inputs(clip['ex'], pog)]
    wholes, carried = device_buffers(B, 4)
    id_whole, d_id = guarded((B, T), torch.int32, 99)
    ms_whole, d_ms = guarded((B, T), torch.float32, -777.25)
    assert saccades_call(clip['sspec'], frames, carried, (d_id, d_ms), cuda(lengths)) == 0
    torch.cuda.synchronize()
    assert default_kernels().lib.eve_last_kernel().decode() == 'gaze_saccades_kernel'
    assert d_id.cpu().numpy().tobytes() == clip['out']['saccade_id'].tobytes()
    assert d_ms.cpu().numpy().tobytes() == clip['out']['saccade_ms'].tobytes()
    assert_carried(carried, clip['carried'])
    assert guards_hold(id_whole, 99) and guards_hold(ms_whole, -777.25) and all(guards_hold(w, s_) for w, s_ in wholes)


def device_run(sspec, clip, sizes, capacity=4, resets=None):
    """The clip's reference arrays through the wrapper in chunks of `sizes` -> (outputs joined, the five buffers)."""
    pog, _, _, _, _, lengths = clip['inputs']
    arrays = saccade_inputs(clip['ex'], pog)
    B = pog.shape[0]
    k = default_kernels()
    carried = data.saccade_buffers(B, capacity, 'cuda')
    parts, t0 = [], 0
    for i, n in enumerate(sizes):
        parts.append(k.gaze_saccades(*[cuda(a[:, t0:t0 + n]) for a in arrays], sspec, *carried, lengths=cuda(np.clip(lengths - t0, 0, n).astype(np.int32)),
                                     reset=None if resets is None else cuda(np.asarray(resets[i], dtype=np.int32))))
        t0 += n
    assert t0 == pog.shape[1]
    return {k_: torch.cat([p[k_] for p in parts], dim=1) for k_ in SACCADE_KEYS}, carried


def test_chunks_equal_one_pass_on_the_device(clip):
    whole = device_run(clip['sspec'], clip, [70])
    for k_ in SACCADE_KEYS:
        assert whole[0][k_].cpu().numpy().tobytes() == clip['out'][k_].tobytes(), k_
    for sizes in ([64, 6], [1, 69], [10] * 7, [63, 1, 1, 5]):
        split = device_run(clip['sspec'], clip, sizes)
        for k_ in SACCADE_KEYS:
            assert split[0][k_].cpu().numpy().tobytes() == whole[0][k_].cpu().numpy().tobytes(), (sizes, k_)
        for a, b_ in zip(whole[1], split[1]):
            assert a.cpu().numpy().tobytes() == b_.cpu().numpy().tobytes(), sizes      # exactly, in every column: the atan2 is the device's in both


def test_the_other_verdicts_on_the_same_frames(clip):
    """Another spec on the clip's arrays: the 25 ms saccades and the one-interval step are short (the rule before small), the 42 ms
    one is long, and the one with a missing frame is accepted with missing = 1."""
    pog, _, _, _, _, lengths = clip['inputs']
    sspec = SaccadeSpec(min_duration_s=0.03, max_duration_s=0.04, max_missing=1)
    want, log = ref.fresh(3, 4), ref.new_log()
    out = ref.run(sspec, *saccade_inputs(clip['ex'], pog), *want, lengths=lengths, log=log)
    assert ref.thresholds_clear(sspec, log)
    assert want[1][:, [ref.ACCEPTED, ref.SHORT, ref.LONG, ref.INTERRUPTED]].tolist() == [[0, 1, 1, 0], [1, 1, 0, 0], [0, 1, 0, 0]]
    assert want[2][1, 0, ref.R_MISSING] == 1 and want[2][1, 0, ref.R_N] == 3
    got, carried = device_run(sspec, clip, [70])
    for k_ in SACCADE_KEYS:
        assert got[k_].cpu().numpy().tobytes() == out[k_].tobytes(), k_
    assert_carried(carried, want)


def test_one_frame_no_frames_with_reset_flags_and_a_full_store(clip):
    pog, _, _, _, _, lengths = clip['inputs']
    arrays = saccade_inputs(clip['ex'], pog)
    k = default_kernels()
    sspec = clip['sspec']
    # 64 frames, then T = 1 (frame 64, inside stream 0's second saccade), then T = 0 with reset flags, then the rest with a reset of
    # stream 2 -- against the reference walked the same way; a store of one row: stream 0's second saccade is dropped
    want, got = ref.fresh(3, 1), data.saccade_buffers(3, 1, 'cuda')
    steps = [(0, 64, None), (64, 65, None), (65, 65, [1, 0, 1]), (65, 70, [0, 0, 1])]
    for t0, t1, reset in steps:
        n = t1 - t0
        ln = np.clip(lengths - t0, 0, n).astype(np.int32)
        rs = None if reset is None else np.asarray(reset, dtype=np.int32)
        if n:
            w = ref.run(sspec, *[a[:, t0:t1] for a in arrays], *want, lengths=ln, reset=rs)
            g = k.gaze_saccades(*[cuda(a[:, t0:t1]) for a in arrays], sspec, *got, lengths=cuda(ln), reset=None if rs is None else cuda(rs))
            for k_ in SACCADE_KEYS:
                assert g[k_].cpu().numpy().tobytes() == w[k_].tobytes(), (t0, k_)
        else:
            ref.run(sspec, None, None, None, None, None, None, None, *want, reset=rs)
            assert k.gaze_saccades(None, None, None, None, None, None, None, sspec, *got, reset=cuda(rs)) == {}
        assert_carried(got, want)
        if (t0, t1) == (64, 65):
            assert want[0][0, ref.OPEN] == 1 and want[0][0, ref.N] == 3 and g['saccade_id'][0, 0] == 1
    state, table, store, count, dropped = want
    assert table[:, ref.ABORTED].tolist() == [1, 1, 1] and count.tolist() == [1, 0, 1] and dropped.tolist() == [0, 0, 0]
    assert state[:, ref.NEXT_ID].tolist() == [2, 3, 2] and not state[2, :ref.NEXT_ID].any()
    full = device_run(sspec, clip, [70], capacity=1)[1]
    assert full[3].tolist() == [1, 0, 1] and full[4].tolist() == [1, 0, 0] and full[1][0, ref.ACCEPTED] == 2
    assert full[2][0, 0].cpu().numpy().tobytes() == got[2][0, 0].cpu().numpy().tobytes()


def test_the_library_refuses_without_a_launch(clip):
    k = default_kernels()
    pog = clip['inputs'][0]
    frames = [cuda(a[:, :2]) for a in saccade_inputs(clip['ex'], pog)]
    carried = list(data.saccade_buffers(3, 2, 'cuda'))
    outs = (torch.zeros((3, 2), dtype=torch.int32, device='cuda'), torch.zeros((3, 2), dtype=torch.float32, device='cuda'))
    k.gaze_events(None, None, None, None, RAW, torch.zeros((1, 32), dtype=torch.float64, device='cuda'),
                  torch.zeros((1, 1, 8), dtype=torch.float64, device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda'),
                  torch.zeros(1, dtype=torch.int32, device='cuda'))
    before = k.lib.eve_last_kernel()
    assert before == b'gaze_events_kernel'

    class Bad(object):
        def __init__(self, **kw):
            self.__dict__.update(dict(SaccadeSpec().__dict__, **kw))

    def refused(status, *words):
        msg = k.lib.eve_last_error().decode()
        assert status != 0 and msg.startswith('gaze_saccades:') and all(w in msg for w in words), msg
        assert k.lib.eve_last_kernel() == before

    for i in range(5):
        refused(saccades_call(SaccadeSpec(), frames, carried[:i] + [None] + carried[i + 1:], outs), 'null carried buffer')
    for i in range(7):
        refused(saccades_call(SaccadeSpec(), frames[:i] + [None] + frames[i + 1:], carried, outs, T=2), 'null frame input or output')
    refused(saccades_call(SaccadeSpec(), frames, carried, (None, outs[1])), 'null frame input or output')
    refused(saccades_call(SaccadeSpec(), frames, carried, outs, T=-1), 'T >= 0')
    refused(k.lib.eve_gaze_saccades(3, 2, *[k._p(a) for a in frames], None, None, 0.5, 0.0, 0.2, 0, *[k._p(a) for a in carried[:2]], 0,
                                    *[k._p(a) for a in carried[2:]], k._p(outs[0]), k._p(outs[1]), k._stream()), 'S >= 1')
    refused(k.lib.eve_gaze_saccades(1 << 27, 0, *[None] * 9, 0.5, 0.0, 0.2, 0, *[k._p(a) for a in carried[:2]], 1,
                                    *[k._p(a) for a in carried[2:]], None, None, k._stream()), '31 bits')
    refused(k.lib.eve_gaze_saccades(1 << 20, 0, *[None] * 9, 0.5, 0.0, 0.2, 0, *[k._p(a) for a in carried[:2]], 1 << 10,
                                    *[k._p(a) for a in carried[2:]], None, None, k._stream()), 'S * 16', '31 bits')
    for name in ('min_amplitude_deg', 'min_duration_s', 'max_duration_s'):
        for bad in (float('nan'), float('inf'), -float('inf')):
            refused(saccades_call(Bad(**{name: bad}), frames, carried, outs), 'finite')
    refused(saccades_call(Bad(min_amplitude_deg=-0.1), frames, carried, outs), 'min_amplitude_deg')
    refused(saccades_call(Bad(max_duration_s=0.0), frames, carried, outs), 'max_duration_s')
    refused(saccades_call(Bad(min_duration_s=-1e-9), frames, carried, outs), 'min_duration_s')
    refused(saccades_call(Bad(max_missing=-1), frames, carried, outs), 'max_missing')
    # the wrapper's own type and shape checks
    with pytest.raises(TypeError, match='state'):
        k.gaze_saccades(*frames, SaccadeSpec(), carried[0].float(), *carried[1:])
    with pytest.raises(TypeError, match='store'):
        k.gaze_saccades(*frames, SaccadeSpec(), carried[0], carried[1], carried[2][:, :, :8].contiguous(), *carried[3:])
    with pytest.raises(TypeError, match='gaze_vector'):
        k.gaze_saccades(frames[0], frames[1], frames[2].float(), *frames[3:], SaccadeSpec(), *carried)
    with pytest.raises(TypeError, match='velocity'):
        k.gaze_saccades(*frames[:5], frames[5][:, :1].contiguous(), frames[6], SaccadeSpec(), *carried)
    with pytest.raises(TypeError, match='no frame inputs'):
        k.gaze_saccades(None, frames[1], None, None, None, None, None, SaccadeSpec(), *carried)
    torch.cuda.synchronize()
    assert k.lib.eve_last_kernel() == before and not any(t.any() for t in carried) and not outs[0].any()


# ---------------------------------------------------------------------------------------------------------------- the device's own events
def test_the_stand_alone_entry_on_the_device_s_own_events(clip):
    pog, o, inv_cam, ppm, valid, _ = clip['inputs']
    keep = slice(0, 2)                                    # (the stand-alone entry takes no lengths: the two full streams)
    args = [cuda(a[keep]) for a in (np.nan_to_num(pog), np.nan_to_num(o), inv_cam, ppm)]
    res = data.gaze_saccades(*args, RAW, clip['sspec'], valid=cuda(valid[keep]) != 0, saccade_capacity=4)
    assert sorted(res) == sorted(GAZE_EVENT_KEYS + SACCADE_KEYS + ('saccades', 'saccade_count', 'saccade_dropped', 'saccade_table'))
    for k_ in SACCADE_KEYS:
        assert res[k_].cpu().numpy().tobytes() == clip['out'][k_][keep].tobytes(), k_
    for k_ in ('gaze_event', 'fixation_id'):
        assert res[k_].cpu().numpy().tobytes() == clip['ex'][k_][keep].tobytes(), k_
    assert same_or_adjacent_float32(res['gaze_velocity'].cpu().numpy(), clip['ex']['gaze_velocity'][keep])
    state, table, store, count, dropped = (a[keep] for a in clip['carried'])
    got = (cuda(state), res['saccade_table'], res['saccades'], res['saccade_count'], res['saccade_dropped'])      # (the entry returns no state row)
    assert_carried(got, (state, table, store, count, dropped), device_events=True)
    fit = data.main_sequence(res['saccade_table'])
    assert fit['n'].tolist() == [2, 0] and fit['duration_slope'][0] > 0 and np.isnan(fit['duration_slope'][1])


S, TC = 3, 5


@pytest.fixture(scope='module')
def rig():
    """One model, one 3 x 10 clip and a saccade threshold in the middle of the clip's own velocities: shared and never modified."""
    model, _ = make_model(refine_net_rnn_type='CGRU')
    _, d, _ = gpu_clip(S, 2 * TC, seed=7)
    chunk = lambda t0, t1: {k: v[:, t0:t1].contiguous() for k, v in d.items()}
    chunks = (chunk(0, TC), chunk(TC, 2 * TC))
    probe = eve_amd.EVEStream(model, S, use_graph=False)
    v = torch.cat([probe.step(c, events=GazeEventSpec(fps=30, saccade_deg_s=1e9))['gaze_velocity'].clone() for c in chunks], dim=1)
    v = np.sort(v[torch.isfinite(v)].cpu().numpy().astype(np.float64))
    gaps = np.diff(v)
    i = len(v) // 4 + int(np.argmax(gaps[len(v) // 4:3 * len(v) // 4]))      # the widest gap around the median: clear of every velocity
    return {'model': model, 'chunks': chunks, 'spec': GazeEventSpec(fps=30, saccade_deg_s=float(0.5 * (v[i] + v[i + 1])))}


SACCADES = SaccadeSpec(min_amplitude_deg=0.0, max_duration_s=10.0)


def keep_out(out):
    return {k: v.clone() for k, v in out.items()}


def reference_steps(outs, chunks, spec, sspec, lengths=None, resets=None, capacity=256):
    """The steps' saccade outputs == the reference on the steps' OWN source PoG and origin, the state carried between them -> the
    reference's five buffers."""
    ecarried, carried = eref.fresh(S, 256), ref.fresh(S, capacity)
    for i, (out, chunk) in enumerate(zip(outs, chunks)):
        o = _mean2(chunk['left_o'], chunk['right_o']) if 'eye_valid' not in out else _fuse2(chunk['left_o'], chunk['right_o'], out['eye_valid'])
        valid = out['valid'].cpu().numpy() if 'eye_valid' in out else None
        ln = None if lengths is None else np.asarray(lengths[i], dtype=np.int32)
        rs = None if resets is None or resets[i] is None else np.asarray(resets[i], dtype=np.int32)
        elog, log = eref.new_log(), ref.new_log()
        pog = out['PoG_px_final'].cpu().numpy()
        ex = ref.events_ex(spec, pog, o.float().cpu().numpy(), chunk['inv_camera_transformation'].float().cpu().numpy(),
                           chunk['pixels_per_millimeter'].float().cpu().numpy(), *ecarried, valid=valid, lengths=ln, reset=rs, log=elog)
        want = ref.run(sspec, ex['sample'], ex['sample_time'], ex['gaze_vector'], ref.point_of(spec, pog, ex), ex['gaze_event'],
                       ex['gaze_velocity'], ex['fixation_id'], *carried, lengths=ln, reset=rs, log=log)
        assert eref.thresholds_clear(spec, elog) and ref.thresholds_clear(sspec, log) and elog['velocities']
        where = out['valid'].cpu().numpy() if 'valid' in out else np.ones((S, TC), dtype=bool)
        for k_ in SACCADE_KEYS:
            g = out[k_].cpu().numpy()
            assert g.dtype == want[k_].dtype and g[where].tobytes() == want[k_][where].tobytes(), (i, k_)
        assert out['gaze_event'].cpu().numpy()[where].tobytes() == ex['gaze_event'][where].tobytes()
    return carried


@pytest.mark.parametrize('mode', ['plain', 'lengths', 'eye_mask'])
def test_stream_saccades_eager_and_captured(rig, mode):
    model, chunks, spec = rig['model'], rig['chunks'], rig['spec']
    kw, lengths = {}, None
    if mode == 'lengths':
        lengths = [[5, 0, 4], [5, 3, 5]]
    elif mode == 'eye_mask':
        mask = torch.ones((S, TC, 2), dtype=torch.bool, device='cuda')
        mask[0, 1, 0] = mask[0, 3, 1] = mask[2, 2, 0] = mask[2, 2, 1] = False
        mask[1, :, 1] = False
        kw = dict(eye_mask=mask)
    eager_stream, graph_stream = eve_amd.EVEStream(model, S, use_graph=False), eve_amd.EVEStream(model, S)
    step = lambda s_, i: keep_out(s_.step(chunks[i], events=spec, saccades=SACCADES, **(kw if lengths is None else dict(lengths=lengths[i]))))
    eager = [step(eager_stream, 0), step(eager_stream, 1)]
    graph = [step(graph_stream, 0), step(graph_stream, 1)]
    assert len(graph_stream._graphs) == 1                 # the second step replayed the first one's graph
    for e, g in zip(eager, graph):
        assert sorted(e) == sorted(g) and not set(EX_KEYS) & set(e)      # the three _ex arrays stay internal
        where = e['valid'] if 'valid' in e else torch.ones((S, TC), dtype=torch.bool, device='cuda')
        for k_ in SACCADE_KEYS + GAZE_EVENT_KEYS:
            assert e[k_][where].cpu().numpy().tobytes() == g[k_][where].cpu().numpy().tobytes(), k_
    want = reference_steps(eager, chunks, spec, SACCADES, lengths=lengths)
    if mode == 'plain':
        assert want[3].sum() >= 1                         # (the clip does hold a completed saccade)
    for s_ in (eager_stream, graph_stream):               # (the capture's warm-up steps moved nothing)
        assert_carried(s_._saccade_buffers(), want, device_events=True)
        rows = s_.saccades()
        assert [r.shape for r in rows] == [(int(c), 16) for c in want[3]]
        assert s_.saccade_counts()[0].tolist() == want[3].tolist() and torch.equal(s_.saccade_table(), s_._saccade_buffers().table)


def test_reset_mid_saccade_and_a_masked_step_give_the_reference_s_tallies(rig):
    model, chunks = rig['model'], rig['chunks']
    always = GazeEventSpec(fps=30, saccade_deg_s=1e-9)    # every chained frame is a saccade frame: one saccade per stream, never landing
    stream = eve_amd.EVEStream(model, S)
    first = keep_out(stream.step(chunks[0], events=always, saccades=SACCADES))
    assert first['saccade_id'].tolist() == [[-1, 0, 0, 0, 0]] * S and (stream.get_saccade_state()[:, ref.OPEN] == 1).all()
    assert np.allclose(first['saccade_ms'].cpu().numpy(), [[0, 1000 / 30.0, 2000 / 30.0, 3000 / 30.0, 4000 / 30.0]] * S)
    stream.reset([1])
    mask = torch.ones((S, TC, 2), dtype=torch.bool, device='cuda')
    mask[2, 1] = False
    second = keep_out(stream.step(chunks[1], events=always, saccades=SACCADES, eye_mask=mask))
    assert second['saccade_id'].tolist() == [[0] * 5, [-1, 1, 1, 1, 1], [0, -1, 0, 0, 0]]
    want = reference_steps([first, second], chunks, always, SACCADES, resets=[None, [0, 1, 0]])
    assert want[1][:, ref.ABORTED].tolist() == [0, 1, 0] and want[0][:, ref.MISSING].tolist() == [0, 0, 1] and want[0][:, ref.NEXT_ID].tolist() == [1, 2, 1]
    assert_carried(stream._saccade_buffers(), want, device_events=True)
    # a reset before a step without the stage reaches the row through one launch with no frames; an events-only step leaves it stale,
    # and the next saccades step starts every row afresh before it runs
    stream.reset([0])
    stream.step(chunks[0])
    assert stream.saccade_table()[:, ref.ABORTED].tolist() == [1, 1, 0] and stream.get_saccade_state()[:, ref.OPEN].tolist() == [0, 1, 1]
    stream.step(chunks[0], events=always)
    assert stream._saccades_stale
    third = stream.step(chunks[1], events=always, saccades=SACCADES)
    assert (third['saccade_id'] == -1).all() and stream.saccade_table()[:, ref.ABORTED].tolist() == [1, 2, 1] and not stream._saccades_stale
    assert stream.get_saccade_state()[:, ref.NEXT_ID].tolist() == [1, 2, 1] and not stream.get_saccade_state()[:, ref.OPEN].any()


def launches(stream, chunk, **kw):
    """One step -> (the result, the (wrapper, kernel) pair of every call of the kernels object that launched something)."""
    k = default_kernels()
    names = [n for n in dir(type(k)) if not n.startswith('_') and callable(getattr(type(k), n))]
    seen = []
    # (a wrapper that launches nothing reports the name before it: every run starts from the same one, a launch with no frames)
    z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device='cuda')
    k.gaze_events(None, None, None, None, RAW, z(1, 32), z(1, 1, 8), z(1, dtype=torch.int32), z(1, dtype=torch.int32))

    def wrap(name, fn):
        def run(*a, **kw_):
            r = fn(*a, **kw_)
            seen.append((name, k.lib.eve_last_kernel().decode()))
            return r
        return run
    try:
        for n in names:
            setattr(k, n, wrap(n, getattr(k, n)))
        out = keep_out(stream.step(chunk, **kw))
    finally:
        for n in names:
            delattr(k, n)
    return out, seen


def test_a_step_without_saccades_issues_the_events_step_s_launches(rig):
    model, chunks, spec = rig['model'], rig['chunks'], rig['spec']
    base, base_seen = launches(eve_amd.EVEStream(model, S, use_graph=False), chunks[0], events=spec)
    stream = eve_amd.EVEStream(model, S, use_graph=False)
    none, none_seen = launches(stream, chunks[0], events=spec, saccades=None)
    assert none_seen == base_seen and ('gaze_events', 'gaze_events_kernel') in base_seen and stream._saccades is None
    assert not any(n in ('gaze_events_ex', 'gaze_saccades') for n, _ in base_seen)
    assert sorted(none) == sorted(base) and all(none[k_].cpu().numpy().tobytes() == base[k_].cpu().numpy().tobytes() for k_ in base)
    full, full_seen = launches(eve_amd.EVEStream(model, S, use_graph=False), chunks[0], events=spec, saccades=SACCADES)
    i = base_seen.index(('gaze_events', 'gaze_events_kernel'))
    assert full_seen == base_seen[:i] + [('gaze_events_ex', 'gaze_events_kernel'), ('gaze_saccades', 'gaze_saccades_kernel')] + base_seen[i + 1:]
    assert sorted(full) == sorted(list(base) + list(SACCADE_KEYS)) and all(full[k_].cpu().numpy().tobytes() == base[k_].cpu().numpy().tobytes() for k_ in base)
    with pytest.raises(ValueError, match='events='):
        stream.step(chunks[0], saccades=SACCADES)
