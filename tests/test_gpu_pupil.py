"""GPU: eve_pupil_track against the numpy contract of tests/pupil_ref.py, and EVEStream's step(pupil=...) around it (eager and
captured).  Every test here needs the entry point, PupilSpec or the pupil argument, so every one fails without them.

Every comparison with the reference is exact equality -- integers, and the bits of every float, NaNs at the reference's places:
nothing but + - * /, fabs and comparisons of doubles leads to any of them."""
import numpy as np
import pytest
import torch

import eve_amd
import eye_gate_ref
import pupil_ref as ref
from eve_amd import data
from eve_amd.data import BlinkSpec, EyeGateSpec, PupilSpec
from eve_amd.kernels import default_kernels
from test_gpu_calibration import cuda, guarded, guards_hold
from test_gpu_face_pose import CAM, face_chunks, rest_of_clip
from test_gpu_stream import gpu_clip, make_model

pytestmark = pytest.mark.gpu
KEYS = ref.KEYS
FLOATS = KEYS[:5]
CARRIED = ('state', 'table', 'light', 'store', 'count', 'dropped')
FRAME_INPUTS = ('eye_valid', 'frame_time', 'luminance', 'baseline_mark')
SPEC = ref.Spec(fps=30.0, min_mm=2.0, max_mm=8.0, max_speed_mm_s=6.0, max_gap_s=0.12, offset_rate=0.2, cutoff_hz=4.0, light_tau_s=0.3,
                baseline_tau_s=1.5, dilate_mm_s=0.4, constrict_mm_s=0.5, min_amplitude_mm=0.02)


def scene(B, T, seed=11, rich=True):
    """Sizes that wander around 4 mm with an inter-eye difference, at 30 Hz.  rich: withheld eyes with garbage and NaN behind them,
    spikes (speed), values out of range, NaN sizes at delivered eyes, gaps above max_gap_s, a NaN and an infinite time, a stall and a
    step backwards, a luminance with NaNs, marks in runs."""
    rng = np.random.RandomState(seed)
    c = 4.0 + np.cumsum(rng.normal(0, 0.03, (B, T)), axis=1) + 0.6 * np.sin(np.arange(T) / 7.0)[None]
    left, right = (c + 0.15 + rng.normal(0, 0.01, (B, T))).astype(np.float32), (c - 0.15 + rng.normal(0, 0.01, (B, T))).astype(np.float32)
    ev = np.ones((B, T, 2), np.uint8)
    dt = np.full((B, T), 1 / 30.0)
    if rich:
        dt = rng.uniform(0.030, 0.036, (B, T))
        dt[rng.rand(B, T) < 0.04] = 0.5
    tt = np.cumsum(dt, axis=1) + 50.0 * np.arange(B)[:, None]
    lum = (40.0 + 15.0 * np.sin(np.arange(T) / 11.0)[None] + rng.normal(0, 1.0, (B, T))).astype(np.float32)
    marks = np.zeros((B, T), np.uint8)
    marks[:, 1:1 + max(T // 8, 1)] = 1
    marks[:, T // 2:T // 2 + 3] = 1
    if rich:
        left[rng.rand(B, T) < 0.05] += 1.0
        right[rng.rand(B, T) < 0.04] = 11.0
        right[rng.rand(B, T) < 0.02] = 0.5
        left[rng.rand(B, T) < 0.06] = np.nan
        ev = (rng.rand(B, T, 2) > 0.15).astype(np.uint8)
        if T > 30:
            ev[0, 20:27] = 0
        for e, side in enumerate((left, right)):
            hidden = ev[..., e] == 0
            side[hidden] = np.resize(np.float32([np.nan, 1e30, -3.0, np.inf, 4.0]), hidden.sum())
        lum[rng.rand(B, T) < 0.06] = np.nan
        if T > 12:
            tt[0, 5], tt[0, 9], tt[0, 11] = np.nan, np.inf, tt[0, 10]
            tt[B - 1, 7] = tt[B - 1, 6] - 2.0
    return dict(left=left, right=right, eye_valid=ev, frame_time=tt, luminance=lum, baseline_mark=marks)


def cut_of(sc, t0, t1, use):
    return {k: sc[k][:, t0:t1] for k in use if sc.get(k) is not None}


def ref_run(spec, sc, buffers, t0=0, t1=None, use=FRAME_INPUTS, **kw):
    return ref.run(spec, sc['left'][:, t0:t1], sc['right'][:, t0:t1], *buffers, **dict(cut_of(sc, t0, t1, use), **kw))


def device_buffers(buffers):
    return [cuda(a) for a in buffers]


def device_run(spec, sc, buffers, t0=0, t1=None, use=FRAME_INPUTS, **kw):
    """The wrapper on the device copies of the scene's frames t0 .. t1; buffers: device tensors, updated in place."""
    size = cuda(np.stack([sc['left'][:, t0:t1], sc['right'][:, t0:t1]]))
    return default_kernels().pupil_track(size, spec, *buffers, **dict({k: cuda(v) for k, v in cut_of(sc, t0, t1, use).items()},
                                                                      **{k: cuda(np.asarray(v, np.int32)) for k, v in kw.items()}))


def assert_same(got, want, buffers, want_buffers):
    for k in KEYS:
        g = got[k].cpu().numpy()
        assert g.dtype == want[k].dtype and g.shape == want[k].shape and g.tobytes() == want[k].tobytes(), k
    for name, g, w in zip(CARRIED, buffers, want_buffers):
        assert g.cpu().numpy().dtype == w.dtype and g.cpu().numpy().tobytes() == w.tobytes(), name


OUT_SHAPES = lambda B, T: {k: ((B, T, 2) if k.startswith('eye_') else (B, T), torch.float32 if k in FLOATS else torch.uint8) for k in KEYS}


def raw_call(spec, B, T, size, buffers, outs, eye_valid=None, frame_time=None, lengths=None, reset=None, flush=None, luminance=None,
             baseline_mark=None, capacity=None, **over):
    """The C entry point itself, so that everything can lie between guards and bad arguments reach the library."""
    k = default_kernels()
    p = k._p
    state, table, light, store, count, dropped = buffers
    s = dict(fps=0.0 if spec.fps is None else spec.fps, min_mm=spec.min_mm, max_mm=spec.max_mm, max_speed_mm_s=spec.max_speed_mm_s,
             max_gap_s=spec.max_gap_s, offset_rate=spec.offset_rate, cutoff_hz=spec.cutoff_hz, light_tau_s=spec.light_tau_s,
             baseline_tau_s=0.0 if spec.baseline_tau_s is None else spec.baseline_tau_s, dilate_mm_s=spec.dilate_mm_s,
             constrict_mm_s=spec.constrict_mm_s, min_amplitude_mm=spec.min_amplitude_mm)
    s.update(over)
    k._ck(k.lib.eve_pupil_track(B, T, p(size), p(eye_valid), p(frame_time), p(lengths), p(reset), p(flush), p(luminance), p(baseline_mark),
                                *[float(s[f]) for f in ('fps', 'min_mm', 'max_mm', 'max_speed_mm_s', 'max_gap_s', 'offset_rate', 'cutoff_hz', 'light_tau_s',
                                                        'baseline_tau_s', 'dilate_mm_s', 'constrict_mm_s', 'min_amplitude_mm')],
                                p(state), p(table), p(light), (capacity if capacity is not None else 2 if store is None else store.shape[1]), p(store),
                                p(count), p(dropped), *[None if outs is None else p(outs[k_]) for k_ in KEYS], k._stream()))
    assert k.lib.eve_last_kernel().decode() == 'pupil_track_kernel'


# ---------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize('B, T, lengths', [(1, 1, None), (3, 5, [5, 0, 3]), (2, 64, None), (2, 65, None), (2, 130, [130, 97])])
def test_the_kernel_equals_the_reference_at_the_pass_boundaries(B, T, lengths):
    sc = scene(B, T, seed=T)
    kw = {} if lengths is None else dict(lengths=np.array(lengths, np.int32))
    want_buffers, buffers = ref.fresh(B, 16), device_buffers(ref.fresh(B, 16))
    want = ref_run(SPEC, sc, want_buffers, flush=np.ones(B, np.int32), **kw)
    assert T < 64 or (want['valid'].sum() > B * T // 3 and want_buffers[4].sum() >= 2)
    assert_same(device_run(SPEC, sc, buffers, flush=[1] * B, **kw), want, buffers, want_buffers)


def test_every_kind_of_frame_in_one_launch():
    """Three streams arrive with state from an earlier call of 20 plain frames (an open episode among them).  lengths (100, 100, 0);
    stream 1 is reset mid-sequence of calls (its open episode goes to the store, its row starts afresh, the episode counter runs on),
    stream 0 is flushed and has a light response, stream 2 gets no frame and keeps its row.  Every buffer lies between guards."""
    B, T, V = 3, 100, 24
    sc = scene(B, T, seed=5)
    sc['frame_time'][1, 40] = sc['frame_time'][1, 39] - 2.0              # a step backwards in a stream that gets frames
    want_buffers = ref.fresh(B, V)
    want_buffers[2][0] = (1.0, -0.02, 40.0, 0.0)
    pre = scene(B, 20, seed=6, rich=False)
    pre['frame_time'] = pre['frame_time'] - 1.0
    ref_run(SPEC, pre, want_buffers)
    assert (want_buffers[0][:, ref.HAS_PREV] == 1).all() and want_buffers[0][:, ref.EP_OPEN].sum() >= 1
    want_buffers[0][1, ref.EP_OPEN], want_buffers[0][1, ref.EP_D_START] = 1.0, want_buffers[0][1, ref.EP_D_END] - 1.0      # (whatever it was: one is open now)
    want_buffers[0][1, ref.EP_PHASE] = 1.0
    lengths, reset, flush = (np.array(a, np.int32) for a in ([100, 100, 0], [0, 1, 0], [1, 0, 0]))
    sentinels = {'state': -777.25, 'table': -777.25, 'light': -777.25, 'store': -777.25, 'count': -7, 'dropped': -7}
    wholes, buffers = {}, []
    for name, a in zip(CARRIED, want_buffers):
        wholes[name], payload = guarded(a.shape, torch.from_numpy(a).dtype, sentinels[name])
        payload.copy_(cuda(a))
        buffers.append(payload)
    outs = {}
    for k, (shape, dtype) in OUT_SHAPES(B, T).items():
        wholes[k], outs[k] = guarded(shape, dtype, 99)
        sentinels[k] = 99
    before = [a.copy() for a in want_buffers]
    want = ref_run(SPEC, sc, want_buffers, lengths=lengths, reset=reset, flush=flush)
    state, table, light, store, count, dropped = want_buffers
    # what the case is meant to hold, asserted on the reference alone
    reasons = want['eye_reason'][:2].reshape(-1)
    assert all((reasons == r).sum() >= 2 for r in (ref.WITHHELD, ref.NOT_FINITE, ref.RANGE, ref.SPEED))
    assert want['valid'][0, [5, 9]].tolist() == [0, 0] and (want['eye_reason'][0, [5, 9]] == 0).all() and (want['valid'][2] == 0).all()
    assert want['valid'][0, 10:12].sum() <= 1 and want['valid'][1, 40] == 0 and (want['eye_reason'][1, 40] == 0).all()      # the stall and the step backwards
    assert want['valid'][:2].sum() > 100 and np.isnan(want['velocity'][:2][want['valid'][:2] == 1]).sum() >= 4      # restarts after the gaps
    assert count[1] >= before[4][1] + 1 and state[1, ref.TICKS] == 100 and state[2].tobytes() == before[0][2].tobytes() and state[0, ref.EP_OPEN] == 0
    assert table[0, ref.N] > 50 and table[0, ref.LOST] > 0 and (want['eye_used'][:2].sum(axis=2) == 1).sum() > 20 and set(want['event'].reshape(-1)) == {0, 1, 2}
    assert np.isfinite(want['change_pct'][:2]).sum() > 100 and not (want['mm'][0] == want['raw_mm'][0]).all()
    raw_call(SPEC, B, T, cuda(np.stack([sc['left'], sc['right']])), buffers, outs, *[cuda(sc[k]) for k in ('eye_valid', 'frame_time')], cuda(lengths),
             cuda(reset), cuda(flush), cuda(sc['luminance']), cuda(sc['baseline_mark']))
    torch.cuda.synchronize()
    assert_same(outs, want, buffers, want_buffers)
    for name, whole in wholes.items():
        assert guards_hold(whole, sentinels[name]), name


@pytest.mark.parametrize('combo', range(16))
def test_every_combination_of_the_optional_inputs(combo):
    use = tuple(k for i, k in enumerate(FRAME_INPUTS) if combo >> i & 1)
    B, T = 2, 70
    sc = scene(B, T, seed=20)
    want_buffers, buffers = ref.fresh(B, 16), device_buffers(ref.fresh(B, 16))
    want = ref_run(SPEC, sc, want_buffers, use=use, flush=np.ones(B, np.int32))
    assert want['valid'].sum() > 40 and ('baseline_mark' in use or (np.isfinite(want['change_mm']) == (want['valid'] == 1)).all())
    assert_same(device_run(SPEC, sc, buffers, use=use, flush=[1] * B), want, buffers, want_buffers)
    # ... and with neither marks nor a follower the changes are NaN
    if 'baseline_mark' not in use:
        bare = ref.Spec(**dict(SPEC.__dict__, baseline_tau_s=None))
        want_buffers, buffers = ref.fresh(B, 16), device_buffers(ref.fresh(B, 16))
        want = ref_run(bare, sc, want_buffers, use=use)
        assert np.isnan(want['change_mm']).all()
        assert_same(device_run(bare, sc, buffers, use=use), want, buffers, want_buffers)


def test_a_full_store_drops_and_counts():
    B, T = 2, 130
    sc = scene(B, T, seed=31)
    want_buffers, buffers = ref.fresh(B, 1), device_buffers(ref.fresh(B, 1))
    want = ref_run(SPEC, sc, want_buffers, flush=np.ones(B, np.int32))
    assert want_buffers[4].tolist() == [1, 1] and want_buffers[5].min() >= 2
    assert_same(device_run(SPEC, sc, buffers, flush=[1, 1]), want, buffers, want_buffers)
    roomy = ref.fresh(B, 64)
    ref_run(SPEC, sc, roomy, flush=np.ones(B, np.int32))
    assert (roomy[4] == want_buffers[4] + want_buffers[5]).all() and buffers[1].cpu().numpy().tobytes() == roomy[1].tobytes()
    assert buffers[3].cpu().numpy()[:, 0].tobytes() == roomy[3][:, 0].tobytes() and buffers[0].cpu().numpy().tobytes() == roomy[0].tobytes()


def test_chunks_equal_one_pass_on_the_device():
    B, T = 2, 130
    sc = scene(B, T, seed=41)
    lengths = np.array([130, 97])
    for use, spec in ((FRAME_INPUTS, SPEC), (('eye_valid', 'luminance'), SPEC)):      # explicit times, and the counted clock
        want_buffers = ref.fresh(B, 32)
        want = ref_run(spec, sc, want_buffers, use=use, lengths=lengths, flush=np.ones(B, np.int32))
        whole = device_buffers(ref.fresh(B, 32))
        assert_same(device_run(spec, sc, whole, use=use, lengths=lengths, flush=[1, 1]), want, whole, want_buffers)
        parts, outs, t0 = device_buffers(ref.fresh(B, 32)), [], 0
        for n in (1, 64, 65):
            more = dict(flush=[1, 1]) if t0 + n == T else {}
            outs.append(device_run(spec, sc, parts, t0, t0 + n, use=use, lengths=np.clip(lengths - t0, 0, n), **more))
            t0 += n
        assert_same({k: torch.cat([o[k] for o in outs], dim=1) for k in KEYS}, want, parts, want_buffers)
        assert want_buffers[0][:, ref.TICKS].tolist() == [130, 97] and want_buffers[4].min() >= 3


def test_the_stand_alone_call_is_the_kernel_call():
    B, T = 3, 70
    sc = scene(B, T, seed=51)
    spec = PupilSpec('size', **{k: v for k, v in SPEC.__dict__.items() if k != 'fps'})
    buffers = device_buffers(ref.fresh(B, 256))
    light = np.zeros((B, 4))
    light[1] = (1.0, 0.01, 40.0, 0.0)
    buffers[2].copy_(cuda(light))
    want = device_run(spec, sc, buffers, flush=[1] * B)
    got = data.pupil_track(spec, cuda(sc['left']), cuda(sc['right']), eye_valid=cuda(sc['eye_valid']) != 0, frame_time=cuda(sc['frame_time']),
                           luminance=cuda(sc['luminance']), baseline_mark=cuda(sc['baseline_mark']), light=cuda(light))
    assert sorted(got) == sorted(['size_' + k for k in KEYS] + ['table', 'episodes', 'episode_count', 'episode_dropped', 'light', 'state'])
    for k in KEYS:
        assert got['size_' + k].cpu().numpy().tobytes() == want[k].cpu().numpy().tobytes(), k
    for k, b_ in zip(('state', 'table', 'light', 'episodes', 'episode_count', 'episode_dropped'), buffers):
        assert got[k].cpu().numpy().tobytes() == b_.cpu().numpy().tobytes(), k
    assert int(got['episode_count'].min()) >= 2 and not got['state'][:, ref.EP_OPEN].any()
    with pytest.raises(ValueError, match='fps'):
        data.pupil_track(spec, cuda(sc['left']), cuda(sc['right']))
    with pytest.raises(TypeError, match='right'):
        data.pupil_track(spec, cuda(sc['left']), cuda(sc['right'][:, :5]), frame_time=cuda(sc['frame_time']))
    with pytest.raises(TypeError, match='frame_time'):
        data.pupil_track(spec, cuda(sc['left']), cuda(sc['right']), frame_time=torch.zeros((B, T), device='cuda'))
    with pytest.raises(TypeError, match='luminance'):
        data.pupil_track(spec, cuda(sc['left']), cuda(sc['right']), frame_time=cuda(sc['frame_time']), luminance=cuda(sc['luminance']).double())


def test_the_library_refuses_without_a_launch():
    k = default_kernels()
    B, T = 1, 2
    z = lambda *s, dtype=torch.float32: torch.zeros(s, dtype=dtype, device='cuda')
    buffers = device_buffers(ref.fresh(B, 2))
    buffers[0][0, ref.EP_COUNT] = 5.0
    outs = {k_: z(*shape, dtype=d) for k_, (shape, d) in OUT_SHAPES(B, T).items()}
    size = z(2, B, T)
    # a launch of another kernel first: eve_last_kernel must still name IT after every refusal
    k.gaze_aoi(None, None, SPEC, *data.aoi_buffers(1, 1, 1, 'cuda'))
    last = k.lib.eve_last_kernel().decode()
    assert last and last != 'pupil_track_kernel'
    call = lambda B_=B, T_=T, size_=size, buffers_=buffers, outs_=outs, **kw: raw_call(SPEC, B_, T_, size_, buffers_, outs_, **kw)
    without = lambda i: [None if j == i else t for j, t in enumerate(buffers)]
    bad = [dict(buffers_=without(i)) for i in range(6)]                                     # null carried buffers
    bad += [dict(B_=0), dict(T_=-1), dict(capacity=0), dict(size_=None)] + [dict(outs_=dict(outs, **{k_: None})) for k_ in KEYS]
    bad += [dict(B_=2 ** 31 // 16), dict(T_=2 ** 30), dict(capacity=2 ** 29)]               # index products past 31 bits
    bad += [dict(min_mm=8.0), dict(min_mm=9.0), dict(offset_rate=0.0), dict(offset_rate=1.0625), dict(offset_rate=float('nan'))]
    for field in ('min_mm', 'max_mm', 'max_speed_mm_s', 'max_gap_s', 'cutoff_hz', 'light_tau_s', 'dilate_mm_s', 'constrict_mm_s', 'fps'):
        bad += [{field: v} for v in (0.0, -1.0, float('nan'), float('inf'))]                # (fps: no frame_time, so it counts)
    for field in ('baseline_tau_s', 'min_amplitude_mm'):
        bad += [{field: v} for v in (-1.0, float('nan'), float('inf'))]
    for kw in bad:
        with pytest.raises(RuntimeError, match='pupil_track'):
            call(**kw)
        assert k.lib.eve_last_kernel().decode() == last, kw
    with pytest.raises(TypeError, match='state'):
        k.pupil_track(size, SPEC, buffers[0].float(), *buffers[1:])
    with pytest.raises(TypeError, match='size'):
        k.pupil_track(z(B, T), SPEC, *buffers)
    with pytest.raises(TypeError, match='luminance'):
        k.pupil_track(size, SPEC, *buffers, luminance=z(B, T + 1))
    with pytest.raises(TypeError, match='no frame inputs'):
        k.pupil_track(None, SPEC, *buffers, luminance=z(B, T))
    torch.cuda.synchronize()
    want = ref.fresh(B, 2)
    want[0][0, ref.EP_COUNT] = 5.0
    for g, w in zip(buffers, want):
        assert g.cpu().numpy().tobytes() == w.tobytes()
    # with frame_time a bad fps does not matter; T = 0 needs no frame pointer and only resets and flushes
    call(fps=0.0, frame_time=z(B, T, dtype=torch.float64))
    raw_call(SPEC, B, 0, None, buffers, None, reset=cuda(np.ones(B, np.int32)))
    torch.cuda.synchronize()
    assert buffers[0].cpu().numpy()[0].tolist() == [0.0] * ref.EP_COUNT + [5.0]


# ---------------------------------------------------------------------------------------------------------------- EVEStream
S, TC = 3, 5


def spec_around(p, fps=30.0):
    """A PupilSpec laid around the pupil sizes p [S, T, 2] of a probe stream (an untrained EyeNet's head ends in a ReLU, so nothing
    physiological may be assumed): the range leaves out the sizes below their 12th and above their 88th percentile, the speed bound is
    the 70th percentile of the frame-to-frame speeds -- so that the trace has range rejects, speed rejects and samples."""
    v = np.unique(p[np.isfinite(p)])
    assert len(v) >= 8, 'the probe gives too few distinct pupil sizes: %r' % (v,)
    lo, hi = float(np.percentile(v, 12)), float(np.percentile(v, 88))
    speeds = np.abs(np.diff(p, axis=1)).reshape(-1) * fps
    bound = float(np.percentile(speeds[np.isfinite(speeds) & (speeds > 0)], 70))
    return PupilSpec(fps=fps, min_mm=lo, max_mm=hi, max_speed_mm_s=bound, max_gap_s=0.1, offset_rate=0.25, cutoff_hz=4.0, baseline_tau_s=0.5,
                     dilate_mm_s=bound / 50, constrict_mm_s=bound / 50, min_amplitude_mm=0.0)


def probe_sizes(model, chunks, **kw):
    probe = eve_amd.EVEStream(model, S, use_graph=False)
    outs = [probe.step(c, **kw) for c in chunks]
    return torch.cat([torch.stack([o['left_pupil_size'], o['right_pupil_size']], dim=-1).clone() for o in outs], dim=1).double().cpu().numpy()


@pytest.fixture(scope='module')
def rig():
    """One model, one 3 x 10 clip, a luminance and baseline marks, and a spec laid around the clip's own pupil sizes, shared and never
    modified."""
    model, _ = make_model(refine_net_rnn_type='CGRU')
    _, d, _ = gpu_clip(S, 2 * TC, seed=7)
    rng = np.random.RandomState(3)
    d = dict(d, pupil_luminance=cuda(rng.uniform(20, 60, (S, 2 * TC)).astype(np.float32)), pupil_baseline=cuda((np.arange(2 * TC)[None].repeat(S, 0) % 4 < 2)))
    chunk = lambda t0, t1: {k: v[:, t0:t1].contiguous() for k, v in d.items()}
    chunks = (chunk(0, TC), chunk(TC, 2 * TC))
    p = probe_sizes(model, [{k: v for k, v in c.items() if not k.startswith('pupil_')} for c in chunks])
    print('probe pupil sizes', p.min(), p.max(), np.unique(p).size)
    return {'model': model, 'chunks': chunks, 'spec': spec_around(p)}


def keep(out):
    return {k: v.clone() for k, v in out.items()}


def specified(a, out):
    return a[out['valid']] if 'valid' in out and tuple(a.shape[:2]) == tuple(out['valid'].shape) else a


def stream_buffers(stream, name='pupil'):
    st = stream.get_pupil_state()[name]
    return [st[k] for k in ('state', 'table', 'light', 'episodes', 'count', 'dropped')]


def reference_on(outs, chunks, spec, lengths=None, name='pupil', capacity=256):
    """The reference on the steps' OWN pupil sizes and eye_valid, the buffers carried between the steps.  -> (buffers, the reference's
    outputs per step and the delivered frames)."""
    n = lambda t: t.cpu().numpy()
    buffers, wants = ref.fresh(S, capacity), []
    for i, (out, chunk) in enumerate(zip(outs, chunks)):
        want = ref.run(spec, n(out['left_pupil_size'].float()), n(out['right_pupil_size'].float()), *buffers,
                       eye_valid=n(out['eye_valid']).astype(np.uint8) if 'eye_valid' in out else None,
                       lengths=None if lengths is None else np.asarray(lengths[i]), luminance=n(chunk['pupil_luminance']) if 'pupil_luminance' in chunk else None,
                       baseline_mark=n(chunk['pupil_baseline']).astype(np.uint8) if 'pupil_baseline' in chunk else None)
        live = np.ones((S, TC), bool) if lengths is None else np.arange(TC)[None, :] < np.asarray(lengths[i])[:, None]
        wants.append((want, live))
    return buffers, wants


def outputs_match(outs, wants, name='pupil'):
    for i, (out, (want, live)) in enumerate(zip(outs, wants)):
        for k in KEYS:
            g = out['%s_%s' % (name, k)].cpu().numpy()
            assert g.dtype == want[k].dtype and g[live].tobytes() == want[k][live].tobytes(), (i, k)


def rig_conditions(wants):
    """The three conditions every stream case asserts on the reference's result before it compares anything."""
    valid = np.concatenate([w['valid'][live] for w, live in wants])
    reasons = np.concatenate([w['eye_reason'][live].reshape(-1) for w, live in wants])
    print('samples %d of %d, range rejects %d, speed rejects %d' % (valid.sum(), valid.size, (reasons == ref.RANGE).sum(), (reasons == ref.SPEED).sum()))
    assert 2 * valid.sum() >= valid.size                  # at least half of the delivered frames are samples
    assert (reasons == ref.RANGE).sum() >= 1 and (reasons == ref.SPEED).sum() >= 1


@pytest.mark.parametrize('mode', ['lengths', 'eye_mask'])
def test_stream_pupil_eager_and_captured(rig, mode):
    model, chunks, spec = rig['model'], rig['chunks'], rig['spec']
    if mode == 'lengths':
        kw = dict(lengths=[[5, 0, 4], [5, 3, 5]])
    else:
        mask = torch.ones((S, TC, 2), dtype=torch.bool, device='cuda')
        mask[0, 1, 0] = mask[0, 3, 1] = mask[2, 2, 0] = mask[2, 2, 1] = False
        mask[1, 1:3, 1] = False
        kw = dict(eye_mask=mask)
    at = lambda i: {k: (v[i] if k == 'lengths' else v) for k, v in kw.items()}
    eager_stream, graph_stream = eve_amd.EVEStream(model, S, use_graph=False), eve_amd.EVEStream(model, S)
    first_eager = keep(eager_stream.step(chunks[0], pupil=spec, **at(0)))
    first_graph = keep(graph_stream.step(chunks[0], pupil=spec, **at(0)))
    # the carried buffers after the FIRST captured step of a shape: the capture's two warm-up steps were put back (_carried())
    for e, g in zip(stream_buffers(eager_stream), stream_buffers(graph_stream)):
        assert e.cpu().numpy().tobytes() == g.cpu().numpy().tobytes()
    eager = [first_eager, keep(eager_stream.step(chunks[1], pupil=spec, **at(1)))]
    graph = [first_graph, keep(graph_stream.step(chunks[1], pupil=spec, **at(1)))]
    for e, g in zip(eager, graph):
        assert sorted(e) == sorted(g)
        for k in e:
            assert specified(e[k], e).cpu().numpy().tobytes() == specified(g[k], e).cpu().numpy().tobytes(), k
    assert len(graph_stream._graphs) == 1                                # the second step replayed the first one's graph
    buffers, wants = reference_on(eager, chunks, spec, lengths=kw.get('lengths'))
    rig_conditions(wants)
    outputs_match(eager, wants)
    outputs_match(graph, wants)
    for s_ in (eager_stream, graph_stream):
        for name, g, w in zip(CARRIED, stream_buffers(s_), buffers):
            assert g.cpu().numpy().tobytes() == w.tobytes(), name
    assert buffers[0][:, ref.TICKS].tolist() == ([10, 3, 9] if mode == 'lengths' else [10, 10, 10]) and buffers[1][:, ref.N].sum() >= 14
    if mode == 'eye_mask':
        assert eager[0]['pupil_eye_reason'][0, 1].tolist()[0] == ref.WITHHELD and eager[0]['pupil_eye_reason'][2, 2].tolist() == [1, 1]
        assert not eager[0]['pupil_valid'][2, 2] and (eager[0]['pupil_eye_reason'][1, 1:3, 1] == 1).all()
    # without pupil= the same EVEStream returns the plain step's bits and leaves the table alone
    plain = keep(eve_amd.EVEStream(model, S).step(chunks[0], **at(0)))
    graph_stream.reset()
    back = graph_stream.step(chunks[0], **at(0))
    assert sorted(back) == sorted(plain) and not [k for k in back if k.startswith('pupil_')]
    for k in plain:
        assert specified(back[k], plain).cpu().numpy().tobytes() == specified(plain[k], plain).cpu().numpy().tobytes(), k
    assert graph_stream.pupil_table().cpu().numpy().tobytes() == buffers[1].tobytes()


def test_stream_gate_and_pupil_withhold_the_gated_eyes():
    """The eye gate's rig (a face-landmark clip whose eyes close and whose head turns): the eyes the gate vetoes -- a blink and its
    hold-off among them -- are the ones this stage withholds."""
    B = 3
    model, _ = make_model(refine_net_rnn_type='CGRU')
    model.eye_net.face_huber_px = 0.25
    rest = rest_of_clip(B, 2 * TC, seed=7)
    frames = torch.randint(0, 256, (B, 2 * TC) + CAM + (3,), generator=torch.Generator().manual_seed(8), dtype=torch.uint8).cuda()
    lm, face_rig = face_chunks(B, 2 * TC, seed=9, invalid=[(0, 3)])
    contours = np.concatenate([eye_gate_ref.eyelid_trace(2 * TC, c, seed=20 + b, C=3)[0] for b, c in enumerate(([(1, 2)], [], [(4, 3)]))])
    contours[0, 1:3, 1] = contours[0, 0, 1]
    d = dict(rest, camera_frame=frames, face_landmarks=lm, eye_contours=cuda(contours))
    chunks = [dict({k: v[:, t0:t1].contiguous() for k, v in d.items()}, face_rig=face_rig) for t0, t1 in ((0, TC), (TC, 2 * TC))]
    gate = EyeGateSpec(blink=BlinkSpec(hold_frames=1, max_closed_frames=20))
    probe = eve_amd.EVEStream(model, B, use_graph=False)
    outs = [keep(probe.step(c, gate=gate)) for c in chunks]
    usable = torch.cat([o['eye_valid'] for o in outs], dim=1).cpu().numpy()
    p = torch.cat([torch.stack([o['left_pupil_size'], o['right_pupil_size']], dim=-1) for o in outs], dim=1).double().cpu().numpy()
    assert (~usable).sum() >= 4 and usable.sum() >= 30
    spec = spec_around(np.where(usable, p, np.nan)[:, :, :])
    eager_stream, graph_stream = eve_amd.EVEStream(model, B, use_graph=False), eve_amd.EVEStream(model, B)
    eager = [keep(eager_stream.step(c, gate=gate, pupil=spec)) for c in chunks]
    graph = [keep(graph_stream.step(c, gate=gate, pupil=spec)) for c in chunks]
    buffers, wants = reference_on(eager, chunks, spec)
    rig_conditions(wants)
    outputs_match(eager, wants)
    outputs_match(graph, wants)
    for s_ in (eager_stream, graph_stream):
        for name, g, w in zip(CARRIED, stream_buffers(s_), buffers):
            assert g.cpu().numpy().tobytes() == w.tobytes(), name
    for out in eager:
        withheld = (out['pupil_eye_reason'] == ref.WITHHELD).cpu().numpy()
        assert np.array_equal(withheld, ~out['eye_valid'].cpu().numpy()) and not (out['pupil_eye_used'].bool() & ~out['eye_valid']).any()
        assert np.array_equal((out['blink'] != 0).cpu().numpy() & withheld, (out['blink'] != 0).cpu().numpy())      # a blinking eye is withheld
    assert sum(int((o['blink'] != 0).sum()) for o in eager) >= 2 and sum(int(o['pupil_valid'].sum()) for o in eager) >= 10
