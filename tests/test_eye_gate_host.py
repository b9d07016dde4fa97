"""CPU: the eye gate -- the numpy contract (tests/eye_gate_ref.py) on a synthetic eyelid trace, under chunk splits and on the coverage
lattice, eve_amd.EyeGateSpec / BlinkSpec, and the EVEStream plumbing (step(gate=...), the refusals, the graph key, reset, the blink
store) over a stand-in whose eye_gate is the reference itself.  The GPU suite (test_gpu_eye_gate.py) checks the HIP kernel."""
import numpy as np
import pytest
import torch

import eve_amd
import eye_gate_ref as ref
from eve_amd import kernels
from eve_amd.data import EYE_GATE_KEYS, BlinkSpec, EyeGateSpec, GazeEventSpec
from test_calibration_host import CalibFakes
from test_gaze_events_host import EventFakes
from test_stream_host import chunk_of, clip, make_model

BLINK = BlinkSpec(hold_frames=2, max_closed_frames=20)
P = ref.params_of(EyeGateSpec(blink=BLINK))


# ---------------------------------------------------------------------------------------------------------------- the eyelid trace
CLOSURES = [(0, 3), (40, 6), (80, 12)]                   # (first frame, frames): the first one starts on the trace's first frame


def walk(contours, capacity=8, **kw):
    T = contours.shape[1]
    carried = ref.fresh(1, capacity)
    return (ref.run(P, 1, T, *carried, contours=contours, **kw),) + carried


def test_the_trace_gives_the_closures_that_do_not_start_on_frame_zero():
    contours, ear = ref.eyelid_trace(120, CLOSURES)
    out, state, store, count, dropped = walk(contours)
    assert count[0] == 4 and dropped[0] == 0               # two closures, two eyes: the one the trace opens with is no blink
    rows = store[0, :4]
    assert rows[:, 0].tolist() == [0, 1, 0, 1] and rows[:, 1].tolist() == [40, 40, 80, 80] and rows[:, 2].tolist() == [45, 45, 91, 91]
    assert (rows[:, 3] < 0.3).all() and (rows[:, 3] > 0.1).all()          # 0.05 .. 0.06 over a baseline near 0.3
    for e in range(2):
        r = out['reason'][0, :, e]
        # the baseline recovers from the first frame's closed eye: frames 0 .. 2 count as open, and the real closures are seen
        assert not r[:40].any() and state[0, e, ref.BASE] > 0.28
        assert (r[40:46] == ref.R_CLOSED).all() and (r[80:92] == ref.R_CLOSED).all()
        # hold_frames frames from the reopening one on are withheld, and nothing else
        assert (r[46:48] == ref.R_HOLD).all() and (r[92:94] == ref.R_HOLD).all() and not r[48:80].any() and not r[94:].any()
        assert np.array_equal(out['blink'][0, :, e], (r == ref.R_CLOSED).astype(np.uint8))
        assert np.array_equal(out['usable'][0, :, e], (r == 0).astype(np.uint8))
        # ten open frames after the closed start the baseline's gap of 0.25 has halved ten times (baseline_rise 0.5); from then on the
        # baseline lies inside the noise band 0.29 .. 0.31 and so does the ratio: within 0.31 / 0.29 - 1 < 0.1 of 1
        open_frames = np.flatnonzero(r == 0)
        assert np.abs(out['openness'][0, open_frames[open_frames >= 13], e] - 1.0).max() < 0.1
    assert state[0, 0, ref.TICK] == 120 and (state[0, :, ref.CLOSED] == 0).all()


def test_a_full_store_drops_and_counts():
    contours, _ = ref.eyelid_trace(120, CLOSURES)
    _, _, store, count, dropped = walk(contours, capacity=1)
    assert count[0] == 1 and dropped[0] == 3 and store[0, 0].tolist()[:3] == [0, 40, 45]


def test_stuck_closed_rebaselines_and_stores_nothing():
    contours, _ = ref.eyelid_trace(80, [(10, 40)])
    out, state, store, count, dropped = walk(contours)
    r = out['reason'][0, :, 0]
    assert count[0] == 0 and dropped[0] == 0
    assert (r[10:30] == ref.R_CLOSED).all() and not r[30:].any() and not (r == ref.R_HOLD).any()      # 20 closed frames, then the guard
    assert out['openness'][0, 30, 0] == 1.0 and out['openness'][0, 29, 0] < 0.3       # frame 30's own ear is the new baseline
    assert state[0, 0, ref.BASE] > 0.28                   # ... which the reopened eye pulls up again
    # a closure of exactly max_closed_frames frames is still a blink
    contours, _ = ref.eyelid_trace(80, [(10, 20)])
    _, _, store, count, _ = walk(contours)
    assert count[0] == 2 and store[0, 0].tolist()[:3] == [0, 10, 29]


def test_unknown_frames_move_nothing():
    contours, _ = ref.eyelid_trace(60, [(20, 5)], C=3)
    want, state, store, count, _ = walk(contours)
    holes = contours.copy()
    holes[0, 22, 0, 3, 1] = np.nan                       # inside the closure
    holes[0, 24, 0, :, 2] = 0.0                          # its last closed frame: a weight of 0
    holes[0, 25, 0, 0, 0] = np.inf                       # the reopening frame: the blink ends one frame later
    holes[0, 40, 0, 0] = holes[0, 40, 0, 3]              # an eye of no width
    out, state2, store2, count2, _ = walk(holes)
    assert np.isnan(out['openness'][0, [22, 24, 25, 40], 0]).all() and out['reason'][0, 20:27, 0].tolist() == [32] * 6 + [64]
    # the right eye's blink now ends first and is stored first; the left one's lasts a frame longer
    assert store2[0, 0].tobytes() == store[0, 1].tobytes() and store2[0, 1].tolist()[:3] == [0, 20, 25] and count2[0] == count[0] == 2
    assert store[0, :2, :3].tolist() == [[0, 20, 24], [1, 20, 24]]
    assert out['reason'][0, :, 1].tobytes() == want['reason'][0, :, 1].tobytes()


@pytest.mark.parametrize('sizes', [[1, 69], [64, 6], [10] * 7, [33, 37]], ids=['1+69', '64+6', '7x10', '33+37'])
def test_any_split_into_chunks_equals_one_pass(sizes):
    """70 frames of the shared case (ragged lengths, a reset flag, every criterion), and the same with a reset in the middle."""
    params = ref.params_of(EyeGateSpec(blink=BlinkSpec(**ref.CASE_BLINK), **ref.CASE_SPEC))
    case = ref.kernel_case(70, params)
    B, T = 3, 70
    for mid_reset in (None, 35):
        def run_split(chunks):
            carried = [case[k].copy() for k in ('state', 'store', 'count', 'dropped')]
            outs, t0 = [], 0
            for n in chunks:
                cut2 = lambda a: a.reshape(2, B, T, -1)[:, :, t0:t0 + n].reshape(2, B * n, -1)
                reset = case['reset'] if t0 == 0 else np.array([1, 0, 1], dtype=np.int32) if t0 == mid_reset else None
                outs.append(ref.run(params, B, n, *carried, pose_valid=case['pose_valid'][:, t0:t0 + n], reproj_rms=case['reproj_rms'][:, t0:t0 + n],
                                    inliers=case['inliers'][:, t0:t0 + n], warp=cut2(case['warp']), h=cut2(case['h']),
                                    contours=case['contours'][:, t0:t0 + n], lengths=np.clip(case['lengths'] - t0, 0, n), reset=reset,
                                    frame=case['frame'], patch=case['patch']))
                t0 += n
            assert t0 == T
            return {k: np.concatenate([o[k] for o in outs], axis=1) for k in outs[0]}, carried
        if mid_reset is None:
            whole, carried = run_split([T])
            assert ref.case_is_rich(T, whole, case, carried[2], carried[3])
            pieces = sizes
        else:                                            # a reset can only sit on a chunk border: the one pass is two chunks here
            whole, carried = run_split([35, 35])
            pieces = [n for half in (35, 35) for n in ([10, 10, 10, 5] if sizes == [10] * 7 else [min(sizes[0], 35), 35 - min(sizes[0], 35)]) if n]
            assert sum(pieces) == T
        got, carried_split = run_split(pieces)
        for k in whole:
            assert got[k].tobytes() == whole[k].tobytes(), (mid_reset, k)
        for a, b_ in zip(carried, carried_split):
            assert a.tobytes() == b_.tobytes(), mid_reset


# ---------------------------------------------------------------------------------------------------------------- coverage
@pytest.mark.parametrize('k', [0, 1, 4, 8])
def test_a_translation_puts_k_lattice_columns_outside(k):
    """A 128 x 64 patch: lattice columns at ox = 8, 24, .., 120.  Shifted by IW - 16 (8 - k) pixels, the columns with ox >= 16 (8 - k) land
    at u >= IW: k of them."""
    IW, IH = 640, 480
    m = ref.translation_warp(IW - 16 * (8 - k), 10.0)
    assert ref.inside_count(m, (IW, IH), (128, 64)) == 64 - 8 * k
    m = ref.translation_warp(-16.0 * k - 1.0, 10.0)      # ... and off the left edge: u = ox - 16k - 1 > -1 iff ox > 16k
    assert ref.inside_count(m, (IW, IH), (128, 64)) == 64 - 8 * k
    spec = EyeGateSpec(min_coverage=(64 - 8 * k + 1) / 64.0) if k else None
    if spec is not None:                                 # one point more than there is: the bit is set; exactly as many: it is not
        warp = np.tile(m, (2, 1, 1))
        for s_, bit in ((spec, ref.R_COVERAGE), (EyeGateSpec(min_coverage=max(64 - 8 * k, 1) / 64.0), 0 if k < 8 else ref.R_COVERAGE)):
            out = ref.run(ref.params_of(s_), 1, 1, *ref.fresh(1, 1), warp=warp, frame=(IW, IH), patch=(128, 64))
            assert out['reason'].reshape(-1).tolist() == [bit, bit]


def test_a_zero_warp_covers_nothing():
    assert ref.inside_count(np.zeros(9, dtype=np.float32), (640, 480), (128, 64)) == 0
    nan = np.full(9, np.nan, dtype=np.float32)
    assert ref.inside_count(nan, (640, 480), (128, 64)) == 0
    behind = ref.translation_warp(100.0, 100.0)
    behind[8] = -1.0                                     # Wd < 0: behind the camera
    assert ref.inside_count(behind, (640, 480), (128, 64)) == 0


# ---------------------------------------------------------------------------------------------------------------- the specs
def test_the_specs_compare_by_value_and_refuse_nonsense():
    a, b_ = EyeGateSpec(max_reproj_px=2, blink=BlinkSpec()), EyeGateSpec(max_reproj_px=2.0, blink=BlinkSpec(close_ratio=0.65))
    assert a == b_ and hash(a) == hash(b_) and a != EyeGateSpec(max_reproj_px=2) and a != EyeGateSpec(max_reproj_px=3, blink=BlinkSpec())
    assert a != EyeGateSpec(max_reproj_px=2, blink=BlinkSpec(hold_frames=3)) and a != 2 and BlinkSpec() != BlinkSpec(open_ratio=0.8)
    assert EyeGateSpec(head_yaw_left=(-0.5, 0.2)) != EyeGateSpec(head_yaw_right=(-0.5, 0.2)) and len({a, b_, EyeGateSpec()}) == 2
    assert eve_amd.EyeGateSpec is EyeGateSpec and eve_amd.BlinkSpec is BlinkSpec
    d = EyeGateSpec()                                    # every criterion off but the pose
    assert d.key() == (None,) * 7 and not d.head_angles and d.min_inside is None
    bl = BlinkSpec()                                     # closing near two thirds, reopening above it, a couple of frames of hold-off
    assert 0.6 <= bl.close_ratio <= 0.7 < bl.open_ratio < 1.0 and bl.hold_frames == 2 and bl.max_closed_frames >= 30
    assert EyeGateSpec(min_coverage=0.5).min_inside == 32 and EyeGateSpec(min_coverage=0.501).min_inside == 33
    assert EyeGateSpec(min_coverage=1e-9).min_inside == 1 and EyeGateSpec(min_coverage=1).min_inside == 64
    assert EyeGateSpec(head_pitch=(-float('inf'), 0.3)).head_pitch == (-float('inf'), 0.3)
    nan, inf = float('nan'), float('inf')
    for name, bads in (('max_reproj_px', (0, -1.0, nan, inf, '2', True)), ('min_inliers', (0, 256, 2.5, nan, True)),
                       ('min_coverage', (0, -0.1, 1.01, nan, '0.5', True)), ('head_pitch', (0.3, (0.3,), (0.3, -0.3), (nan, 0.3), ('a', 'b'))),
                       ('head_yaw_left', ((1, 0), (0, nan))), ('head_yaw_right', ((1, 0), 5)), ('blink', (True, 0.7, dict()))):
        for bad in bads:
            with pytest.raises(ValueError, match=name):
                EyeGateSpec(**{name: bad})
    for name, bads in (('close_ratio', (0, -0.5, nan, inf, '0.6')), ('open_ratio', (0, nan, inf, 0.65, 0.5)),
                       ('baseline_rate', (-0.1, 1.5, nan, None)), ('baseline_rise', (-0.1, 1.5, nan)), ('hold_frames', (-1, 1.5, nan, True)),
                       ('max_closed_frames', (0, -3, 2.5, None))):
        for bad in bads:
            with pytest.raises(ValueError, match=name):
                BlinkSpec(**{name: bad})


# ---------------------------------------------------------------------------------------------------------------- EVEStream
class GateFakes(EventFakes, CalibFakes):
    """EventFakes and CalibFakes (the ragged, masked, events and collecting steps' stand-ins, both MaskFakes) plus eye_gate, evaluated by
    tests/eye_gate_ref.py."""

    def eye_gate(self, spec, B, T, state, store, count, dropped, pose_valid=None, reproj_rms=None, inliers=None, warp=None, h=None,
                 contours=None, lengths=None, reset=None, frame_size=None, patch_size=None):
        self.calls.append('eye_gate')
        n = lambda t: None if t is None else t.detach().numpy()
        out = ref.run(ref.params_of(spec), B, T, n(state), n(store), n(count), n(dropped), pose_valid=n(pose_valid), reproj_rms=n(reproj_rms),
                      inliers=n(inliers), warp=n(warp), h=n(h), contours=n(contours), lengths=n(lengths), reset=n(reset), frame=frame_size,
                      patch=patch_size)
        return {k: torch.from_numpy(v) for k, v in out.items()}


@pytest.fixture()
def fake():
    k = GateFakes()
    kernels.set_default_kernels(k)
    yield k
    kernels.set_default_kernels(None)
    eve_amd.reset_standalone_config()


B, T = 2, 3
GATE = EyeGateSpec(blink=BlinkSpec(hold_frames=1))


def eyelids(closed):
    """eye_contours [B, 2T, 2, 6, 2] for the two chunks: open everywhere but at the (stream, frame, eye) listed."""
    c = np.concatenate([ref.eyelid_trace(2 * T, [], seed=b)[0] for b in range(B)])
    for b, t, e in closed:
        c[b, t, e] = ref.eyelid_points(0.05, centre=(100.0 + 80.0 * e, 60.0))
    return torch.from_numpy(c)


CLOSED = [(0, 1, 0), (1, 2, 1), (1, 3, 1)]              # stream 0: the left eye in frame 1; stream 1: the right eye in frames 2 .. 3


@pytest.fixture()
def scene(fake):
    model, _ = make_model(dict(refine_net_rnn_type='CGRU'))
    batch = clip(B, 2 * T, size=32)
    c = eyelids(CLOSED)
    return model, dict(chunk_of(batch, 0, T), eye_contours=c[:, :T].contiguous()), dict(chunk_of(batch, T, 2 * T), eye_contours=c[:, T:].contiguous())


def run(stream, chunk, **kw):
    return {k: v.clone() for k, v in stream.step(chunk, **kw).items()}


def reference_on(chunks, spec, capacity=256, resets=None):
    carried = ref.fresh(B, capacity)
    outs = [ref.run(ref.params_of(spec), B, T, *carried, contours=c['eye_contours'].numpy(), reset=None if resets is None else resets[i])
            for i, c in enumerate(chunks)]
    return (outs,) + carried


def test_a_gated_step_is_the_masked_step_plus_one_launch(fake, scene):
    model, c0, c1 = scene
    (w0, w1), state, store, count, _ = reference_on((c0, c1), GATE)
    assert w0['reason'][:, :, 0].tolist() == [[0, 32, 64], [0, 0, 0]] and w0['reason'][:, :, 1].tolist() == [[0, 0, 0], [0, 0, 32]]
    assert w1['reason'][:, :, 1].tolist() == [[0, 0, 0], [32, 64, 0]] and count.tolist() == [1, 1]
    masked_stream = eve_amd.EVEStream(model, B, use_graph=False)
    masked = run(masked_stream, c0, eye_mask=torch.from_numpy(w0['usable']))
    calls_masked = list(fake.calls)
    assert 'eye_gate' not in calls_masked and calls_masked.count('stream_mask_plan') == 1
    del fake.calls[:]
    s = eve_amd.EVEStream(model, B, use_graph=False)
    out = run(s, c0, gate=GATE)
    at = calls_masked.index('stream_mask_plan')
    assert fake.calls == calls_masked[:at] + ['eye_gate'] + calls_masked[at:]        # the masked step's launches and one more, before the plan
    assert sorted(out) == sorted(list(masked) + list(EYE_GATE_KEYS))
    for k in masked:
        assert torch.equal(out[k], masked[k]), k
    assert out['eye_valid'].numpy().tolist() == (w0['usable'] != 0).tolist() and out['valid'].tolist() == [[True] * 3] * 2
    for key, name in (('eye_gate_reason', 'reason'), ('eye_openness', 'openness'), ('blink', 'blink')):
        assert out[key].numpy().tobytes() == w0[name].tobytes(), key
    # the second step: the state carried; an eye_mask of the caller's is ANDed with the gate's verdict
    mine = torch.ones(B, T, 2, dtype=torch.bool)
    mine[0, 2, 0] = False
    out1 = run(s, c1, gate=GATE, eye_mask=mine)
    masked1 = run(masked_stream, c1, eye_mask=torch.from_numpy(w1['usable'] != 0) & mine)
    for k in masked1:
        assert torch.equal(out1[k], masked1[k]), k
    assert out1['eye_gate_reason'].numpy().tobytes() == w1['reason'].tobytes()
    assert s.get_gate_state().numpy().tobytes() == state.tobytes() and s.blink_counts()[0].tolist() == [1, 1]
    rows = s.blinks()
    assert rows[0].tolist() == [[0.0, 1.0, 1.0, store[0, 0, 3]]] and rows[1][0, :3].tolist() == [1.0, 2.0, 3.0] and len(s.blinks([1])) == 1
    s.clear_blinks([0])
    assert s.blink_counts()[0].tolist() == [0, 1] and not any('gate' in k for k in s.get_state())
    # ragged: frames past a stream's count are not delivered -- no tick, no state, reason 0
    s = eve_amd.EVEStream(model, B, use_graph=False)
    out = run(s, c0, gate=GATE, lengths=[2, 0])
    assert out['eye_gate_reason'][0].tolist() == [[0, 0], [32, 0], [0, 0]] and not out['eye_gate_reason'][1].any()
    assert torch.isnan(out['eye_openness'][1]).all() and s.get_gate_state()[:, 0, ref.TICK].tolist() == [2.0, 0.0]
    assert out['eye_valid'][0].tolist() == [[True, True], [False, True], [False, False]]


def test_without_gate_every_step_issues_what_it_always_did(fake, scene):
    model, c0, c1 = scene
    used = eve_amd.EVEStream(model, B, use_graph=False)
    run(used, c0, gate=GATE)
    events = GazeEventSpec(fps=30)
    target = torch.full((B, T, 2), 500.0)
    modes = [dict(), dict(lengths=[2, 1]), dict(eye_mask=torch.ones(B, T, 2, dtype=torch.bool)), dict(events=events),
             dict(chunk=dict(calibration_target=target))]
    for kw in modes:
        kw = dict(kw)
        extra = kw.pop('chunk', {})
        plain = {k: v for k, v in c1.items() if k != 'eye_contours'}
        del fake.calls[:]
        want = run(eve_amd.EVEStream(model, B, use_graph=False), dict(plain, **extra), **kw)
        calls = list(fake.calls)
        assert 'eye_gate' not in calls
        for chunk in (plain, c1):                        # eye_contours alone in the chunk changes nothing either
            del fake.calls[:]
            fresh = eve_amd.EVEStream(model, B, use_graph=False)
            fresh._gate_buffers()
            got = run(fresh, dict(chunk, **extra), **kw)
            assert fake.calls == calls and sorted(got) == sorted(want), kw
            for k in want:
                assert got[k].numpy().tobytes() == want[k].numpy().tobytes(), k
    state = used.get_gate_state()
    run(used, c1)                                        # a step without gate leaves the gate's state alone
    assert torch.equal(used.get_gate_state(), state) and state[:, 0, ref.TICK].tolist() == [T, T]


def test_refusals_come_before_any_launch(fake, scene):
    model, c0, _ = scene
    s = eve_amd.EVEStream(model, B, use_graph=False)
    bare = {k: v for k, v in c0.items() if k != 'eye_contours'}
    with pytest.raises(ValueError, match='EyeGateSpec'):
        s.step(c0, gate=dict(blink=True))
    with pytest.raises(ValueError, match='min_coverage'):
        s.step(c0, gate=EyeGateSpec(min_coverage=0.5))
    for name in ('head_pitch', 'head_yaw_left', 'head_yaw_right'):
        with pytest.raises(ValueError, match='camera form'):
            s.step(c0, gate=EyeGateSpec(**{name: (-0.3, 0.3)}))
    with pytest.raises(ValueError, match='max_reproj_px'):
        s.step(c0, gate=EyeGateSpec(max_reproj_px=2.0))
    with pytest.raises(ValueError, match='min_inliers'):
        s.step(c0, gate=EyeGateSpec(min_inliers=5))
    with pytest.raises(ValueError, match='eye_contours'):
        s.step(bare, gate=GATE)
    good = c0['eye_contours']
    for bad in (good.double(), good[:, :, :, :5], good[:, :2], good[..., :1], good.numpy(), torch.cat([good, good], dim=-1)):
        with pytest.raises(ValueError, match='eye_contours'):
            s.step(dict(bare, eye_contours=bad), gate=GATE)
        with pytest.raises(ValueError, match='eye_contours'):
            s.step(dict(bare, eye_contours=bad), gate=EyeGateSpec())          # checked whenever a gate comes with it
    # the face-landmark form without face_inliers (no face_huber_px, no face_landmarks_raw); a surface without its layout
    faced = dict(bare, camera_frame=torch.zeros(B, T, 48, 64, 3, dtype=torch.uint8), face_landmarks=torch.zeros(B, T, 7, 2),
                 face_rig=torch.zeros(B, 12 + 21))
    faced = {k: v for k, v in faced.items() if k not in ('left_eye_patch', 'right_eye_patch')}
    with pytest.raises(ValueError, match='min_inliers'):
        s._check_gate(faced, EyeGateSpec(min_inliers=5), B, T)
    surface = dict({k: v for k, v in faced.items() if k != 'camera_frame'}, camera_surface=torch.zeros(B, T, 48, 64, dtype=torch.uint8))
    with pytest.raises(ValueError, match='camera_layout'):
        s._check_gate(surface, EyeGateSpec(min_coverage=0.5), B, T)
    with pytest.raises(ValueError, match='blink_capacity'):
        eve_amd.EVEStream(model, B, use_graph=False, blink_capacity=0)
    with pytest.raises(ValueError, match='state'):
        s.set_gate_state(np.zeros((B, 2, 7)))
    assert fake.calls == []
    # what the checks let through: the frame size from the frame key's shape, or from the layout
    plan = s._check_gate(faced, EyeGateSpec(min_coverage=0.5, max_reproj_px=2.0, head_pitch=(-1, 1)), B, T)
    assert plan['frame_size'] == (64, 48)
    nv12 = dict({k: v for k, v in faced.items() if k != 'camera_frame'}, camera_frame_nv12=torch.zeros(B, T, 72, 64, dtype=torch.uint8))
    assert s._check_gate(nv12, EyeGateSpec(min_coverage=0.5), B, T)['frame_size'] == (64, 48)
    model.eye_net.face_huber_px = 2.0
    assert s._check_gate(faced, EyeGateSpec(min_inliers=5), B, T)['frame_size'] is None
    model.eye_net.face_huber_px = None
    assert fake.calls == []
    out = s.step(c0, gate=EyeGateSpec())                 # pre-cut patches, no criterion: a masked step in which everything is usable
    assert out['eye_valid'].all() and not out['eye_gate_reason'].any() and torch.isnan(out['eye_openness']).all()


def test_the_graph_key_holds_the_spec_and_the_contours(fake, scene):
    model, c0, _ = scene
    s = eve_amd.EVEStream(model, B, use_graph=False)
    plan = lambda spec, ch=c0: s._check_gate(ch, spec, B, T)
    bare = s._graph_key(c0, False, False, True)
    a = s._graph_key(c0, False, False, True, None, None, plan(GATE))
    assert a != bare and a == s._graph_key(dict(c0), False, False, True, None, None, plan(EyeGateSpec(blink=BlinkSpec(hold_frames=1))))
    assert a != s._graph_key(c0, False, False, True, None, None, plan(EyeGateSpec(blink=BlinkSpec(hold_frames=2))))
    assert a != s._graph_key(c0, False, False, True, None, None, plan(EyeGateSpec()))
    without = {k: v for k, v in c0.items() if k != 'eye_contours'}
    assert s._graph_key(c0, False, False, True, None, None, plan(EyeGateSpec())) != \
        s._graph_key(without, False, False, True, None, None, plan(EyeGateSpec(), without))
    weighted = dict(c0, eye_contours=torch.cat([c0['eye_contours'], torch.ones(B, T, 2, 6, 1)], dim=-1))
    assert a != s._graph_key(weighted, False, False, True, None, None, plan(GATE, weighted))
    captured = []
    s._capture = lambda chunk, *a_, **k_: captured.append((a_, k_)) or {'n': len(captured)}
    first = s._graph_for(c0, False, False, True, None, None, plan(GATE))
    assert s._graph_for(c0, False, False, True, None, None, plan(GATE)) is first and len(captured) == 1 and 'gate' in captured[0][1]
    assert s._graph_for(c0, False, False, True) is not first and len(captured) == 2 and captured[1] == ((False, False, True, None), {})


def test_reset_reaches_the_gate_with_and_without_a_gated_step(fake, scene):
    model, c0, c1 = scene
    s = eve_amd.EVEStream(model, B, use_graph=False)
    run(s, c0, gate=GATE)
    assert s.get_gate_state()[1, 1, ref.CLOSED] == 1      # stream 1's right eye is closed at the chunk's end
    s.reset([1])
    out = run(s, c1, gate=GATE)
    (_, w1), state, _, count, _ = reference_on((c0, c1), GATE, resets=[None, np.array([0, 1], dtype=np.int32)])
    assert out['eye_gate_reason'].numpy().tobytes() == w1['reason'].tobytes() and s.get_gate_state().numpy().tobytes() == state.tobytes()
    assert s.blink_counts()[0].tolist() == count.tolist() == [1, 0]      # the closure the reset cut short is no blink
    assert s.get_gate_state()[:, 0, ref.TICK].tolist() == [2 * T, T]
    # a reset before a step WITHOUT gate still clears the flagged stream's rows: no launch, and the plain step
    before = s.get_gate_state()
    s.reset([0])
    del fake.calls[:]
    run(s, {k: v for k, v in c0.items() if k != 'eye_contours'})
    assert 'eye_gate' not in fake.calls
    after = s.get_gate_state()
    assert not after[0].any() and torch.equal(after[1], before[1]) and s.blink_counts()[0].tolist() == [1, 0]
