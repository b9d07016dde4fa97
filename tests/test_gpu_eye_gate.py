"""GPU: eve_eye_gate against the numpy contract of tests/eye_gate_ref.py, and EVEStream's step(gate=...) around it (eager and
captured).  Every test here needs the entry point, EyeGateSpec or the gate argument, so every one fails without them.

Everything is compared bit for bit: usable, reason, openness (the float32 rounded once from the float64 value), blink, the state rows,
the store and its counters.  Nothing but + - * / sqrt and comparisons leads to them, each correctly rounded in float64 on both sides.
Before each comparison the reference ALONE is asked whether the inputs show what they were built to show (ref.case_is_rich)."""
import ctypes

import numpy as np
import pytest
import torch

import eve_amd
import eye_gate_ref as ref
from eve_amd import data
from eve_amd._lib import EyeGateParams
from eve_amd.data import EYE_GATE_KEYS, BlinkSpec, EyeGateSpec, GazeEventSpec
from eve_amd.eye_net import eye_pose_batch
from eve_amd.kernels import default_kernels
from test_gpu_calibration import cuda, guarded, guards_hold
from test_gpu_face_pose import CAM, face_chunks, rest_of_clip
from test_gpu_stream import make_model

pytestmark = pytest.mark.gpu
SPEC = EyeGateSpec(blink=BlinkSpec(**ref.CASE_BLINK), **ref.CASE_SPEC)
PARAMS = ref.params_of(SPEC)
OUTS = ('usable', 'reason', 'openness', 'blink')
B = 3


def device_case(case):
    """The case's arrays on the device; state, store and counters as fresh copies."""
    return {k: (cuda(v) if isinstance(v, np.ndarray) else v) for k, v in case.items()}


def launch(dev, spec=SPEC, t0=None, t1=None, lengths='case', reset='case'):
    """HipKernels.eye_gate on frames t0 .. t1 - 1 of the device case (state, store and counters updated in place)."""
    T = dev['pose_valid'].shape[1]
    t0, t1 = 0 if t0 is None else t0, T if t1 is None else t1
    n = t1 - t0
    cut = lambda a: a[:, t0:t1].contiguous()
    cut2 = lambda a: a.view(2, B, T, -1)[:, :, t0:t1].reshape(2, B * n, -1).contiguous()
    return default_kernels().eye_gate(
        spec, B, n, dev['state'], dev['store'], dev['count'], dev['dropped'], pose_valid=cut(dev['pose_valid']), reproj_rms=cut(dev['reproj_rms']),
        inliers=cut(dev['inliers']), warp=cut2(dev['warp']), h=cut2(dev['h']), contours=cut(dev['contours']),
        lengths=dev['lengths'] if lengths == 'case' else lengths, reset=dev['reset'] if reset == 'case' else reset,
        frame_size=dev['frame'], patch_size=dev['patch'])


def same_bits(got, want, what=''):
    for k in OUTS:
        g = got[k].cpu().numpy()
        assert g.dtype == want[k].dtype and g.tobytes() == want[k].tobytes(), (what, k)


# ---------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize('T', [1, 5, 70])
def test_kernel_equals_the_reference_bit_for_bit(T):
    """B = 3 and the shared case (ref.kernel_case): every reason bit, both values of usable for each eye (T = 1, with its four delivered
    cells, cannot show a usable eye too), a stored and a dropped blink, NaN contours, a weight of 0, a NaN rms, a zero warp, lengths
    of 0 and of T, a reset flag; T = 70 crosses the 64-frame pass boundary with an eye closed.  The state and the store lie between
    guards."""
    case = ref.kernel_case(T, PARAMS)
    want, state, store, count, dropped = ref.run_case(case, PARAMS)
    assert ref.case_is_rich(T, want, case, count, dropped)
    dev = device_case(case)
    SENT = -777.25
    s_whole, dev['state'] = guarded((B, 2, 8), torch.float64, SENT)
    f_whole, dev['store'] = guarded((B, 2, 4), torch.float64, SENT)
    dev['state'].copy_(cuda(case['state'])), dev['store'].copy_(cuda(case['store']))
    got = launch(dev)
    torch.cuda.synchronize()
    assert default_kernels().lib.eve_last_kernel() == b'eye_gate_kernel'
    same_bits(got, want)
    assert dev['state'].cpu().numpy().tobytes() == state.tobytes() and dev['store'].cpu().numpy().tobytes() == store.tobytes()
    assert dev['count'].cpu().tolist() == count.tolist() and dev['dropped'].cpu().tolist() == dropped.tolist()
    assert guards_hold(s_whole, SENT) and guards_hold(f_whole, SENT)


def split_run(case, sizes):
    """The case's 70 frames in chunks of `sizes`, the state carried between the launches; lengths and reset as in the case, cut to
    the chunk (the reset flag with the first chunk only)."""
    dev = device_case(case)
    parts, t0 = [], 0
    for n in sizes:
        lengths = (dev['lengths'] - t0).clamp(0, n).to(torch.int32)
        parts.append(launch(dev, t0=t0, t1=t0 + n, lengths=lengths, reset=dev['reset'] if t0 == 0 else None))
        t0 += n
    assert t0 == case['pose_valid'].shape[1]
    joined = {k: torch.cat([p[k] for p in parts], dim=1) for k in OUTS}
    return joined, [dev[k] for k in ('state', 'store', 'count', 'dropped')]


def test_chunk_splits_on_the_device_give_identical_bits():
    case = ref.kernel_case(70, PARAMS)
    want, state, store, count, dropped = ref.run_case(case, PARAMS)
    whole, carried = split_run(case, [70])
    same_bits(whole, want)
    for sizes in ([64, 6], [1, 69], [10] * 7):
        split, carried_split = split_run(case, sizes)
        for k in OUTS:
            assert split[k].cpu().numpy().tobytes() == whole[k].cpu().numpy().tobytes(), (sizes, k)
        for a, b_ in zip(carried, carried_split):
            assert a.cpu().numpy().tobytes() == b_.cpu().numpy().tobytes(), sizes
    assert carried[0].cpu().numpy().tobytes() == state.tobytes() and carried[2].cpu().tolist() == count.tolist()


def test_two_launches_on_copies_of_one_state_agree():
    case = ref.kernel_case(70, PARAMS)
    runs = []
    for _ in range(2):
        dev = device_case(case)
        out = launch(dev)
        runs.append([out[k] for k in OUTS] + [dev[k] for k in ('state', 'store', 'count', 'dropped')])
    for a, b_ in zip(*runs):
        assert a.cpu().numpy().tobytes() == b_.cpu().numpy().tobytes()


def test_the_library_refuses_without_a_launch():
    k = default_kernels()
    T = 2
    z = lambda *s, dtype=torch.float32: torch.zeros(s, dtype=dtype, device='cuda')
    state, store, count, dropped = z(B, 2, 8, dtype=torch.float64), z(B, 2, 4, dtype=torch.float64), z(B, dtype=torch.int32), z(B, dtype=torch.int32)
    outs = [z(B, T, 2, dtype=torch.uint8), z(B, T, 2, dtype=torch.uint8), z(B, T, 2), z(B, T, 2, dtype=torch.uint8)]
    warp, contours = z(2, B * T, 9), z(B, T, 2, 6, 3)
    state.fill_(5.0)
    before = k.lib.eve_last_kernel()

    def params(**over):
        P = EyeGateParams()
        for name, v in ref.params_of(SPEC, **over).items():
            if name in ('yaw_lo', 'yaw_hi'):
                getattr(P, name)[0], getattr(P, name)[1] = v
            else:
                setattr(P, name, v)
        return P

    def call(P=None, Bn=B, Tn=T, C=3, sizes=(640, 480, 128, 64), capacity=2, null=None, with_warp=True, with_contours=True):
        p = k._p
        o = [None if null == i else p(t) for i, t in enumerate(outs)]
        return k.lib.eve_eye_gate(Bn, Tn, None, None, None, p(warp) if with_warp else None, None, p(contours) if with_contours else None, C, None,
                                  None, *sizes, ctypes.byref(P if P is not None else params()), None if null == 'state' else p(state), capacity,
                                  p(store), p(count), p(dropped), *o, k._stream())

    nan = float('nan')
    refused = [dict(null=0), dict(null=2), dict(null='state'), dict(Bn=0), dict(Tn=0), dict(capacity=0), dict(C=4), dict(C=1),
               dict(sizes=(0, 480, 128, 64)), dict(sizes=(640, 480, 0, 0)), dict(Bn=0x7fffffff // 36 + 1, Tn=1), dict(Bn=1 << 40),
               dict(P=params(max_reproj_px=nan)), dict(P=params(pitch_lo=nan)), dict(P=params(yaw_hi=(0.5, nan))), dict(P=params(open_ratio=nan)),
               dict(P=params(baseline_rate=nan)), dict(P=params(open_ratio=0.5, close_ratio=0.5)), dict(P=params(open_ratio=0.4, close_ratio=0.6)),
               dict(P=params(min_inside=0)), dict(P=params(min_inside=65)), dict(P=params(hold_frames=-1)), dict(P=params(max_closed_frames=0))]
    for kw in refused:
        assert call(**kw) != 0, kw
        assert b'eye_gate' in k.lib.eve_last_error(), kw
        assert k.lib.eve_last_kernel() == before, kw
    with pytest.raises(TypeError, match='state'):
        k.eye_gate(SPEC, B, T, state.float(), store, count, dropped)
    with pytest.raises(ValueError, match='criterion'):
        k.eye_gate(EyeGateSpec(), B, T, state, store, count, dropped, warp=warp, frame_size=(640, 480), patch_size=(128, 64))
    torch.cuda.synchronize()
    assert (state == 5.0).all() and not count.any() and not any(o.any() for o in outs)
    assert call(with_warp=True) == 0 and k.lib.eve_last_kernel() == b'eye_gate_kernel'      # the same call with sound arguments
    assert call(with_warp=False, sizes=(0, 0, 0, 0)) == 0 and call(with_contours=False, C=0, P=params(open_ratio=0.1)) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- EVEStream
TC = 5
E2E_BLINK = BlinkSpec(hold_frames=1, max_closed_frames=20)
# the clip's heads: rms 0.05 .. 0.14 px, 6 or 7 inliers of 7, stream 0 turned by some 0.25 rad (its left eye the far one) and pitched by
# up to -0.25; every patch lies inside the frame, so only the invalid pose's zero warp fails the coverage
E2E_SPEC = EyeGateSpec(max_reproj_px=0.125, min_inliers=7, min_coverage=0.9, head_pitch=(-0.22, 0.3), head_yaw_left=(-0.3, 0.25),
                       head_yaw_right=(-0.25, 0.3), blink=E2E_BLINK)
HUBER_PX = 0.25


@pytest.fixture(scope='module')
def rig():
    """One model (face_huber_px set, so the solve reports face_inliers) and one 3 x 10 face-landmark clip with eyelid points, shared and
    never modified: frame (0, 3) has a NaN landmark; stream 0's left eye closes in frames 1 .. 2 and stream 2's both in frames 4 .. 6
    (across the two chunks); a NaN contour at (1, 7)."""
    model, _ = make_model(refine_net_rnn_type='CGRU')
    model.eye_net.face_huber_px = HUBER_PX
    rest = rest_of_clip(B, 2 * TC, seed=7)
    frames = torch.randint(0, 256, (B, 2 * TC) + CAM + (3,), generator=torch.Generator().manual_seed(8), dtype=torch.uint8).cuda()
    lm, face_rig = face_chunks(B, 2 * TC, seed=9, invalid=[(0, 3)])
    contours = np.concatenate([ref.eyelid_trace(2 * TC, c, seed=20 + b, C=3)[0] for b, c in enumerate(([(1, 2)], [], [(4, 3)]))])
    contours[0, 1:3, 1] = contours[0, 0, 1]                  # stream 0: the right eye stays open
    contours[1, 7, 0, 2, 0] = np.nan
    d = dict(rest, camera_frame=frames, face_landmarks=lm, eye_contours=cuda(contours))
    chunk = lambda t0, t1: dict({k: v[:, t0:t1].contiguous() for k, v in d.items()}, face_rig=face_rig)
    return {'model': model, 'chunks': (chunk(0, TC), chunk(TC, 2 * TC))}


def keep(out):
    return {k: v.clone() for k, v in out.items()}


def reference_steps(model, chunks, spec, lengths=None, reset_before=None, capacity=256):
    """The reference over the steps' own derived quantities: eye_pose_batch run once more on each chunk with a carried head pose of
    its own gives the bits the step's launch read (pose_valid, face_reproj_rms, face_inliers, the warps, the head angles).
    -> (per step the reference's outputs, state, store, count, dropped)."""
    face_state = torch.zeros((B, 13), dtype=torch.float64, device='cuda')
    state, store, count, dropped = ref.fresh(B, capacity)
    P = ref.params_of(spec)
    ph, pw = data.eye_patch_hw(model.config)
    wants = []
    for i, chunk in enumerate(chunks):
        n = None if lengths is None else torch.tensor(lengths[i], dtype=torch.int32, device='cuda')
        flags = None
        if reset_before is not None and reset_before[i] is not None:
            flags = torch.zeros((B,), dtype=torch.int32, device='cuda')
            flags[reset_before[i]] = 1
        d = eye_pose_batch(chunk, model.config, face_state, flags, n, huber_px=model.eye_net.face_huber_px)
        T = chunk['camera_frame'].shape[1]
        both = lambda key, m: torch.stack([d['left' + key], d['right' + key]]).reshape(2, B * T, m).float().cpu().numpy()
        wants.append(ref.run(
            P, B, T, state, store, count, dropped, pose_valid=d['pose_valid'].to(torch.uint8).cpu().numpy(),
            reproj_rms=d['face_reproj_rms'].cpu().numpy() if spec.max_reproj_px is not None else None,
            inliers=d['face_inliers'].cpu().numpy() if spec.min_inliers is not None else None,
            warp=both('_eye_warp', 9) if spec.min_coverage is not None else None, h=both('_h', 2) if spec.head_angles else None,
            contours=chunk['eye_contours'].cpu().numpy() if spec.blink is not None else None,
            lengths=None if lengths is None else np.asarray(lengths[i]), reset=None if flags is None else flags.cpu().numpy(),
            frame=(CAM[1], CAM[0]), patch=(pw, ph)))
    return wants, state, store, count, dropped


def two_steps(stream, chunks, lengths=None, masks=None, extra=None, **kw):
    outs = []
    for i, chunk in enumerate(chunks):
        if lengths is not None:
            kw['lengths'] = lengths[i]
        if masks is not None:
            kw['eye_mask'] = masks[i]
        outs.append(keep(stream.step(chunk if extra is None else dict(chunk, **extra[i]), **kw)))
    return outs


def specified(a, out):
    """The entries of a result that the step specifies: those at valid frames."""
    return a[out['valid']] if 'valid' in out and tuple(a.shape[:2]) == tuple(out['valid'].shape) else a


def assert_same_steps(got, want, keys=None):
    for g, w in zip(got, want):
        for k in (keys if keys is not None else w):
            assert specified(g[k], w).cpu().numpy().tobytes() == specified(w[k], w).cpu().numpy().tobytes(), k


def gate_matches(outs, wants, lengths=None):
    for i, (out, want) in enumerate(zip(outs, wants)):
        live = np.ones((B, TC), dtype=bool) if lengths is None else np.arange(TC)[None, :] < np.asarray(lengths[i])[:, None]
        usable = (want['usable'] != 0) & live[:, :, None]
        assert np.array_equal(out['eye_valid'].cpu().numpy(), usable) and np.array_equal(out['valid'].cpu().numpy(), usable.any(axis=2))
        for key, name in (('eye_gate_reason', 'reason'), ('eye_openness', 'openness'), ('blink', 'blink')):
            assert out[key].cpu().numpy().tobytes() == want[name].tobytes(), (i, key)


@pytest.mark.parametrize('mode', ['plain', 'lengths', 'events+calibration'])
def test_gated_step_equals_the_masked_step_on_the_reference_mask(rig, mode):
    model, chunks = rig['model'], rig['chunks']
    lengths = [[5, 3, 5], [4, 5, 0]] if mode == 'lengths' else None
    kw, extra = {}, None
    if mode == 'events+calibration':
        kw['events'] = GazeEventSpec(fps=30)
        extra = [{'calibration_target': torch.full((B, TC, 2), 500.0 + 100 * i, device='cuda')} for i in range(2)]
    wants, state, store, count, dropped = reference_steps(model, chunks, E2E_SPEC, lengths)
    reasons = np.concatenate([w['reason'].reshape(-1) for w in wants])
    assert np.bitwise_or.reduce(reasons) & (ref.R_POSE | ref.R_CLOSED | ref.R_HOLD) == ref.R_POSE | ref.R_CLOSED | ref.R_HOLD
    assert mode == 'lengths' or np.bitwise_or.reduce(reasons) == 127     # every criterion vetoes an eye somewhere in the clip
    assert all((np.concatenate([w['usable'] for w in wants], axis=1)[..., e] == v).any() for e in range(2) for v in (0, 1)) and count.sum() >= 1
    masks = [cuda(w['usable']) for w in wants]
    eager_stream, graph_stream = eve_amd.EVEStream(model, B, use_graph=False), eve_amd.EVEStream(model, B)
    eager = two_steps(eager_stream, chunks, lengths, extra=extra, gate=E2E_SPEC, **kw)
    graph = two_steps(graph_stream, chunks, lengths, extra=extra, gate=E2E_SPEC, **kw)
    masked_stream = eve_amd.EVEStream(model, B, use_graph=False)
    masked = two_steps(masked_stream, chunks, lengths, masks=masks, extra=extra, **kw)
    assert len(graph_stream._graphs) == 1                                # the second step replayed the first one's graph
    for outs in (eager, graph):
        assert sorted(outs[0]) == sorted(list(masked[0]) + list(EYE_GATE_KEYS))
        assert_same_steps(outs, masked)                                  # every key of the masked step, at the frames it specifies
        gate_matches(outs, wants, lengths)
    for s_ in (eager_stream, graph_stream):                              # (the capture's warm-up steps moved no gate state)
        assert s_.get_gate_state().cpu().numpy().tobytes() == state.tobytes()
        assert s_._gate[1].cpu().numpy().tobytes() == store.tobytes() and s_.blink_counts()[0].tolist() == count.tolist()
    if mode == 'events+calibration':                                     # the events and the collection consumed the gated validity
        for a, b_ in zip(eager_stream._events, masked_stream._events):
            assert a.cpu().numpy().tobytes() == b_.cpu().numpy().tobytes()
        for a, b_ in zip(eager_stream._calib_store, masked_stream._calib_store):
            assert a.cpu().numpy().tobytes() == b_.cpu().numpy().tobytes()
        assert eager_stream.calibration_counts()[0].sum() < 2 * B * 2 * TC


def test_blinks_over_two_steps_and_a_reset(rig):
    model, chunks = rig['model'], rig['chunks']
    spec = EyeGateSpec(blink=E2E_BLINK)
    wants, state, store, count, dropped = reference_steps(model, chunks, spec, reset_before=[None, [1]])
    assert count.tolist() == [1, 0, 2] and state[:, 0, ref.TICK].tolist() == [10, 5, 10]
    stream = eve_amd.EVEStream(model, B, blink_capacity=256)
    assert [b_.shape for b_ in stream.blinks()] == [(0, 4)] * B
    first = keep(stream.step(chunks[0], gate=spec))
    before = stream.get_gate_state()
    stream.reset([1])
    second = keep(stream.step(chunks[1], gate=spec))
    gate_matches([first, second], wants)
    after = stream.get_gate_state().cpu().numpy()
    assert after.tobytes() == state.tobytes() and before[1, 0, ref.TICK] == 5 and after[1, 0, ref.TICK] == 5
    got, lost = stream.blink_counts()
    assert got.tolist() == count.tolist() and lost.tolist() == dropped.tolist()
    rows = stream.blinks()
    for b in range(B):
        assert rows[b].tobytes() == store[b, :count[b]].tobytes()
    assert rows[0][0].tolist()[:3] == [0.0, 1.0, 2.0] and rows[2][:, :3].tolist() == [[0.0, 4.0, 6.0], [1.0, 4.0, 6.0]]
    assert len(stream.blinks([2])) == 1
    stream.clear_blinks([2])
    assert stream.blink_counts()[0].tolist() == [1, 0, 0]
    # a reset before a step WITHOUT gate still clears the flagged stream's rows, and leaves the others'
    stream.reset([0])
    stream.step({k: v for k, v in chunks[0].items() if k != 'eye_contours'})
    cleared = stream.get_gate_state().cpu().numpy()
    assert not cleared[0].any() and cleared[1:].tobytes() == state[1:].tobytes()
    saved = stream.get_gate_state()
    stream.set_gate_state(torch.zeros(B, 2, 8))
    assert not stream.get_gate_state().any()
    stream.set_gate_state(saved)
    assert torch.equal(stream.get_gate_state(), saved)


def test_the_stand_alone_call_is_the_kernel_call_from_fresh_state():
    case = ref.kernel_case(5, PARAMS)
    T = 5
    inputs = {k: v for k, v in case.items() if k not in ('state', 'store', 'count', 'dropped', 'reset')}
    inputs['contours'] = np.concatenate([ref.eyelid_trace(T, [(1, 2)], seed=b, C=3)[0] for b in range(B)])      # from fresh state: a blink of its own
    state, store, count, dropped = ref.fresh(B, 4)
    want = ref.run(PARAMS, B, T, state, store, count, dropped, **inputs)
    assert count.sum() >= 1 and want['reason'].any() and (want['usable'] == 1).any()
    got = data.eye_gate(SPEC, B, T, pose_valid=cuda(case['pose_valid']) != 0, reproj_rms=cuda(case['reproj_rms']), inliers=cuda(case['inliers']),
                        warps=cuda(case['warp']).view(2, B, T, 3, 3), h=cuda(case['h']).view(2, B, T, 2), eye_contours=cuda(inputs['contours']),
                        frame_size=case['frame'], patch_size=case['patch'], lengths=cuda(case['lengths']), blink_capacity=4)
    assert sorted(got) == sorted(('usable', 'blinks', 'blink_count', 'blink_dropped', 'gate_state') + EYE_GATE_KEYS)
    for key, name in (('usable', 'usable'), ('eye_gate_reason', 'reason'), ('eye_openness', 'openness'), ('blink', 'blink')):
        assert got[key].cpu().numpy().tobytes() == want[name].tobytes(), key
    assert got['gate_state'].cpu().numpy().tobytes() == state.tobytes() and got['blinks'].cpu().numpy().tobytes() == store.tobytes()
    assert got['blink_count'].cpu().tolist() == count.tolist() and got['blink_dropped'].cpu().tolist() == dropped.tolist()
    with pytest.raises(ValueError, match='min_coverage'):
        data.eye_gate(SPEC, B, T, reproj_rms=cuda(case['reproj_rms']), inliers=cuda(case['inliers']), h=cuda(case['h']).view(2, B, T, 2),
                      eye_contours=cuda(case['contours']))
    with pytest.raises(ValueError, match='EyeGateSpec'):
        data.eye_gate(None, B, T)
