"""GPU: eve_gaze_history_plan + eve_gaze_history_update against the numpy contract of tests/gaze_history_ref.py, and EVEStream's
step(history=...) around them (eager and captured).  Every comparison is EQUAL BITS -- maps, per-frame maps and state rows: the contract
owns its exp, so nothing is left to a library.  Every test here needs the entry points, GazeHistorySpec or the history argument, so
every one fails without them."""
import numpy as np
import pytest
import torch

import eve_amd
import gaze_history_ref as ref
import overlay_ref as oref
from eve_amd import data
from eve_amd.data import GazeEventSpec, GazeHistorySpec, OverlaySpec
from eve_amd.kernels import default_kernels
from test_gpu_calibration import cuda, guarded, guards_hold
from test_gpu_overlay import CAPTURE, nv12_capture
from test_gpu_stream import gpu_clip, make_model

pytestmark = pytest.mark.gpu
SENT = -777.25


def device_run(P, screen, state, maps, T, pog=None, heat=None, frame_time=None, valid=None, valid_key=None, lengths=None, reset=None,
               per_frame=False):
    """The two C entry points themselves, every buffer they write between guards.  -> (state, maps, frames) as numpy."""
    k = default_kernels()
    p = k._p
    B, MH, MW = maps.shape
    s_whole, d_state = guarded((B, 8), torch.float64, SENT)
    m_whole, d_maps = guarded((B, MH, MW), torch.float32, SENT)
    c_whole, d_coef = guarded((B, max(T, 1), 4), torch.float64, SENT)
    l_whole, d_clear = guarded((B,), torch.int32, -7)
    f_whole, d_frames = guarded((B, max(T, 1), MH, MW), torch.float32, SENT)
    d_state.copy_(cuda(state)), d_maps.copy_(cuda(maps))
    dev = lambda a, dtype=None: None if a is None else cuda(np.asarray(a) if dtype is None else np.asarray(a).astype(dtype))
    d_heat, d_pog, d_time = dev(heat), dev(pog), dev(frame_time)          # (held until the launches have run)
    d_valid, d_key, d_len, d_reset = dev(valid, np.uint8), dev(valid_key, np.uint8), dev(lengths, np.int32), dev(reset, np.int32)
    k._ck(k.lib.eve_gaze_history_plan(B, T, p(d_pog), p(d_time), p(d_valid), p(d_key), p(d_len), p(d_reset),
                                      0.0 if P['fps'] is None else P['fps'], P['ln_decay'], 1 if P['seconds'] else 0, P['max_gap_s'], P['gain'], MW, MH, float(screen[0]), float(screen[1]),
                                      p(d_state), p(d_coef) if T else None, p(d_clear), k._stream()))
    assert k.lib.eve_last_kernel().decode() == 'gaze_history_plan_kernel'
    k._ck(k.lib.eve_gaze_history_update(B, T, MH, MW, p(d_coef) if T else None, p(d_clear), p(d_heat), P['alpha'], P['floor'], p(d_maps),
                                        p(d_frames) if per_frame else None, k._stream()))
    assert k.lib.eve_last_kernel().decode() == 'gaze_history_update_kernel'
    torch.cuda.synchronize()
    for whole, sentinel in ((s_whole, SENT), (m_whole, SENT), (c_whole, SENT), (l_whole, -7), (f_whole, SENT)):
        assert guards_hold(whole, sentinel)
    if not per_frame or T == 0:
        assert bool((d_frames == SENT).all())
    if T == 0:
        assert bool((d_coef == SENT).all())
    return d_state.cpu().numpy(), d_maps.cpu().numpy(), d_frames.cpu().numpy() if per_frame else None


def check(P, screen, state, maps, T, lengths=None, per_frame=False, **kw):
    """Device == reference, bit for bit, from the same carried state and maps (which the reference then holds updated)."""
    got_state, got_maps, got_frames = device_run(P, screen, state, maps, T, lengths=lengths, per_frame=per_frame, **kw)
    want_frames = ref.run(P, screen, state, maps, T, lengths=lengths, per_frame=per_frame, **kw)
    assert got_state.tobytes() == state.tobytes()
    assert got_maps.tobytes() == maps.tobytes()
    assert np.isfinite(maps).all() and not ((maps != 0) & (np.abs(maps) < 2.0 ** -100)).any()
    if per_frame:
        n = [T] * maps.shape[0] if lengths is None else [min(max(int(v), 0), T) for v in lengths]
        for b, nb in enumerate(n):
            assert got_frames[b, :nb].tobytes() == want_frames[b, :nb].tobytes(), b
    return want_frames


def centres(B, T, MW, MH, scale=16.0):
    """On a pixel, between pixels, far off the screen (screen = map * 16, so 16 px of the screen are one of the map, exactly)."""
    pog = np.zeros((B, T, 2), dtype=np.float32)
    kinds = [(scale * (MW // 2), scale * (MH // 2)), (scale * (MW // 3) + 8.0, scale * (MH // 3) + 5.0), (1e7, -3e6),
             (scale * (MW - 1), 0.0), (-40.0, scale * (MH - 1) + 7.5)]
    for b in range(B):
        for t in range(T):
            pog[b, t] = kinds[(b * T + t + b) % len(kinds)]
    return pog


# ---------------------------------------------------------------------------------------------------------------- the kernels
def test_one_chunk_with_every_kind_of_frame():
    """B = 3, T = 5, explicit times, a carried non-zero map and state in every stream.
    stream 0: a deposit, a validity hole (decays only), a NaN point (decays only), a NaN time (ignored), a deposit;
    stream 1: lengths 0 and a reset flag: row and map cleared;
    stream 2: lengths 4: a deposit, a time that decreases (ignored), a deposit, a frame whose valid_key is 0, and a fifth frame past
              its length that holds NaNs."""
    B, T, (MW, MH) = 3, 5, (128, 72)
    screen = (1920, 1080)
    P = ref.params((MW, MH), 3.0, 0.999, floor=1e-8)
    state, maps = ref.fresh(B, MH, MW)
    rng = np.random.RandomState(3)
    pre = rng.uniform(0, 1, (B, 3, 2)).astype(np.float32) * np.float32([1920, 1080])
    ref.run(P, screen, state, maps, 3, pog=pre, frame_time=np.tile(np.arange(-3, 0) / 30.0, (B, 1)))
    assert (state[:, ref.HAS_PREV] == 1).all() and (maps.max(axis=(1, 2)) > 0.5).all()
    pog = (rng.uniform(0.1, 0.9, (B, T, 2)) * [1920, 1080]).astype(np.float32)
    frame_time = np.tile(np.arange(T) / 30.0, (B, 1))
    valid, valid_key = np.ones((B, T), dtype=np.uint8), np.ones((B, T), dtype=np.uint8)
    valid[0, 1] = 0
    pog[0, 2, 1] = np.nan
    frame_time[0, 3] = np.nan
    frame_time[2, 1] = -0.5
    valid_key[2, 3] = 0
    pog[2, 4], frame_time[2, 4] = np.nan, np.nan
    lengths, reset = [5, 0, 4], [0, 1, 0]
    before = maps.copy()
    frames = check(P, screen, state, maps, T, pog=pog, frame_time=frame_time, valid=valid, valid_key=valid_key, lengths=lengths, reset=reset,
                   per_frame=True)
    assert not maps[1].any() and not state[1].any() and state[:, ref.TICKS].tolist() == [8, 0, 7]
    assert frames[0, 3].tobytes() == frames[0, 2].tobytes() and frames[2, 1].tobytes() == frames[2, 0].tobytes()      # ignored frames
    assert (before > 0).all() and (frames[0, 1] < frames[0, 0]).all() and (frames[0, 2] < frames[0, 1]).all()      # decay alone
    assert (frames[0, 4] > frames[0, 3]).any()                           # ... and a deposit


@pytest.mark.parametrize('size,B,T', [((5, 3), 2, 3), ((1, 1), 2, 3), ((128, 72), 2, 3), ((131, 75), 2, 3), ((1024, 576), 1, 2)])
def test_map_shapes(size, B, T):
    MW, MH = size
    P = ref.params(size, 3.0, 0.999, fps=30.0)
    state, maps = ref.fresh(B, MH, MW)
    maps[:] = np.random.RandomState(MW).uniform(0, 2, maps.shape).astype(np.float32)
    check(P, (16 * MW, 16 * MH), state, maps, T, pog=centres(B, T, MW, MH), per_frame=True)
    assert state[:, ref.TICKS].tolist() == [T] * B


def test_a_clip_longer_than_a_pass_of_frames():
    """T = 70 on 16 x 9, counted time on carried ticks: past the plan's pass of 64 frames and the update's passes of 16."""
    B, T, (MW, MH) = 2, 70, (16, 9)
    P = ref.params((MW, MH), 1.5, 0.99, fps=60.0, weight='seconds')
    state, maps = ref.fresh(B, MH, MW)
    rng = np.random.RandomState(8)
    pog = (rng.uniform(-0.1, 1.1, (B, T, 2)) * [256, 144]).astype(np.float32)
    valid = (rng.uniform(size=(B, T)) > 0.2).astype(np.uint8)
    ref.run(P, (256, 144), state, maps, 5, pog=pog[:, :5])
    check(P, (256, 144), state, maps, T, pog=pog, valid=valid, lengths=[70, 67], per_frame=True)
    assert state[:, ref.TICKS].tolist() == [75, 72]


def test_no_frames_and_a_reset_flag_clear_and_write_nothing_else():
    B, (MW, MH) = 2, (37, 11)
    P = ref.params((MW, MH), 2.0, 0.999, fps=30.0)
    state, maps = ref.fresh(B, MH, MW)
    maps[:] = 1.25
    state[:] = [1.0, 0.5, 16.0, 0, 0, 0, 0, 0]
    check(P, (370, 110), state, maps, 0, reset=[0, 1])
    assert (maps[0] == 1.25).all() and not maps[1].any() and state[0, ref.TICKS] == 16 and not state[1].any()


@pytest.mark.parametrize('name,kw', [('seconds', dict(weight='seconds', normalize=True, floor=1e-8, decay_per_ms=1.0)),
                                     ('seconds_fps', dict(weight='seconds', fps=25.0, max_gap_s=0.02, decay_per_ms=0.995)),
                                     ('frame', dict(weight='frame', normalize=True, decay_per_ms=0.9))])
def test_weights_normalisation_floor_and_no_decay(name, kw):
    B, T, (MW, MH) = 2, 4, (40, 24)
    P = ref.params((MW, MH), 2.5, **kw)
    state, maps = ref.fresh(B, MH, MW)
    pog = centres(B, T, MW, MH)
    frame_time = np.array([[0.0, 0.03, 0.031, 0.5], [10.0, 10.04, 10.08, 10.12]])
    check(P, (16 * MW, 16 * MH), state, maps, T, pog=pog, frame_time=frame_time, per_frame=True)
    check(P, (16 * MW, 16 * MH), state, maps, T, pog=pog, frame_time=frame_time + 1.0)      # carried on


def test_a_ten_minute_gap_empties_the_map_exactly():
    B, (MW, MH) = 1, (32, 18)
    P = ref.params((MW, MH), 3.0, 0.999)
    state, maps = ref.fresh(B, MH, MW)
    pog = np.float32([[[256, 144], [256, 144], [100, 100]]])
    frames = check(P, (512, 288), state, maps, 3, pog=pog, frame_time=np.array([[0.0, 600.0, 600.01]]), valid=[[1, 0, 1]], per_frame=True)
    assert frames[0, 0].max() == 1.0 and not frames[0, 1].any() and np.isfinite(frames).all() and frames[0, 2].max() > 0.9


def test_the_heat_map_source():
    B, T, (MW, MH) = 2, 3, (128, 72)
    P = ref.params((MW, MH), 3.0, 0.999)
    state, maps = ref.fresh(B, MH, MW)
    heat = np.random.RandomState(12).uniform(0, 1, (B, T, MH, MW)).astype(np.float32)
    frame_time = np.array([[0.0, 0.033, 0.07], [5.0, 5.035, 5.066]])
    valid = np.array([[1, 1, 1], [1, 0, 1]], dtype=np.uint8)
    check(P, (1920, 1080), state, maps, T, heat=heat, frame_time=frame_time, valid=valid, per_frame=True)
    check(P, (1920, 1080), state, maps, T, heat=heat, frame_time=frame_time + 0.1)


def test_the_library_refuses_without_a_launch():
    k = default_kernels()
    state = torch.zeros((2, 8), dtype=torch.float64, device='cuda')
    maps = torch.zeros((2, 9, 16), dtype=torch.float32, device='cuda')
    P = ref.params((16, 9), 2.0, 0.999)
    with pytest.raises(RuntimeError, match='gaze_history_plan'):
        k.gaze_history_plan(dict(P, fps=None, max_gap_s=float('nan')), (256, 144), state, 0)
    with pytest.raises(RuntimeError, match='gaze_history_plan'):
        k.gaze_history_plan(dict(P, ln_decay=0.5, fps=30.0), (256, 144), state, 0)
    coef, clear = k.gaze_history_plan(P, (256, 144), state, 0)
    with pytest.raises(RuntimeError, match='gaze_history_update'):
        k.gaze_history_update(dict(P, alpha=0.0), coef, clear, maps)
    with pytest.raises(RuntimeError, match='gaze_history_update'):
        k.gaze_history_update(dict(P, floor=-1.0), coef, clear, maps)
    with pytest.raises(ValueError, match='fps'):
        k.gaze_history_plan(P, (256, 144), state, 2, pog=torch.zeros((2, 2, 2), device='cuda'))
    with pytest.raises(TypeError, match='maps'):
        k.gaze_history_update(P, coef, clear, maps[:, :8])


def test_the_stand_alone_entry():
    S, T, (MW, MH) = 2, 6, (64, 36)
    spec = GazeHistorySpec(size=(MW, MH), sigma=2.0, decay_per_ms=0.998, fps=30.0, per_frame=True, name='dwell')
    pog = (np.random.RandomState(4).uniform(0, 1, (S, T, 2)) * [1920, 1080]).astype(np.float32)
    valid = np.ones((S, T), dtype=bool)
    valid[1, 2] = False
    out = data.gaze_history(spec, (1920, 1080), pog_px=cuda(pog), valid=cuda(valid))
    state, maps = ref.fresh(S, MH, MW)
    frames = ref.run(ref.spec_params(spec), (1920, 1080), state, maps, T, pog=pog, valid=valid, per_frame=True)
    assert sorted(out) == ['dwell', 'dwell_frames', 'state']
    assert out['dwell'].cpu().numpy().tobytes() == maps.tobytes() and out['dwell_frames'].cpu().numpy().tobytes() == frames.tobytes()
    assert out['state'].cpu().numpy().tobytes() == state.tobytes()


# ---------------------------------------------------------------------------------------------------------------- EVEStream
S, TC = 3, 6
TIMES = np.cumsum(np.random.RandomState(2).uniform(0.030, 0.037, (S, TC)), axis=1) + np.arange(S)[:, None] * 50.0


@pytest.fixture(scope='module')
def rig():
    """One model and one 3 x 6 clip, shared and never modified."""
    model, _ = make_model(refine_net_rnn_type='CGRU')
    _, d, _ = gpu_clip(S, TC, seed=11)
    d = dict(d, frame_time=cuda(TIMES))
    chunk = lambda t0, t1: {k: v[:, t0:t1].contiguous() for k, v in d.items()}
    return {'model': model, 'clip': d, 'chunk': chunk}


def keep(out):
    return {k: v.clone() for k, v in out.items()}


def reference_on(model, spec, outs, chunks, source='PoG_px_final', lengths=None, valid_key=None):
    """The contract fed with the steps' own source, `valid` and frame_time, carried from step to step.  -> (state, maps, [frames])."""
    P = ref.spec_params(spec, model.config)
    MW, MH = P['size']
    state, maps = ref.fresh(S, MH, MW)
    frames = []
    for i, (out, chunk) in enumerate(zip(outs, chunks)):
        T = chunk['frame_time'].shape[1]
        n = lambda t: None if t is None else t.cpu().numpy()
        src = out[source]
        frames.append(ref.run(P, tuple(model.config.actual_screen_size), state, maps, T,
                              pog=None if source == 'heatmap_final' else n(src.float()),
                              heat=n(src.float().reshape(S, T, MH, MW)) if source == 'heatmap_final' else None,
                              frame_time=n(chunk['frame_time']), valid=n(out.get('valid')) if 'eye_valid' in out else None,
                              valid_key=None if valid_key is None else n(out[valid_key]),
                              lengths=None if lengths is None else lengths[i], per_frame=True))
    return state, maps, frames


def test_stream_history_eager_captured_and_in_chunks(rig):
    model, chunk = rig['model'], rig['chunk']
    spec = GazeHistorySpec(per_frame=True, floor=1e-8)
    whole = [chunk(0, 6)]
    eager, graph = eve_amd.EVEStream(model, S, use_graph=False), eve_amd.EVEStream(model, S)
    e = keep(eager.step(whole[0], history=spec))
    g = keep(graph.step(whole[0], history=spec))
    assert sorted(e) == sorted(g) and 'gaze_history' in e and tuple(e['gaze_history_frames'].shape) == (S, 6, 72, 128)
    for k_ in e:
        assert e[k_].cpu().numpy().tobytes() == g[k_].cpu().numpy().tobytes(), k_
    state, maps, frames = reference_on(model, spec, [e], whole)
    assert e['gaze_history'].cpu().numpy().tobytes() == maps.tobytes() and e['gaze_history_frames'].cpu().numpy().tobytes() == frames[0].tobytes()
    assert maps.min() > 0                                                # (the floor of six frames)
    for s_ in (eager, graph):                                            # (the capture's warm-up steps left map and rows alone)
        assert s_.gaze_history().cpu().numpy().tobytes() == maps.tobytes()
        assert s_.get_gaze_history_state()['gaze_history']['rows'].cpu().numpy().tobytes() == state.tobytes()
    # chunks of 2 + 3 + 1; the point of gaze of a chunked pass equals the whole pass's, so do the maps
    parts = eve_amd.EVEStream(model, S)
    outs = [keep(parts.step(chunk(a, b), history=spec)) for a, b in ((0, 2), (2, 5), (5, 6))]
    assert torch.equal(torch.cat([o['PoG_px_final'] for o in outs], dim=1), e['PoG_px_final'])
    assert torch.equal(torch.cat([o['gaze_history_frames'] for o in outs], dim=1), e['gaze_history_frames'])
    assert torch.equal(outs[-1]['gaze_history'], e['gaze_history']) and torch.equal(outs[0]['gaze_history'], e['gaze_history_frames'][:, 1])
    # a carried map survives the warm-up and capture of another chunk shape (above: three shapes on one map); reset([1]) clears stream 1 only
    parts.reset([1])
    again = keep(parts.step(chunk(0, 2), history=spec))
    assert torch.equal(again['gaze_history'][1], outs[0]['gaze_history'][1]) and not torch.equal(again['gaze_history'][0], outs[0]['gaze_history'][0])
    rows = parts.get_gaze_history_state()['gaze_history']['rows'].cpu().numpy()
    assert rows[:, ref.TICKS].tolist() == [8, 2, 8]
    parts.reset([0])                                                     # ... and before a step without history=
    parts.step(chunk(0, 2))
    assert not parts.gaze_history()[0].any() and torch.equal(parts.gaze_history()[1:], again['gaze_history'][1:])


@pytest.mark.parametrize('mode', ['lengths', 'eye_mask', 'fixations', 'two_specs'])
def test_stream_history_combines(rig, mode):
    model, chunk = rig['model'], rig['chunk']
    chunks = [chunk(0, 3), chunk(3, 6)]
    spec, kw, lengths, source, valid_key = GazeHistorySpec(per_frame=True), {}, None, 'PoG_px_final', None
    if mode == 'lengths':
        lengths = [[3, 0, 2], [3, 3, 1]]
    elif mode == 'eye_mask':
        mask = torch.ones((S, 3, 2), dtype=torch.bool, device='cuda')
        mask[0, 1] = False
        mask[2, :, 0] = False
        kw = dict(eye_mask=mask)
    elif mode == 'fixations':
        spec = GazeHistorySpec(name='fix_map', source='fixation_px', valid_key='fixating', weight='seconds', decay_per_ms=1.0, normalize=True,
                               per_frame=True)
        kw, source, valid_key = dict(events=GazeEventSpec(saccade_deg_s=1e9, min_fixation_s=0.03)), 'fixation_px', 'fixating'
    outs = {}
    for name, use_graph in (('eager', False), ('graph', True)):
        s_ = eve_amd.EVEStream(model, S, use_graph=use_graph)
        history = [spec, GazeHistorySpec(name='refined', source='heatmap_final', decay_per_ms=0.99)] if mode == 'two_specs' else spec
        outs[name] = [keep(s_.step(c, history=history, **dict(kw, **({} if lengths is None else {'lengths': lengths[i]}))))
                      for i, c in enumerate(chunks)]
    for e, g in zip(outs['eager'], outs['graph']):
        where = e['valid'] if 'valid' in e else None
        for k_ in (spec.name, spec.name + '_frames') + (('refined',) if mode == 'two_specs' else ()):
            a, b = e[k_], g[k_]
            if k_.endswith('_frames') and where is not None and mode == 'lengths':
                a, b = a[where], b[where]
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), k_
    state, maps, frames = reference_on(model, spec, outs['eager'], chunks, source=source, lengths=lengths, valid_key=valid_key)
    last = outs['eager'][-1]
    assert last[spec.name].cpu().numpy().tobytes() == maps.tobytes()
    if mode != 'lengths':
        assert last[spec.name + '_frames'].cpu().numpy().tobytes() == frames[-1].tobytes()
    if mode == 'fixations':
        assert maps.sum() > 0
    if mode == 'two_specs':
        with_hm = [keep(eve_amd.EVEStream(model, S, use_graph=False).step(chunks[0], return_heatmaps=True))]
        spec2 = GazeHistorySpec(name='refined', source='heatmap_final', decay_per_ms=0.99)
        _, maps2, _ = reference_on(model, spec2, with_hm, chunks[:1], source='heatmap_final')
        assert outs['eager'][0]['refined'].cpu().numpy().tobytes() == maps2.tobytes()


def test_stream_history_feeds_the_overlay(rig):
    model, chunk = rig['model'], rig['chunk']
    cap = nv12_capture(44, B=S, T=3)
    c = dict({k_: v for k_, v in chunk(0, 3).items() if k_ != 'screen_frame'}, screen_frame_nv12=cap)
    spec = GazeHistorySpec(name='trail', per_frame=True)
    overlay = OverlaySpec(markers=[], inset=None, out_format='rgb', heat=False, heat_key='trail')
    e = keep(eve_amd.EVEStream(model, S, use_graph=False).step(c, history=spec, render=overlay))
    g = keep(eve_amd.EVEStream(model, S).step(c, history=spec, render=overlay))
    assert torch.equal(e['rendered'], g['rendered'])
    N = S * 3
    heat = dict(heat=e['trail_frames'].reshape(N, 72, 128).cpu().numpy(), color=overlay.heat_color, amax=overlay.heat_amax)
    want = oref.render(cap.reshape((N,) + tuple(cap.shape[2:])).cpu().numpy(), 'nv12', 'rgb', 'bt601', None, heat, None, None)
    assert np.array_equal(e['rendered'].reshape(want.shape).cpu().numpy(), want)
    bare = oref.render(cap.reshape((N,) + tuple(cap.shape[2:])).cpu().numpy(), 'nv12', 'rgb', 'bt601', None, None, None, None)
    assert not np.array_equal(want, bare)
