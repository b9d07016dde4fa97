"""CPU: the time-decayed gaze history -- the numpy contract (tests/gaze_history_ref.py) against np.exp, against the project's
restatement of the reference (oracle.eve.gaze_history_maps) and under chunk splits, eve_amd.GazeHistorySpec, and the EVEStream plumbing
(step(history=...), the refusals, the graph key, reset, the carried state, the overlay's heat_key) over a stand-in whose two calls are
the reference itself.  The GPU suite (test_gpu_gaze_history.py) checks the HIP kernels."""
import itertools
import math
import types

import numpy as np
import pytest
import torch

import eve_amd
import gaze_history_ref as ref
from eve_amd import kernels
from eve_amd.data import GazeEventSpec, GazeHistorySpec, OverlaySpec
from oracle import eve as oracle_eve
from test_gaze_events_host import EventOverlayFakes
from test_overlay_host import stream_chunk
from test_stream_host import chunk_of, clip, make_model

SCREEN = (1920, 1080)


# ---------------------------------------------------------------------------------------------------------------- gh_exp
def test_gh_exp_against_numpy():
    """At most 8 ulp of float64 (2^-50 relative) on a grid of [-104, 0]: four times the 2.0 ulp a probe over 5.1 M points found."""
    rng = np.random.RandomState(0)
    x = np.concatenate([-np.linspace(0.0, 104.0, 200001), -rng.uniform(0, 104, 200000), -rng.uniform(0, 1e-3, 20000), [-104.0, -1e-300]])
    got, want = ref.gh_exp(x), np.exp(x)
    rel = np.abs(got - want) / want
    print('gh_exp: worst %.3f ulp' % (rel.max() / 2.0 ** -53))
    assert rel.max() <= 2.0 ** -50
    assert ref.gh_exp(0.0) == 1.0 and ref.gh_exp(-0.0) == 1.0
    assert (ref.gh_exp(np.array([-104.0000001, -1e3, -1e300, -np.inf])) == 0.0).all() and ref.gh_exp(-104.0) > 0


# ---------------------------------------------------------------------------------------------------------------- the reference's maps
def oracle_config(size=(128, 72), decay=0.999):
    return types.SimpleNamespace(gaze_heatmap_size=list(size), actual_screen_size=list(SCREEN), gaze_history_map_decay_per_ms=decay)


def recording(B, T, seed):
    rng = np.random.RandomState(seed)
    timestamps = (1_000_000_000 + np.cumsum(rng.randint(30_000_000, 37_000_001, (B, T)), axis=1)).astype(np.int64)
    pog = (rng.uniform(0.05, 0.95, (B, T, 2)) * SCREEN).astype(np.float32)
    validity = rng.uniform(size=(B, T)) > 0.25
    validity[0, -1] = False                              # the clip's last frame among the holes
    return timestamps, pog, validity


def within_four_yardsticks(got, want64, got32):
    """tests/test_gpu_harness_f64.py's rule: at most 4 x the error of the float32 oracle against the float64 one, that yardstick floored
    at 2^-24 of the map's maximum."""
    err = np.abs(got.astype(np.float64) - want64).max()
    yardstick = max(np.abs(got32.astype(np.float64) - want64).max(), 2.0 ** -24 * np.abs(want64).max())
    print('err %.3e  yardstick %.3e  ratio %.3f' % (err, yardstick, err / yardstick))
    return err <= 4.0 * yardstick


@pytest.mark.parametrize('source', ['pog', 'heat'])
def test_the_recurrence_is_the_reference_windowed_sum(source):
    B, T, (MW, MH) = 2, 30, (128, 72)
    cfg = oracle_config()
    timestamps, pog, validity = recording(B, T, seed=5)
    P = ref.params((MW, MH), 3.0, 0.999, floor=1e-8)
    state, maps = ref.fresh(B, MH, MW)
    ts, val = torch.from_numpy(timestamps), torch.from_numpy(validity)
    if source == 'pog':
        ref.run(P, SCREEN, state, maps, T, pog=pog, frame_time=timestamps * 1e-9, valid=validity)
        heat = lambda dtype: oracle_eve.make_heatmaps(torch.from_numpy(pog).reshape(B * T, 2).to(dtype), 3.0, cfg).view(B, T, 1, MH, MW)
    else:
        hm = np.random.RandomState(6).uniform(0, 1, (B, T, MH, MW)).astype(np.float32)
        ref.run(P, SCREEN, state, maps, T, heat=hm, frame_time=timestamps * 1e-9, valid=validity)
        heat = lambda dtype: torch.from_numpy(hm).view(B, T, 1, MH, MW).to(dtype)
    want64 = oracle_eve.gaze_history_maps(ts, heat(torch.float64), val, cfg).numpy()[:, 0]
    got32 = oracle_eve.gaze_history_maps(ts, heat(torch.float32), val, cfg).numpy()[:, 0]
    assert want64.dtype == np.float64 and got32.dtype == np.float32 and want64.max() > 1.0
    assert within_four_yardsticks(maps, want64, got32)


# ---------------------------------------------------------------------------------------------------------------- chunk splits
def compositions(n):
    for cuts in itertools.product([0, 1], repeat=n - 1):
        parts, last = [], 0
        for i, c in enumerate(cuts, 1):
            if c:
                parts.append(i - last)
                last = i
        yield parts + [n - last]


@pytest.mark.parametrize('timed', [True, False])
def test_every_split_of_a_clip_gives_the_bits_of_one_pass(timed):
    B, T, (MW, MH) = 2, 7, (24, 13)
    rng = np.random.RandomState(9)
    pog = (rng.uniform(-0.1, 1.1, (B, T, 2)) * SCREEN).astype(np.float32)
    valid = rng.uniform(size=(B, T)) > 0.3
    pog[1, 3, 0] = np.nan
    frame_time = np.cumsum(rng.uniform(0.02, 0.05, (B, T)), axis=1) if timed else None
    if timed:
        frame_time[0, 4] = frame_time[0, 2]              # a time that does not advance past frame 3's: ignored
    P = ref.params((MW, MH), 2.0, 0.99, weight='seconds', fps=None if timed else 30.0, normalize=True)
    state, maps = ref.fresh(B, MH, MW)
    frames = ref.run(P, SCREEN, state, maps, T, pog=pog, frame_time=frame_time, valid=valid, per_frame=True)
    assert maps.any() and len(list(compositions(T))) == 64
    for parts in compositions(T):
        s2, m2 = ref.fresh(B, MH, MW)
        got, t0 = [], 0
        for n in parts:
            got.append(ref.run(P, SCREEN, s2, m2, n, pog=pog[:, t0:t0 + n], frame_time=None if frame_time is None else frame_time[:, t0:t0 + n],
                               valid=valid[:, t0:t0 + n], per_frame=True))
            t0 += n
        assert m2.tobytes() == maps.tobytes() and s2.tobytes() == state.tobytes(), parts
        assert np.concatenate(got, axis=1).tobytes() == frames.tobytes(), parts


# ---------------------------------------------------------------------------------------------------------------- semantics
def one_stream(P, T, pog, size, **kw):
    state, maps = ref.fresh(1, size[1], size[0])
    frames = ref.run(P, SCREEN, state, maps, T, pog=np.asarray(pog, dtype=np.float32).reshape(1, T, 2), per_frame=True, **kw)
    return state, maps, frames[0]


def test_invalid_nan_and_out_of_order_frames():
    size = (32, 18)
    P = ref.params(size, 2.0, 0.99)
    centre = [960.0, 540.0]
    ft = np.array([[0.0, 0.03, 0.06, 0.09]])
    # an invalid frame decays and deposits nothing
    _, _, f = one_stream(P, 4, [centre] * 4, size, frame_time=ft, valid=[[1, 0, 1, 1]])
    d = ref.gh_exp(30.0 * math.log(0.99))
    assert np.array_equal(f[1], (f[0].astype(np.float64) * d).astype(np.float32)) and f[2].max() > f[1].max()
    # a NaN point leaves no NaN, and counts as a tick of the time chain
    state, maps, f = one_stream(P, 4, [centre, [np.nan, 540.0], [960.0, np.inf], centre], size, frame_time=ft)
    assert np.isfinite(f).all() and np.array_equal(f[1], (f[0].astype(np.float64) * d).astype(np.float32)) and state[0, ref.T_PREV] == 0.09
    # a decreasing or NaN time is ignored: the map as it stands, t_prev stays, the tick counts
    state, maps, f = one_stream(P, 4, [centre] * 4, size, frame_time=np.array([[0.0, np.nan, -1.0, 0.03]]))
    assert np.array_equal(f[1], f[0]) and np.array_equal(f[2], f[0]) and state[0].tolist()[:3] == [1.0, 0.03, 4.0]
    s1, m1, _ = one_stream(P, 2, [centre] * 2, size, frame_time=np.array([[0.0, 0.03]]))
    assert m1.tobytes() == maps.tobytes()
    # an equal time is not a decreasing one: no decay, a second deposit
    _, _, f = one_stream(P, 2, [centre] * 2, size, frame_time=np.array([[1.0, 1.0]]))
    assert f[1].max() == 2.0
    # a frame past its length is ignored, and does not tick
    state, maps, f = one_stream(P, 4, [centre] * 4, size, frame_time=ft, lengths=[2])
    assert state[0].tolist()[:3] == [1.0, 0.03, 2.0] and maps.tobytes() == f[1].tobytes()


def test_a_dwell_map_sums_to_the_seconds_watched():
    size = (64, 36)
    T, fps = 40, 50.0
    P = ref.params(size, 2.0, 1.0, weight='seconds', normalize=True, fps=fps)
    pog = np.tile([[960.0, 540.0]], (T, 1)) + np.random.RandomState(1).uniform(-300, 300, (T, 2))       # 12 sigma inside the map
    _, maps, _ = one_stream(P, T, pog, size)
    assert abs(maps.astype(np.float64).sum() - T / fps) <= 1e-6 * (T / fps)
    # max_gap_s caps the deposit: a 2 s hole deposits 0.075 s
    ft = np.array([[0.0, 0.02, 2.02, 2.04]])
    _, maps, _ = one_stream(ref.params(size, 2.0, 1.0, weight='seconds', normalize=True), 4, pog[:4], size, frame_time=ft)
    assert abs(maps.astype(np.float64).sum() - (0.0 + 0.02 + 0.075 + 0.02)) <= 1e-6 * 0.115


def test_reset_clears_with_and_without_frames():
    size = (16, 9)
    P = ref.params(size, 2.0, 0.999, fps=30.0)
    state, maps = ref.fresh(2, 9, 16)
    pog = np.full((2, 3, 2), 500.0, dtype=np.float32)
    ref.run(P, SCREEN, state, maps, 3, pog=pog)
    filled = maps.copy()
    ref.run(P, SCREEN, state, maps, 0, reset=[0, 1])
    assert np.array_equal(maps[0], filled[0]) and not maps[1].any() and state[:, ref.TICKS].tolist() == [3, 0]
    ref.run(P, SCREEN, state, maps, 3, pog=pog, reset=[1, 0])
    assert maps[0].tobytes() == filled[0].tobytes() and maps[1].tobytes() == filled[1].tobytes()
    ref.run(P, SCREEN, state, maps, 3, pog=pog, reset=[1, 0], lengths=[0, 0])
    assert not maps[0].any() and not state[0].any() and maps[1].tobytes() == filled[1].tobytes()


# ---------------------------------------------------------------------------------------------------------------- the spec
def test_the_spec_compares_by_value_and_refuses_bad_numbers():
    a, b_ = GazeHistorySpec(fps=30, sigma=3), GazeHistorySpec(fps=30.0, sigma=3.0)
    assert a == b_ and hash(a) == hash(b_) and a != GazeHistorySpec(fps=60, sigma=3) and a != GazeHistorySpec(fps=30, sigma=3, per_frame=True)
    assert a != GazeHistorySpec(fps=30, sigma=3, name='other') and a != 30 and len({a, b_, GazeHistorySpec()}) == 2
    assert eve_amd.GazeHistorySpec is GazeHistorySpec
    d = GazeHistorySpec()
    assert d.key() == ('gaze_history', None, None, None, None, None, 'frame', 0.075, None, 0.0, False, False)
    assert d.resolved(types.SimpleNamespace(gaze_heatmap_size=[128, 72], gaze_heatmap_sigma_history=3.0, gaze_history_map_decay_per_ms=0.999)) == \
        ((128, 72), 3.0, 0.999)
    P = GazeHistorySpec(size=(40, 20), sigma=2.0, decay_per_ms=0.5, normalize=True, weight='seconds', fps=25).launch_params()
    assert P == ref.params((40, 20), 2.0, 0.5, 'seconds', 0.075, 25.0, 0.0, True)
    for name, bads in (('sigma', (0, -1.0, float('nan'), float('inf'), '3', True)), ('decay_per_ms', (0, 1.0001, -0.5, float('nan'), True)),
                       ('max_gap_s', (0, -1.0, float('nan'), float('inf'))), ('fps', (0, -30, float('nan'), '30')),
                       ('floor', (-1e-9, float('nan'), float('inf'), None)), ('size', ((0, 5), (5, 2049), (5,), 5, (5.0, 3), (True, 3))),
                       ('weight', ('time', None)), ('source', ('PoG_cm_final', 'heatmap_initial')), ('name', ('', None, 3)),
                       ('valid_key', ('', 3))):
        for bad in bads:
            with pytest.raises(ValueError, match=name):
                GazeHistorySpec(**{name: bad})
    assert GazeHistorySpec(decay_per_ms=1).decay_per_ms == 1.0 and GazeHistorySpec(size=[2048, 1]).size == (2048, 1)


# ---------------------------------------------------------------------------------------------------------------- EVEStream
class HistoryFakes(EventOverlayFakes):
    """The events' and the overlay's stand-ins plus the two gaze history calls, evaluated by tests/gaze_history_ref.py: the plan keeps its
    inputs for the update, which runs the reference on the carried rows and maps."""

    def gaze_history_plan(self, P, screen_size, state, T, pog=None, frame_time=None, valid=None, valid_key=None, lengths=None, reset=None):
        self.calls.append('gaze_history_plan')
        n = lambda t: None if t is None else t.detach().numpy().copy()
        coef = torch.zeros((state.shape[0], T, 4), dtype=torch.float64)
        self._planned = (id(coef), dict(screen=tuple(screen_size), state=state, T=T, pog=n(pog), frame_time=n(frame_time), valid=n(valid),
                                        valid_key=n(valid_key), lengths=n(lengths), reset=n(reset)))
        return coef, torch.zeros((state.shape[0],), dtype=torch.int32)

    def gaze_history_update(self, P, coef, clear, maps, heat=None, per_frame=False):
        self.calls.append('gaze_history_update')
        token, a = self._planned
        assert token == id(coef)
        frames = ref.run(P, a['screen'], a['state'].numpy(), maps.numpy(), a['T'], pog=a['pog'], heat=None if heat is None else heat.numpy(),
                         frame_time=a['frame_time'], valid=a['valid'], valid_key=a['valid_key'], lengths=a['lengths'], reset=a['reset'],
                         per_frame=per_frame)
        return torch.from_numpy(frames) if per_frame else None


NEW_CALLS = ('gaze_history_plan', 'gaze_history_update')


@pytest.fixture()
def fake():
    k = HistoryFakes()
    kernels.set_default_kernels(k)
    yield k
    kernels.set_default_kernels(None)
    eve_amd.reset_standalone_config()


B, T = 2, 3


@pytest.fixture()
def scene(fake):
    model, _ = make_model(dict(refine_net_rnn_type='CGRU'))
    batch = clip(B, 2 * T, size=32)
    return model, chunk_of(batch, 0, T), chunk_of(batch, T, 2 * T)


def run(stream, chunk, **kw):
    return {k: v.clone() for k, v in stream.step(chunk, **kw).items()}


def reference_on(model, spec, out, source, state, maps, **kw):
    P = ref.spec_params(spec, model.config)
    src = out[source].numpy()
    heat = source == 'heatmap_final'
    return ref.run(P, tuple(model.config.actual_screen_size), state, maps, src.shape[1], pog=None if heat else src,
                   heat=src.reshape(src.shape[:2] + src.shape[-2:]) if heat else None, per_frame=True, **kw)


def test_a_step_with_history_adds_the_map_and_two_launches(fake, scene):
    model, c0, c1 = scene
    MW, MH = model.config.gaze_heatmap_size
    plain = run(eve_amd.EVEStream(model, B, use_graph=False), c0)
    calls_plain = list(fake.calls)
    assert not set(NEW_CALLS) & set(calls_plain)
    del fake.calls[:]
    s = eve_amd.EVEStream(model, B, use_graph=False)
    spec = GazeHistorySpec(fps=30, per_frame=True)
    out = run(s, c0, history=spec)
    assert fake.calls == calls_plain + list(NEW_CALLS)                   # the plain step's launches, then the two
    assert sorted(out) == sorted(list(plain) + ['gaze_history', 'gaze_history_frames'])
    for k in plain:
        assert torch.equal(out[k], plain[k]), k
    assert tuple(out['gaze_history'].shape) == (B, MH, MW) and out['gaze_history'].dtype == torch.float32
    assert tuple(out['gaze_history_frames'].shape) == (B, T, MH, MW)
    state, maps = ref.fresh(B, MH, MW)
    frames = reference_on(model, spec, out, 'PoG_px_final', state, maps)
    assert out['gaze_history'].numpy().tobytes() == maps.tobytes() and out['gaze_history_frames'].numpy().tobytes() == frames.tobytes()
    out1 = run(s, c1, history=spec)                                      # carried into the second step
    reference_on(model, spec, out1, 'PoG_px_final', state, maps)
    assert out1['gaze_history'].numpy().tobytes() == maps.tobytes() and s.gaze_history().numpy().tobytes() == maps.tobytes()
    assert s.get_gaze_history_state()['gaze_history']['rows'].numpy().tobytes() == state.tobytes() and state[0, ref.TICKS] == 2 * T
    # a step without history afterwards: the plain step's calls, names and order, and the map untouched
    del fake.calls[:]
    back = run(s, c0)
    assert fake.calls == calls_plain and sorted(back) == sorted(plain) and s.gaze_history().numpy().tobytes() == maps.tobytes()
    # the chunk's frame_time wins over fps; an explicit source
    ft = torch.tensor([[0.0, 0.011, 0.019], [5.0, 5.5, 5.51]], dtype=torch.float64)
    spec2 = GazeHistorySpec(name='initial', source='PoG_px_initial', fps=30, decay_per_ms=0.99)
    out2 = run(eve_amd.EVEStream(model, B, use_graph=False), dict(c0, frame_time=ft), history=spec2)
    state2, maps2 = ref.fresh(B, MH, MW)
    reference_on(model, spec2, out2, 'PoG_px_initial', state2, maps2, frame_time=ft.numpy())
    assert out2['initial'].numpy().tobytes() == maps2.tobytes() and 'initial_frames' not in out2 and state2[1, ref.T_PREV] == 5.51


def test_history_on_ragged_masked_and_event_steps_and_two_specs(fake, scene):
    model, c0, _ = scene
    MW, MH = model.config.gaze_heatmap_size
    spec = GazeHistorySpec(fps=30)
    s = eve_amd.EVEStream(model, B, use_graph=False)
    out = run(s, c0, history=spec, lengths=[2, 0])
    state, maps = ref.fresh(B, MH, MW)
    reference_on(model, spec, out, 'PoG_px_final', state, maps, lengths=[2, 0])
    assert out['gaze_history'].numpy().tobytes() == maps.tobytes() and not maps[1].any() and state[:, ref.TICKS].tolist() == [2, 0]
    mask = torch.ones(B, T, 2, dtype=torch.bool)
    mask[0, 1] = False
    mask[1, :, 0] = False
    out = run(eve_amd.EVEStream(model, B, use_graph=False), c0, history=spec, eye_mask=mask)
    state, maps = ref.fresh(B, MH, MW)
    reference_on(model, spec, out, 'PoG_px_final', state, maps, valid=out['valid'].numpy())
    assert out['gaze_history'].numpy().tobytes() == maps.tobytes() and state[:, ref.TICKS].tolist() == [T, T]
    # the fixation heat map, beside the network's own maps accumulated: two specs, four launches after the events'
    events = GazeEventSpec(fps=30, saccade_deg_s=1e9, min_fixation_s=0.02)
    fix = GazeHistorySpec(name='fix', source='fixation_px', valid_key='fixating', weight='seconds', decay_per_ms=1.0, fps=30)
    net = GazeHistorySpec(name='refined', source='heatmap_final', fps=30, floor=0.0)
    del fake.calls[:]
    out = run(eve_amd.EVEStream(model, B, use_graph=False), c0, history=[fix, net], events=events, return_heatmaps=True)
    assert fake.calls[-5:] == ['gaze_events'] + list(NEW_CALLS) * 2
    state, maps = ref.fresh(B, MH, MW)
    reference_on(model, fix, out, 'fixation_px', state, maps, valid_key=out['fixating'].numpy())
    assert out['fix'].numpy().tobytes() == maps.tobytes() and maps.any() and out['fixating'].sum() < B * T
    state, maps = ref.fresh(B, MH, MW)
    reference_on(model, net, out, 'heatmap_final', state, maps)
    assert out['refined'].numpy().tobytes() == maps.tobytes()


def test_refusals_come_before_any_launch(fake, scene):
    model, c0, _ = scene
    s = eve_amd.EVEStream(model, B, use_graph=False)
    spec = GazeHistorySpec(fps=30)
    for bad, match in ((dict(fps=30), 'GazeHistorySpec'), ([], 'GazeHistorySpec'), ([spec] * 3, 'GazeHistorySpec'),
                       ([spec, GazeHistorySpec(fps=60)], 'share the name'), (GazeHistorySpec(), 'frame_time'),
                       (GazeHistorySpec(fps=30, source='PoG_px_filtered'), 'events'), (GazeHistorySpec(fps=30, source='fixation_px'), 'events'),
                       (GazeHistorySpec(fps=30, valid_key='fixating'), 'valid_key'), (GazeHistorySpec(fps=30, valid_key='left_o'), 'valid_key'),
                       (GazeHistorySpec(fps=30, name='PoG_px_final'), 'name'),
                       (GazeHistorySpec(fps=30, source='heatmap_final', size=(16, 9)), 'gaze_heatmap_size')):
        with pytest.raises(ValueError, match=match):
            s.step(c0, history=bad)
    for bad in (torch.zeros(B, T), torch.zeros(B, T + 1, dtype=torch.float64)):
        with pytest.raises(ValueError, match='frame_time'):
            s.step(dict(c0, frame_time=bad), history=spec)
    with pytest.raises(ValueError, match='inv_camera_transformation'):
        s.step({k: v for k, v in c0.items() if k != 'inv_camera_transformation'}, history=spec)
    with pytest.raises(ValueError, match='no gaze history map'):
        s.gaze_history('nothing')
    assert fake.calls == [] and s._history == {}
    eye_only, _ = make_model(dict(refine_net_enabled=False))
    s = eve_amd.EVEStream(eye_only, B, use_graph=False)
    for source in ('PoG_px_final', 'heatmap_final'):
        with pytest.raises(ValueError, match='RefineNet'):
            s.step(c0, history=GazeHistorySpec(fps=30, source=source))
    assert fake.calls == []
    out = s.step({k: v for k, v in c0.items() if k != 'screen_frame'}, history=spec)      # source None without a RefineNet
    MW, MH = eye_only.config.gaze_heatmap_size
    state, maps = ref.fresh(B, MH, MW)
    reference_on(eye_only, spec, out, 'PoG_px_initial', state, maps)
    assert out['gaze_history'].numpy().tobytes() == maps.tobytes()
    # a map is tied to its spec
    with pytest.raises(ValueError, match='clear_gaze_history'):
        s.step(c0, history=GazeHistorySpec(fps=30, decay_per_ms=0.5))
    s.clear_gaze_history('gaze_history')
    assert not s.gaze_history().any()
    s.step({k: v for k, v in c0.items() if k != 'screen_frame'}, history=GazeHistorySpec(fps=30, decay_per_ms=0.5))


def test_the_graph_key_holds_the_spec(fake, scene):
    model, c0, _ = scene
    s = eve_amd.EVEStream(model, B, use_graph=False)
    plan = lambda *specs: s._check_history(c0, list(specs), None, False, B, T)
    bare = s._graph_key(c0, False)
    a = s._graph_key(c0, False, history=plan(GazeHistorySpec(fps=30)))
    assert a != bare and a == s._graph_key(dict(c0), False, history=plan(GazeHistorySpec(fps=30.0)))
    assert a != s._graph_key(c0, False, history=plan(GazeHistorySpec(fps=30, name='b')))
    s.clear_gaze_history()
    assert a != s._graph_key(c0, False, history=plan(GazeHistorySpec(fps=30, per_frame=True)))
    s.clear_gaze_history()
    assert a != s._graph_key(c0, False, history=plan(GazeHistorySpec(fps=30, source='PoG_px_initial')))
    s.clear_gaze_history()
    two = s._graph_key(c0, False, history=plan(GazeHistorySpec(fps=30), GazeHistorySpec(fps=30, name='b')))
    assert two != a
    captured = []
    s._capture = lambda chunk, *a_, **k_: captured.append((a_, k_)) or {'n': len(captured)}
    first = s._graph_for(c0, False, history=plan(GazeHistorySpec(fps=30)))
    assert s._graph_for(c0, False, history=plan(GazeHistorySpec(fps=30))) is first and len(captured) == 1 and 'history' in captured[0][1]
    assert s._graph_for(c0, False) is not first and len(captured) == 2 and captured[1] == ((False, False, False, None), {})


def test_reset_clear_and_the_state_round_trip(fake, scene):
    model, c0, c1 = scene
    spec = GazeHistorySpec(fps=30)
    s = eve_amd.EVEStream(model, B, use_graph=False)
    first = run(s, c0, history=spec)
    s.reset([1])
    second = run(s, c1, history=spec)
    alone = run(eve_amd.EVEStream(model, B, use_graph=False), c1, history=spec)
    assert s.get_gaze_history_state()['gaze_history']['rows'][:, ref.TICKS].tolist() == [2 * T, T]
    assert not torch.equal(second['gaze_history'][0], first['gaze_history'][0])
    # (stream 1 restarted its recurrent state too, so its point of gaze is the second chunk's from zero state)
    state, maps = ref.fresh(B, *reversed(model.config.gaze_heatmap_size))
    reference_on(model, spec, second, 'PoG_px_final', state, maps)
    assert second['gaze_history'][1].numpy().tobytes() == maps[1].tobytes() and alone is not None
    # a reset before a step WITHOUT history still clears the flagged stream: the two launches with no frames, then the plain step
    s.reset([0])
    del fake.calls[:]
    run(s, c0)
    assert fake.calls[:2] == list(NEW_CALLS) and fake.calls.count('gaze_history_plan') == 1
    assert not s.gaze_history()[0].any() and torch.equal(s.gaze_history()[1], second['gaze_history'][1])
    rows = s.get_gaze_history_state()['gaze_history']['rows']
    assert not rows[0].any() and rows[1, ref.TICKS] == T
    # clear_gaze_history by stream; get / set round trip into a fresh EVEStream; get_state() does not hold it
    saved = s.get_gaze_history_state()
    s.clear_gaze_history(streams=[1])
    assert not s.gaze_history().any() and not s.get_gaze_history_state()['gaze_history']['rows'].any()
    fresh = eve_amd.EVEStream(model, B, use_graph=False)
    fresh.set_gaze_history_state(saved)
    assert torch.equal(fresh.gaze_history(), saved['gaze_history']['maps']) and not any('history' in k for k in s.get_state())
    assert torch.equal(fresh.get_gaze_history_state()['gaze_history']['rows'], saved['gaze_history']['rows'])
    with pytest.raises(ValueError, match='maps'):
        fresh.set_gaze_history_state({'gaze_history': dict(saved['gaze_history'], maps=torch.zeros(B, 3, 3))})
    with pytest.raises(ValueError, match='spec'):
        fresh.set_gaze_history_state({'gaze_history': {'maps': saved['gaze_history']['maps'], 'rows': saved['gaze_history']['rows']}})


def test_the_overlay_blends_a_history_map_by_heat_key(fake):
    from test_stream_ragged_host import CONFIGS, make_model as ragged_model
    import overlay_ref as oref
    model = ragged_model(*CONFIGS['gru-cgru'])
    Bc, Tc = 2, 2
    ch = stream_chunk(Bc, Tc)
    s = eve_amd.EVEStream(model, Bc, use_graph=False)
    with pytest.raises(ValueError, match='heat_key'):
        OverlaySpec(heat=True, heat_key='trail')
    overlay = OverlaySpec(markers=[], inset=None, out_format='rgb', heat_key='trail')
    assert overlay.key()[-1] == 'trail' and overlay != OverlaySpec(markers=[], inset=None, out_format='rgb') and not overlay.heat
    for history, match in ((None, 'heat_key'), (GazeHistorySpec(name='other', fps=30, per_frame=True), 'heat_key'),
                           (GazeHistorySpec(name='trail', fps=30), 'per_frame'),
                           (GazeHistorySpec(name='trail', fps=30, per_frame=True, size=(1025, 8)), '1024')):
        with pytest.raises(ValueError, match=match):
            s.step(ch, render=overlay, **({} if history is None else {'history': history}))
    assert fake.calls == [] and s._history == {}                         # refused before a launch and before an allocation
    out = s.step(ch, render=overlay, history=GazeHistorySpec(name='trail', fps=30, per_frame=True, sigma=6.0))
    assert fake.calls[-3:] == list(NEW_CALLS) + ['overlay_render']
    cap = ch['screen_frame_nv12']
    N = Bc * Tc
    frames = out['trail_frames']
    heat = dict(heat=frames.reshape((N,) + tuple(frames.shape[-2:])).numpy(), color=overlay.heat_color, amax=overlay.heat_amax)
    flat = cap.reshape((N,) + tuple(cap.shape[2:])).numpy()
    want = oref.render(flat, 'nv12', 'rgb', 'bt601', None, heat, None, None)
    assert np.array_equal(out['rendered'].reshape(want.shape).numpy(), want)
    assert not np.array_equal(want, oref.render(flat, 'nv12', 'rgb', 'bt601', None, None, None, None))
