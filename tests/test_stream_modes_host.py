"""CPU: every mode of EVEStream.step over the composed stand-ins -- the launches it issues in their order, the keywords it hands to
EVE._predict_sequence and the keys of its result, against literals recorded from the commit before the stages' scaffolding was folded
into shared helpers; the modes' graph keys; and the property the capture's warm-up relies on: putting _carried() back undoes a step."""
import pytest
import torch

import eve_amd
from eve_amd import kernels
from eve_amd.data import BlinkSpec, EyeGateSpec, GazeEventSpec, GazeHistorySpec, OverlaySpec
from test_eye_gate_host import GateFakes, eyelids
from test_gaze_history_host import HistoryFakes
from test_screen_calibration_host import ScreenFakes
from test_screen_formats_host import capture
from test_stream_host import chunk_of, clip, make_model


class ModeFakes(HistoryFakes, ScreenFakes, GateFakes):
    """Every stage's stand-ins at once: the mixins are cooperative, each adds its own entry points to MaskFakes."""


@pytest.fixture()
def fake():
    k = ModeFakes()
    kernels.set_default_kernels(k)
    yield k
    kernels.set_default_kernels(None)
    eve_amd.reset_standalone_config()


B, T = 2, 3
# per mode: the stand-ins' calls in order, sorted(the keywords EVE._predict_sequence saw), sorted(the result) -- recorded by running this
# table on the parent of the commit that introduced _carried(), not on the code under test
WANT = {
 'plain': {'calls': ['stream_state_rows', 'stream_state_rows', 'stream_state_rows', 'stream_state_rows'],
           'kwargs': ['reset', 'return_heatmaps'],
           'result': ['PoG_cm_final', 'PoG_cm_initial', 'PoG_px_final', 'PoG_px_initial', 'g_final', 'g_initial', 'left_g_initial', 'left_pupil_size',
                      'right_g_initial', 'right_pupil_size']},
 'lengths': {'calls': ['stream_state_rows', 'stream_state_rows_at', 'stream_state_rows', 'stream_state_rows_at'],
             'kwargs': ['lengths', 'reset', 'return_heatmaps'],
             'result': ['PoG_cm_final', 'PoG_cm_initial', 'PoG_px_final', 'PoG_px_initial', 'g_final', 'g_initial', 'left_g_initial',
                        'left_pupil_size', 'right_g_initial', 'right_pupil_size', 'valid']},
 'eye_mask': {'calls': ['stream_mask_plan', 'stream_permute_rows', 'stream_permute_rows', 'stream_state_rows', 'stream_state_rows_at',
                        'stream_permute_rows', 'stream_permute_rows', 'stream_state_rows', 'stream_permute_rows', 'stream_permute_rows',
                        'stream_state_rows_at'],
              'kwargs': ['eye_mask', 'lengths', 'masked', 'pose_gate', 'reset', 'return_heatmaps'],
              'result': ['PoG_cm_final', 'PoG_cm_initial', 'PoG_px_final', 'PoG_px_initial', 'eye_valid', 'g_final', 'g_initial', 'left_g_initial',
                         'left_pupil_size', 'right_g_initial', 'right_pupil_size', 'valid']},
 'events': {'calls': ['stream_state_rows', 'stream_state_rows', 'stream_state_rows', 'stream_state_rows', 'gaze_events'],
            'kwargs': ['events', 'reset', 'return_heatmaps'],
            'result': ['PoG_cm_final', 'PoG_cm_initial', 'PoG_px_filtered', 'PoG_px_final', 'PoG_px_initial', 'fixating', 'fixation_id',
                       'fixation_ms', 'fixation_px', 'g_final', 'g_initial', 'gaze_event', 'gaze_velocity', 'left_g_initial', 'left_pupil_size',
                       'right_g_initial', 'right_pupil_size']},
 'gate': {'calls': ['eye_gate', 'stream_mask_plan', 'stream_permute_rows', 'stream_permute_rows', 'stream_state_rows', 'stream_state_rows_at',
                    'stream_permute_rows', 'stream_permute_rows', 'stream_state_rows', 'stream_permute_rows', 'stream_permute_rows',
                    'stream_state_rows_at'],
          'kwargs': ['eye_mask', 'gate', 'lengths', 'masked', 'pose_gate', 'reset', 'return_heatmaps'],
          'result': ['PoG_cm_final', 'PoG_cm_initial', 'PoG_px_final', 'PoG_px_initial', 'blink', 'eye_gate_reason', 'eye_openness', 'eye_valid',
                     'g_final', 'g_initial', 'left_g_initial', 'left_pupil_size', 'right_g_initial', 'right_pupil_size', 'valid']},
 'history': {'calls': ['stream_state_rows', 'stream_state_rows', 'stream_state_rows', 'stream_state_rows', 'gaze_history_plan',
                       'gaze_history_update'],
             'kwargs': ['history', 'reset', 'return_heatmaps'],
             'result': ['PoG_cm_final', 'PoG_cm_initial', 'PoG_px_final', 'PoG_px_initial', 'g_final', 'g_initial', 'gaze_history', 'left_g_initial',
                        'left_pupil_size', 'right_g_initial', 'right_pupil_size']},
 'calibration_collect': {'calls': ['stream_state_rows', 'stream_state_rows', 'calib_append', 'stream_state_rows', 'stream_state_rows'],
                         'kwargs': ['calibration', 'reset', 'return_heatmaps'],
                         'result': ['PoG_cm_final', 'PoG_cm_initial', 'PoG_px_final', 'PoG_px_initial', 'g_final', 'g_initial', 'left_g_initial',
                                    'left_pupil_size', 'right_g_initial', 'right_pupil_size']},
 'calibration_apply': {'calls': ['stream_state_rows', 'stream_state_rows', 'stream_state_rows', 'stream_state_rows'],
                       'kwargs': ['calibration', 'reset', 'return_heatmaps'],
                       'result': ['PoG_cm_final', 'PoG_cm_initial', 'PoG_px_final', 'PoG_px_initial', 'calibrated', 'g_final', 'g_initial',
                                  'left_g_initial', 'left_g_initial_raw', 'left_pupil_size', 'right_g_initial', 'right_g_initial_raw',
                                  'right_pupil_size']},
 'screen_collect': {'calls': ['stream_state_rows', 'stream_state_rows', 'stream_state_rows', 'stream_state_rows', 'screen_calib_append'],
                    'kwargs': ['reset', 'return_heatmaps', 'screen_calibration'],
                    'result': ['PoG_cm_final', 'PoG_cm_initial', 'PoG_px_final', 'PoG_px_initial', 'g_final', 'g_initial', 'left_g_initial',
                               'left_pupil_size', 'right_g_initial', 'right_pupil_size']},
 'screen_apply': {'calls': ['stream_state_rows', 'stream_state_rows', 'stream_state_rows', 'stream_state_rows', 'screen_calib_apply'],
                  'kwargs': ['reset', 'return_heatmaps', 'screen_calibration'],
                  'result': ['PoG_cm_final', 'PoG_cm_initial', 'PoG_px_final', 'PoG_px_final_raw', 'PoG_px_initial', 'g_final', 'g_initial',
                             'left_g_initial', 'left_pupil_size', 'right_g_initial', 'right_pupil_size', 'screen_calibrated']},
 'render': {'calls': ['stream_state_rows', 'stream_state_rows', 'stream_state_rows', 'stream_state_rows', 'overlay_render'],
            'kwargs': ['render', 'reset', 'return_heatmaps'],
            'result': ['PoG_cm_final', 'PoG_cm_initial', 'PoG_px_final', 'PoG_px_initial', 'g_final', 'g_initial', 'left_g_initial',
                       'left_pupil_size', 'rendered', 'right_g_initial', 'right_pupil_size']},
 'everything': {'calls': ['eye_gate', 'stream_mask_plan', 'stream_permute_rows', 'stream_permute_rows', 'stream_state_rows', 'stream_state_rows_at',
                          'stream_permute_rows', 'stream_permute_rows', 'calib_append', 'stream_state_rows', 'stream_permute_rows',
                          'stream_permute_rows', 'stream_state_rows_at', 'screen_calib_append', 'screen_calib_apply', 'gaze_events',
                          'gaze_history_plan', 'gaze_history_update', 'overlay_render'],
                'kwargs': ['calibration', 'events', 'eye_mask', 'gate', 'history', 'lengths', 'masked', 'pose_gate', 'render', 'reset',
                           'return_heatmaps', 'screen_calibration'],
                'result': ['PoG_cm_final', 'PoG_cm_initial', 'PoG_px_filtered', 'PoG_px_final', 'PoG_px_final_raw', 'PoG_px_initial', 'blink',
                           'calibrated', 'eye_gate_reason', 'eye_openness', 'eye_valid', 'fixating', 'fixation_id', 'fixation_ms', 'fixation_px',
                           'g_final', 'g_initial', 'gaze_event', 'gaze_velocity', 'heatmap_final', 'left_g_initial', 'left_g_initial_raw',
                           'left_pupil_size', 'rendered', 'right_g_initial', 'right_g_initial_raw', 'right_pupil_size', 'screen_calibrated', 'trail',
                           'trail_frames', 'valid']},
 'idle_reset': {'calls': ['gaze_events', 'gaze_history_plan', 'gaze_history_update', 'stream_state_rows', 'stream_state_rows', 'stream_state_rows',
                          'stream_state_rows'],
                'kwargs': ['reset', 'return_heatmaps'],
                'result': ['PoG_cm_final', 'PoG_cm_initial', 'PoG_px_final', 'PoG_px_initial', 'g_final', 'g_initial', 'left_g_initial',
                           'left_pupil_size', 'right_g_initial', 'right_pupil_size']}}
KAPPA = torch.tensor([[[0.04, -0.05], [0.03, 0.02]], [[-0.02, 0.01], [0.05, -0.03]]])


@pytest.fixture()
def scene(fake):
    model, _ = make_model(dict(refine_net_rnn_type='CGRU'))
    return model, chunk_of(clip(B, T, size=32), 0, T)


def screen_map():
    coef = torch.zeros(B, 2, 6, dtype=torch.float64)
    coef[:, :, 0] = torch.tensor([30.0, -20.0])
    return coef, [2, 2]


def with_capture(chunk):
    return dict({k: v for k, v in chunk.items() if k != 'screen_frame'}, screen_frame_nv12=capture('nv12', B, T, seed=1))


def with_contours(chunk):
    return dict(chunk, eye_contours=eyelids([(0, 1, 0)])[:, :T].contiguous())


def everything(chunk):
    target = torch.full((B, T, 2), 500.0)
    chunk = with_contours(with_capture(dict(chunk, calibration_target=target, screen_calibration_target=target)))
    overlay = OverlaySpec(markers=[dict(key='PoG_px_final', r_fill=3, r_outline=5), dict(key='fixation_px', valid='fixating')],
                          inset=None, out_format='rgb', heat_key='trail')
    return chunk, dict(lengths=[2, 3], events=GazeEventSpec(fps=30, saccade_deg_s=1e9, min_fixation_s=0.02), gate=EyeGateSpec(blink=BlinkSpec(hold_frames=1)),
                       history=GazeHistorySpec(name='trail', fps=30, per_frame=True), render=overlay, return_heatmaps=True)


def apply_both(s):
    s.set_calibration(KAPPA)
    s.set_screen_calibration(*screen_map())


def run_stages_then_reset(s, chunk):
    s.step(with_contours(chunk), events=GazeEventSpec(fps=30), gate=EyeGateSpec(blink=BlinkSpec(hold_frames=1)), history=GazeHistorySpec(fps=30))
    s.reset([0])


# name -> (what is done to the fresh EVEStream first, the chunk of the observed step, its keywords)
MODES = {
    'plain': lambda c: (None, c, {}),
    'lengths': lambda c: (None, c, dict(lengths=[2, 1])),
    'eye_mask': lambda c: (None, c, dict(eye_mask=torch.tensor([[[1, 1], [0, 1], [1, 1]], [[1, 1]] * 3], dtype=torch.bool))),
    'events': lambda c: (None, c, dict(events=GazeEventSpec(fps=30))),
    'gate': lambda c: (None, with_contours(c), dict(gate=EyeGateSpec(blink=BlinkSpec(hold_frames=1)))),
    'history': lambda c: (None, c, dict(history=GazeHistorySpec(fps=30))),
    'calibration_collect': lambda c: (None, dict(c, calibration_target=torch.full((B, T, 2), 500.0)), {}),
    'calibration_apply': lambda c: (lambda s: s.set_calibration(KAPPA), c, {}),
    'screen_collect': lambda c: (None, dict(c, screen_calibration_target=torch.full((B, T, 2), 500.0)), {}),
    'screen_apply': lambda c: (lambda s: s.set_screen_calibration(*screen_map()), c, {}),
    'render': lambda c: (None, with_capture(c), dict(render=OverlaySpec(markers=[dict(key='PoG_px_final', r_fill=3, r_outline=5)],
                                                                        inset=None, out_format='rgb'))),
    'everything': lambda c: (apply_both,) + everything(c),
    'idle_reset': lambda c: (lambda s: run_stages_then_reset(s, c), c, {}),
}


def observe(fake, model, chunk, name):
    """One step of the mode on a fresh EVEStream -> (the stand-ins' calls, the keywords _predict_sequence saw, the result's keys, the
    graph key of the step as _run's arguments give it)."""
    prepare, chunk, kw = MODES[name](chunk)
    s = eve_amd.EVEStream(model, B, use_graph=False)
    if prepare is not None:
        prepare(s)
    seen, keys = [], []
    inner_predict, inner_run = model._predict_sequence, s._run
    model._predict_sequence = lambda *a, **k: seen.append(sorted(k)) or inner_predict(*a, **k)

    def run(chunk, return_heatmaps, ragged=False, eye_mask=None, masked=False, render=None, events=None, gate=None, history=None):
        keys.append(s._graph_key(chunk, bool(return_heatmaps), ragged, masked, render, events, gate=gate, history=history))
        return inner_run(chunk, return_heatmaps, ragged, eye_mask, masked, render, events, gate=gate, history=history)

    s._run = run
    del fake.calls[:]
    try:
        out = s.step(chunk, **kw)
    finally:
        model._predict_sequence = inner_predict
    assert len(seen) == 1 and len(keys) == 1
    return list(fake.calls), seen[0], sorted(out), keys[0]


@pytest.mark.parametrize('name', list(MODES))
def test_a_mode_issues_the_recorded_calls_keywords_and_result(fake, scene, name):
    model, chunk = scene
    calls, kwargs, result, _ = observe(fake, model, chunk, name)
    want = WANT[name]
    assert calls == want['calls']
    assert kwargs == want['kwargs']
    assert result == want['result']


def test_the_table_is_the_recorded_one():
    assert sorted(MODES) == sorted(WANT)


def test_the_graph_keys_tell_the_modes_apart(fake, scene):
    model, chunk = scene
    keys = {name: observe(fake, model, chunk, name)[3] for name in MODES}
    again = {name: observe(fake, model, chunk, name)[3] for name in MODES}
    # the step after an idle reset IS a plain step on the plain chunk: it replays the plain graph, so the two keys are one
    assert keys.pop('idle_reset') == keys['plain']
    names = list(keys)
    for i, a in enumerate(names):
        assert keys[a] == again[a], a                    # a mode repeated, with specs made anew: the same graph
        assert keys[a][1] == ('lengths' in MODES[a](chunk)[2]), a
        for b_ in names[i + 1:]:
            assert keys[a] != keys[b_], (a, b_)


def tensors_of(x):
    if torch.is_tensor(x):
        return [x]
    if isinstance(x, dict):
        return [t for k in sorted(x) for t in tensors_of(x[k])]
    if isinstance(x, (list, tuple)):
        return [t for v in x for t in tensors_of(v)]
    return []


GETTERS = ('get_state', 'get_head_pose', 'get_calibration', 'calibration_samples', 'calibration_counts', 'get_screen_calibration',
           'screen_calibration_samples', 'screen_calibration_counts', 'get_event_state', 'fixation_counts', 'get_gate_state', 'blink_counts',
           'get_gaze_history_state')


def test_putting_the_carried_tensors_back_undoes_a_step(fake, scene):
    """What _capture's warm-up steps rely on: _carried() is everything a step writes.  A buffer missing from it keeps what the step
    wrote, and its getter then differs."""
    model, chunk = scene
    prepare, chunk, kw = MODES['everything'](chunk)
    s = eve_amd.EVEStream(model, B, use_graph=False)
    prepare(s)
    s.step(chunk, **kw)                                  # every stage's buffers exist and hold something
    before = {g: tensors_of(getattr(s, g)()) for g in GETTERS}
    assert all(before.values())
    carried = s._carried()
    snap = [t.clone() for t in carried]
    s.reset([1])
    s.step(chunk, **kw)
    moved = {g for g in GETTERS if any(not torch.equal(a, b_) for a, b_ in zip(before[g], tensors_of(getattr(s, g)())))}
    # (the step did write: the states, both stores, the events' row, the gate's ticks, the history's map; kappa and the map's
    # coefficients are not a step's to write, and the patch chunk solves no head pose)
    assert moved == set(GETTERS) - {'get_head_pose', 'get_calibration', 'get_screen_calibration'}
    for t, s_ in zip(carried, snap):
        t.copy_(s_)
    for g in GETTERS:
        after = tensors_of(getattr(s, g)())
        assert len(after) == len(before[g]) and all(torch.equal(a, b_) for a, b_ in zip(before[g], after)), g
