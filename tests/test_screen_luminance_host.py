"""Screen luminance on the CPU: the numpy contract (tests/screen_luminance_ref.py) against an independent brute force, the response
table, the spec, and EVEStream.step(chunk, luminance=...) on the stand-in kernels."""
import os
import re

import numpy as np
import pytest
import torch

import pupil_ref
import screen_luminance_ref as ref
import surface_ref as sref
import eve_amd
from eve_amd import _lib, data, kernels
from eve_amd.data import PupilSpec, ScreenLuminanceSpec, SurfaceLayout
from test_pupil_host import PupilFakes
from test_stream_host import chunk_of, clip, make_model

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = ref.srgb_table()


# ---------------------------------------------------------------------------------------------------------------- the contract
@pytest.mark.parametrize('fmt', sref.FORMATS)
def test_the_reference_equals_the_brute_force(fmt):
    """16 x 12 in every format, three frames, discs of 1, 3 and 5 pixels around a centre inside, one on a half-pixel tie and one off
    the screen, lengths that drop the last frame's stream."""
    layout = SurfaceLayout(fmt, 16, 12)
    buf, _ = sref.random_surface(layout, 3, seed=7)
    centres = np.array([[8.0, 6.0], [2.25, 11.75], [-40.0, 3.0]], dtype=np.float32)
    kw = dict(radii=(1, 3, 5), centres=centres, sx=1.0, sy=1.0, centre_valid=np.array([1, 1, 1], np.uint8), lengths=np.array([2, 1]), matrix='bt709')
    a = ref.luminance(buf, layout, TABLE, ref.REC709, 1, 3, **dict(kw, lengths=None))
    b = ref.brute(buf, layout, TABLE, ref.REC709, 1, 3, **dict(kw, lengths=None))
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    assert a[1][0].tolist() == [192, 4, 32, 80] and a[1][2].tolist() == [192, 0, 0, 0] and np.isnan(a[2][2, 1:]).all()
    layout2 = SurfaceLayout(fmt, 16, 12, pitch=16 * sref.BYTES_PER_PIXEL[fmt] + 8, x0=2, y0=2, coded_height=16)
    buf2, _ = sref.random_surface(layout2, 3, seed=8)
    a = ref.luminance(buf2, layout2, TABLE, (65536, 0, 0), 3, 1, **dict(kw, lengths=np.array([1, 0, 1])))
    b = ref.brute(buf2, layout2, TABLE, (65536, 0, 0), 3, 1, **dict(kw, lengths=np.array([1, 0, 1])))
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert not a[1][1].any() and np.isnan(a[2][1]).all()                  # an undelivered frame: every column 0, every mean NaN


def test_a_checkerboard_has_half_the_luminance_and_the_shortcut_says_a_fifth():
    """A one-pixel black / white checker: the mean relative luminance is 0.5; linearising the mean byte (sRGB 128) gives 0.216."""
    H, W = 12, 16
    rgb = np.where(((np.arange(H)[:, None] + np.arange(W)[None, :]) % 2 == 0)[..., None], 255, 0).astype(np.uint8).repeat(3, axis=2)
    layout = SurfaceLayout('rgb', W, H)
    sums, counts, mean = ref.luminance(rgb.reshape(1, -1), layout, TABLE, ref.REC709, 1, 1)
    assert counts[0, 0] == W * H and sums[0, 0] == 65535 * W * H // 2 and mean[0, 0] == np.float32(0.5)
    short = ref.mean_of_resized(rgb, TABLE, ref.REC709, 2)
    assert abs(short - 14146 / 65535.0) < 1e-9 and abs(short - 0.216) < 5e-4 and 2.3 < 0.5 / short < 2.35


@pytest.mark.parametrize('r,q,count', [(1, (16, 12), 4), (3, (16, 12), 32), (3, (0, 0), 8), (3, (-7, 5), 0), (1, (17, 13), 5)])
def test_disc_counts_at_16_by_12(r, q, count):
    assert ref.disc_count(16, 12, r, *q) == count
    rgb = np.full((1, 12 * 16 * 3), 255, dtype=np.uint8)
    centres = np.array([[q[0] / 2.0, q[1] / 2.0]], dtype=np.float32)
    sums, counts, mean = ref.luminance(rgb, SurfaceLayout('rgb', 16, 12), TABLE, ref.REC709, 1, 1, radii=(r,), centres=centres)
    assert counts[0, 1] == count and sums[0, 1] == 65535 * count
    assert np.isnan(mean[0, 1]) if count == 0 else mean[0, 1] == 1.0


def test_centres_quantise_in_float32_with_ties_to_even():
    qx, qy = ref.quantise(np.array([[0.25, 0.75], [1.25, np.nan], [1e9, -np.inf]], np.float32), 1.0, 1.0)
    assert qx[:2].tolist() == [0.0, 2.0] and qy[0] == 2.0 and np.isnan(qy[1]) and qx[2] == np.float32(2e9) and qy[2] == -np.inf
    qx, _ = ref.quantise(np.array([[100.1, 0.0]], np.float32), 0.3, 1.0)
    assert qx[0] == np.rint(np.float32(np.float32(100.1) * np.float32(0.3)) * np.float32(2))


# ---------------------------------------------------------------------------------------------------------------- the table
def test_the_srgb_table_is_pinned():
    t = data.display_response()
    assert t.dtype == torch.uint16 and tuple(t.shape) == (3, 256)
    t = t.numpy()
    assert t.tobytes() == TABLE.tobytes()
    assert t[0, [0, 1, 128, 188, 255]].tolist() == [0, 20, 14146, 32957, 65535] and (np.diff(t.astype(np.int64), axis=1) >= 0).all()
    v = np.arange(256) / 255.0
    x = 65535.0 * np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4) + 0.5
    frac = np.abs(x - np.rint(x))                                         # the distance of floor's argument to an integer
    assert int(np.argmin(frac[1:255])) + 1 == 111 and 0.0016 < frac[111] < 0.0018


def test_power_law_and_measured_responses():
    g = data.display_response('gamma', gamma=2.0).numpy()
    assert g[1, 255] == 65535 and g[2, 128] == int(np.floor(65535.0 * (128 / 255.0) ** 2 + 0.5)) and (g[0] == g[2]).all()
    ramp = np.arange(256) / 255.0
    m = data.display_response('measured', measured=ramp).numpy()
    assert m[0].tolist() == [int(np.floor(65535.0 * v + 0.5)) for v in ramp]
    m3 = data.display_response('measured', measured=np.stack([ramp, ramp ** 2, np.zeros(256)])).numpy()
    assert (m3[0] == m[0]).all() and (m3[1] == g[1]).all() and not m3[2].any()
    for kw in (dict(kind='rec709'), dict(kind='srgb', gamma=2.2), dict(kind='gamma'), dict(kind='gamma', gamma=0.0), dict(kind='gamma', gamma=float('nan')),
               dict(kind='measured'), dict(kind='measured', measured=np.zeros(255)), dict(kind='measured', measured=ramp * 2),
               dict(kind='measured', measured=np.full(256, np.nan)), dict(kind='measured', measured=ramp, gamma=2.0)):
        with pytest.raises(ValueError, match='display_response'):
            data.display_response(**kw)


# ---------------------------------------------------------------------------------------------------------------- the spec
def test_the_spec_compares_by_value_and_refuses_nonsense():
    a = ScreenLuminanceSpec(radii_px=(60, 200), to_pupil=(0.0, 1.0))
    assert a == ScreenLuminanceSpec('screen_luminance', [60.0, 200.0], None, None, 'srgb', 'rec709', [0, 1]) and hash(a) == hash(ScreenLuminanceSpec(
        radii_px=(60, 200), to_pupil=(0.0, 1.0)))
    assert eve_amd.ScreenLuminanceSpec is ScreenLuminanceSpec and 'ScreenLuminanceSpec' in eve_amd.__all__
    assert a.weights == ref.REC709 and sum(a.weights) == 65536 and a.result_keys() == ('screen_luminance', 'screen_luminance_gaze', 'screen_luminance_covariate')
    assert ScreenLuminanceSpec(to_pupil=None).result_keys() == ('screen_luminance',)
    others = [ScreenLuminanceSpec(radii_px=(60, 201), to_pupil=(0.0, 1.0)), ScreenLuminanceSpec('lum', (60, 200), to_pupil=(0.0, 1.0)),
              ScreenLuminanceSpec(radii_px=(60, 200)), ScreenLuminanceSpec(radii_px=(60, 200), to_pupil=(0.0, 1.0), response=('gamma', 2.2)),
              ScreenLuminanceSpec(radii_px=(60, 200), to_pupil=(0.0, 1.0), weights=(19595, 38470, 7471)),
              ScreenLuminanceSpec(radii_px=(60, 200), to_pupil=(0.0, 1.0), source='PoG_px_initial'),
              ScreenLuminanceSpec(radii_px=(60, 200), to_pupil=(0.0, 1.0), valid_key='fixating')]
    assert len({a} | set(others)) == 8
    same_table = ScreenLuminanceSpec(response=data.display_response('gamma', gamma=2.2))
    assert same_table == ScreenLuminanceSpec(response=data.display_response('gamma', gamma=2.2).numpy()) and same_table != ScreenLuminanceSpec()
    assert same_table.response_table().numpy().tobytes() == data.display_response('gamma', gamma=2.2).numpy().tobytes()
    assert a.capture_radii(0.5) == (30, 100) and ScreenLuminanceSpec(radii_px=(0.4,)).capture_radii(1.0) == (1,)
    with pytest.raises(ValueError, match='strictly increasing'):
        ScreenLuminanceSpec(radii_px=(1, 2)).capture_radii(0.25)
    with pytest.raises(ValueError, match='16384'):
        a.capture_radii(100.0)
    for kw in (dict(name=''), dict(name=3), dict(radii_px=(1, 2, 3, 4, 5)), dict(radii_px=(2, 2)), dict(radii_px=(3, 2)), dict(radii_px=(0,)),
               dict(radii_px=(float('nan'),)), dict(radii_px=5), dict(source='heatmap_final'), dict(valid_key=''), dict(valid_key=3),
               dict(response='rec709'), dict(response=np.zeros((3, 256), np.int32)), dict(response=np.zeros((256,), np.uint16)),
               dict(response=('gamma', -1.0)), dict(weights='rec2020'), dict(weights=(1, 2, 3)), dict(weights=(65537, -1, 0)),
               dict(weights=(0.5, 0.25, 0.25)), dict(weights=(65536, 0)), dict(to_pupil=(1.0, 1.0)), dict(to_pupil=()), dict(to_pupil=(0.0,)),
               dict(to_pupil=(float('inf'),)), dict(to_pupil=1.0), dict(radii_px=(5,), to_pupil=(1.0, 1.0, 1.0))):
        with pytest.raises(ValueError):
            ScreenLuminanceSpec(**kw)


def test_the_symbol_is_declared_typed_and_exported():
    assert 'eve_screen_luminance' in _lib.SIGNATURES and 'eve_screen_luminance' in _lib.EXPORTS and _lib.ABI_VERSION == 10
    header = open(os.path.join(REPO, 'include', 'eve_hip.h')).read()
    decl = re.search(r'\nint eve_screen_luminance\((.*?)\);', header, re.S)
    assert decl is not None and '(Additive: ABI v10.)' in header[header.index('/* Screen luminance:'):decl.start()]
    params = re.sub(r'/\*.*?\*/', '', decl.group(1), flags=re.S).split(',')
    assert len(params) == len(_lib.SIGNATURES['eve_screen_luminance']) == 20
    import inspect
    sig = inspect.signature(kernels.HipKernels.screen_luminance)
    assert list(sig.parameters)[1:] == ['frames', 'layout', 'response', 'weights', 'B', 'T', 'radii', 'centres', 'sx', 'sy', 'centre_valid',
                                        'lengths', 'matrix']
    assert sig.parameters['radii'].default == () and sig.parameters['matrix'].default == 'bt601' and sig.parameters['sx'].default == 1.0
    src = open(os.path.join(REPO, 'eve_amd', 'csrc', 'screen_luminance.hip')).read()
    assert 'constexpr int LUM_BAND_ROWS = %d;' % kernels.LUM_BAND_ROWS in src
    assert 'luminance computed from the screen' not in header


# ---------------------------------------------------------------------------------------------------------------- EVEStream
class LuminanceFakes(PupilFakes):
    """The pupil stage's stand-ins plus screen_luminance, evaluated by tests/screen_luminance_ref.py; pupil_track records the
    luminance it was handed."""
    screen_luminance = ref.screen_luminance

    def pupil_track(self, size, spec, *a, **kw):
        self.luminances = getattr(self, 'luminances', []) + [None if kw.get('luminance') is None else kw['luminance'].clone()]
        return PupilFakes.pupil_track(self, size, spec, *a, **kw)


@pytest.fixture()
def fake():
    k = LuminanceFakes()
    kernels.set_default_kernels(k)
    yield k
    kernels.set_default_kernels(None)
    eve_amd.reset_standalone_config()


B, T, IW, IH = 2, 3, 136, 76           # the smallest sizes RefineNet takes are its own 128 x 72: no upscaling


@pytest.fixture()
def scene(fake):
    model, _ = make_model(dict(refine_net_rnn_type='CGRU'))
    with torch.no_grad():
        model.eye_net.fc_to_pupil[2].bias.add_(3.0)
    batch = clip(B, T, size=32)
    c0 = chunk_of(batch, 0, T)
    del c0['screen_frame']
    g = torch.Generator().manual_seed(5)
    c0['screen_frame_nv12'] = torch.randint(0, 256, (B, T, IH * 3 // 2, IW), generator=g, dtype=torch.uint8)
    del fake.calls[:]
    return model, c0


def run(stream, chunk, **kw):
    return {k: v.clone() for k, v in stream.step(chunk, **kw).items()}


def want_for(model, chunk, out, spec, lengths=None, valid=None):
    cfg = model.config
    layout = SurfaceLayout('nv12', IW, IH)
    sx, sy = np.float32(IW / float(cfg.actual_screen_size[0])), np.float32(IH / float(cfg.actual_screen_size[1]))
    radii = spec.capture_radii(IW / float(cfg.actual_screen_size[0]))
    centres = out['PoG_px_final'].numpy().reshape(-1, 2) if radii else None
    return ref.luminance(chunk['screen_frame_nv12'].numpy().reshape(B * T, -1), layout, spec.response_table().numpy(), spec.weights, B, T, radii,
                         centres, sx, sy, valid, lengths, model.refine_net.yuv_matrix)


def test_a_step_with_luminance_adds_its_keys_and_one_launch(fake, scene):
    model, c0 = scene
    W = float(model.config.actual_screen_size[0])
    plain = run(eve_amd.EVEStream(model, B, use_graph=False), c0)
    calls_plain = list(fake.calls)
    assert 'screen_luminance' not in calls_plain
    del fake.calls[:]
    spec = ScreenLuminanceSpec(radii_px=(4 * W / IW, 12 * W / IW), to_pupil=(0.25, 0.0, 0.75))
    s = eve_amd.EVEStream(model, B, use_graph=False)
    out = run(s, c0, luminance=spec)
    assert fake.calls == calls_plain + ['screen_luminance']
    assert sorted(out) == sorted(list(plain) + ['screen_luminance', 'screen_luminance_gaze', 'screen_luminance_covariate'])
    for k in plain:
        assert torch.equal(out[k], plain[k]), k
    _, counts, mean = want_for(model, c0, out, spec)
    assert out['screen_luminance'].dtype == torch.float32 and tuple(out['screen_luminance_gaze'].shape) == (B, T, 2)
    assert out['screen_luminance'].numpy().tobytes() == mean[:, 0].tobytes() and (counts[:, 0] == IW * IH).all()
    assert out['screen_luminance_gaze'].numpy().tobytes() == np.ascontiguousarray(mean[:, 1:]).tobytes()
    assert out['screen_luminance_covariate'].numpy().tobytes() == ref.covariate(mean, spec.to_pupil).tobytes()
    # lengths drop frames from every column; a masked step's valid and a valid_key only touch the discs
    out = run(eve_amd.EVEStream(model, B, use_graph=False), c0, luminance=spec, lengths=[2, 0])
    _, _, mean = want_for(model, c0, out, spec, lengths=np.array([2, 0]))
    assert out['screen_luminance'].numpy().tobytes() == mean[:, 0].tobytes() and torch.isnan(out['screen_luminance'][1]).all()
    mask = torch.ones(B, T, 2, dtype=torch.bool)
    mask[0, 1] = False
    key = torch.tensor([[1, 1, 0], [1, 1, 1]], dtype=torch.bool)
    keyed = ScreenLuminanceSpec(radii_px=spec.radii_px, valid_key='looking', to_pupil=None)
    out = run(eve_amd.EVEStream(model, B, use_graph=False), dict(c0, looking=key), luminance=keyed, eye_mask=mask)
    valid = (out['valid'] & key).numpy().astype(np.uint8).reshape(-1)
    assert valid.tolist() == [1, 0, 0, 1, 1, 1] and 'screen_luminance_covariate' not in out
    _, _, mean = want_for(model, c0, out, keyed, valid=valid)
    assert out['screen_luminance_gaze'].numpy().tobytes() == np.ascontiguousarray(mean[:, 1:]).tobytes()
    assert not torch.isnan(out['screen_luminance']).any() and torch.isnan(out['screen_luminance_gaze'][0, 1:]).all()


def test_the_covariate_reaches_the_pupil_stage(fake, scene):
    model, c0 = scene
    spec = ScreenLuminanceSpec(to_pupil=(2.0,))
    pupil = PupilSpec(fps=32, min_mm=0.1, max_mm=50.0, max_speed_mm_s=1e4)
    out = run(eve_amd.EVEStream(model, B, use_graph=False), c0, luminance=spec, pupil=pupil)
    assert fake.calls[-2:] == ['screen_luminance', 'pupil_track'] and len(fake.luminances) == 1
    assert torch.equal(fake.luminances[0], out['screen_luminance_covariate']) and torch.equal(out['screen_luminance_covariate'], out['screen_luminance'] * 2.0)
    fed = run(eve_amd.EVEStream(model, B, use_graph=False), dict(c0, pupil_luminance=out['screen_luminance_covariate']), pupil=pupil)
    for k in pupil_ref.KEYS:
        assert out['pupil_' + k].numpy().tobytes() == fed['pupil_' + k].numpy().tobytes(), k
    # without to_pupil the pupil stage sees what it always saw
    del fake.luminances[:]
    run(eve_amd.EVEStream(model, B, use_graph=False), c0, luminance=ScreenLuminanceSpec(to_pupil=None), pupil=pupil)
    assert fake.luminances == [None]


def test_refusals_come_before_any_launch(fake, scene):
    model, c0 = scene
    s = eve_amd.EVEStream(model, B, use_graph=False)
    spec = ScreenLuminanceSpec()
    with pytest.raises(ValueError, match='ScreenLuminanceSpec'):
        s.step(c0, luminance=dict(radii_px=()))
    with pytest.raises(ValueError, match='ScreenLuminanceSpec'):
        s.step(c0, luminance=PupilSpec(fps=30))
    bare = {k: v for k, v in c0.items() if k != 'screen_frame_nv12'}
    with pytest.raises(ValueError, match='holds none'):
        s.step(bare, luminance=spec)
    cfg = model.config
    for frame in (torch.zeros(B, T, 3, int(cfg.screen_size[1]), int(cfg.screen_size[0])),
                  torch.zeros(B, T, int(cfg.screen_size[1]), int(cfg.screen_size[0]), 3, dtype=torch.uint8)):
        with pytest.raises(ValueError, match='not a capture'):
            s.step(dict(bare, screen_frame=frame), luminance=spec)
    with pytest.raises(ValueError, match='luminance'):
        s.step(dict(bare, screen_frame_nv12=c0['screen_frame_nv12'][:, :, :-1].contiguous()), luminance=spec)
    with pytest.raises(ValueError, match='screen_layout'):
        s.step(dict(bare, screen_surface=c0['screen_frame_nv12']), luminance=spec)
    with pytest.raises(ValueError, match='pupil_luminance'):
        s.step(dict(c0, pupil_luminance=torch.zeros(B, T)), luminance=spec, pupil=PupilSpec(fps=30))
    for source in ('PoG_px_filtered', 'fixation_px'):
        with pytest.raises(ValueError, match='events='):
            s.step(c0, luminance=ScreenLuminanceSpec(radii_px=(100,), source=source))
    with pytest.raises(ValueError, match='valid_key'):
        s.step(c0, luminance=ScreenLuminanceSpec(radii_px=(100,), valid_key='nowhere'))
    with pytest.raises(ValueError, match='name'):
        s.step(dict(c0, screen_luminance=torch.zeros(B, T)), luminance=spec)
    with pytest.raises(ValueError, match='name'):
        s.step(c0, luminance=ScreenLuminanceSpec('pupil_mm', to_pupil=None), pupil=PupilSpec(fps=30))
    with pytest.raises(ValueError, match='name'):
        s.step(c0, luminance=ScreenLuminanceSpec('g_final', to_pupil=None))
    with pytest.raises(ValueError, match='strictly increasing'):
        s.step(c0, luminance=ScreenLuminanceSpec(radii_px=(1, 2)))           # both are one capture pixel at 136 / actual width
    with pytest.raises(ValueError, match='to_pupil'):
        ScreenLuminanceSpec(to_pupil=(1.0, 1.0))                              # more weights than columns
    assert fake.calls == [] and s._pupil == {}


def test_the_graph_key_holds_the_spec(fake, scene):
    model, c0 = scene
    s = eve_amd.EVEStream(model, B, use_graph=False)
    plan = lambda spec_: s._check_luminance(c0, spec_, None, None, None, None, None, False, B, T)
    spec = ScreenLuminanceSpec(radii_px=(100, 300))
    bare = s._graph_key(c0, False)
    a = s._graph_key(c0, False, luminance=plan(spec))
    assert a != bare and a == s._graph_key(dict(c0), False, luminance=plan(ScreenLuminanceSpec(radii_px=(100.0, 300.0))))
    assert a != s._graph_key(c0, False, luminance=plan(ScreenLuminanceSpec(radii_px=(100, 301))))
    assert a != s._graph_key(c0, False, luminance=plan(ScreenLuminanceSpec(radii_px=(100, 300), source='PoG_px_initial')))
    assert plan(spec)['table'] is plan(ScreenLuminanceSpec(radii_px=(100, 300)))['table']       # cached per spec, made before any capture
    assert plan(spec)['layout'] == SurfaceLayout('nv12', IW, IH) and plan(spec)['matrix'] == model.refine_net.yuv_matrix and plan(spec)['source'] == 'PoG_px_final'
    captured = []
    s._capture = lambda chunk, *a_, **k_: captured.append((a_, k_)) or {'n': len(captured)}
    first = s._graph_for(c0, False, luminance=plan(spec))
    assert s._graph_for(c0, False, luminance=plan(ScreenLuminanceSpec(radii_px=(100, 300)))) is first and len(captured) == 1 and 'luminance' in captured[0][1]
    assert s._graph_for(c0, False) is not first and len(captured) == 2 and len(captured[1][0]) == 4 and captured[1][1] == {}
    assert fake.calls == [] and len(s._carried()) == len(eve_amd.EVEStream(model, B, use_graph=False)._carried())     # no carried state


def test_the_stand_alone_entry_equals_the_reference(fake):
    g = np.random.default_rng(3)
    frames = torch.from_numpy(g.integers(0, 256, size=(2, 2, 12, 16, 4), dtype=np.uint8))
    spec = ScreenLuminanceSpec('lum', radii_px=(8, 24), to_pupil=(0.0, 0.0, 1.0))
    pog = torch.tensor([[[64.0, 48.0], [0.0, 0.0]], [[float('nan'), 3.0], [127.0, 95.0]]])
    out = data.screen_luminance(frames, 'rgb', spec, (128, 96), pog_px=pog, valid=torch.tensor([[1, 1], [1, 0]], dtype=torch.bool))
    layout = SurfaceLayout('rgba', 16, 12)
    sums, counts, mean = ref.luminance(frames.numpy().reshape(4, -1), layout, TABLE, ref.REC709, 2, 2, (1, 3), pog.numpy().reshape(-1, 2),
                                       np.float32(16 / 128.0), np.float32(12 / 96.0), np.array([1, 1, 1, 0], np.uint8))
    assert sorted(out) == ['counts', 'lum', 'lum_covariate', 'lum_gaze', 'sums']
    assert out['sums'].numpy().tobytes() == sums.tobytes() and out['counts'].numpy().tobytes() == counts.tobytes()
    assert out['lum_covariate'].numpy().tobytes() == mean[:, 2].tobytes() and counts[:, 1].tolist() == [4, 1, 0, 0]
    with pytest.raises(ValueError, match='pog_px'):
        data.screen_luminance(frames, 'rgb', spec, (128, 96))
    with pytest.raises(ValueError, match='ScreenLuminanceSpec'):
        data.screen_luminance(frames, 'rgb', None, (128, 96))
    with pytest.raises(ValueError, match='screen_size'):
        data.screen_luminance(frames, 'rgb', spec, (0, 96), pog_px=pog)
    with pytest.raises(TypeError):
        data.screen_luminance(frames.float(), 'rgb', spec, (128, 96), pog_px=pog)
