"""eve_screen_luminance on the device against tests/screen_luminance_ref.py, bit for bit: every format and load form, the discs'
edge cases, lengths, band boundaries, the accumulator width, the refusals, the stand-alone entry and the EVEStream stage."""
import ctypes

import numpy as np
import pytest
import torch

import eve_amd
import pupil_ref
import screen_luminance_ref as ref
import surface_ref as sref
from eve_amd import data, kernels
from eve_amd.data import PupilSpec, ScreenLuminanceSpec, SurfaceLayout
from eve_amd.kernels import default_kernels
from test_gpu_calibration import cuda
from test_gpu_stream import gpu_clip, make_model

pytestmark = pytest.mark.gpu

TABLE = ref.srgb_table()
YUV420 = ('nv12', 'nv21', 'i420', 'yv12')
VEC, BYTE, GENERIC = ('screen_luminance_kernel<yuv420,true>', 'screen_luminance_kernel<yuv420,false>', 'screen_luminance_kernel<generic,false>')


def table_on_device(table=TABLE):
    return torch.from_numpy(table.copy()).cuda()


def centres_for(N, W, H, seed):
    """Centres on and around a W x H frame, quarter pixels so that half-pixel ties occur."""
    g = np.random.default_rng(seed)
    return (g.integers(-8, 4 * max(W, H) + 8, size=(N, 2)) / 4.0).astype(np.float32)


def check(layout, B, T, radii=(), centres=None, sx=1.0, sy=1.0, centre_valid=None, lengths=None, matrix='bt601', seed=0, buf=None, weights=ref.REC709,
          form=None):
    """One launch against the reference -> the reference's (sums, counts, mean)."""
    k = default_kernels()
    if buf is None:
        buf, _ = sref.random_surface(layout, B * T, seed=seed)
    c = lambda a, dtype: None if a is None else cuda(np.asarray(a, dtype=dtype))
    got = k.screen_luminance(cuda(buf), layout, table_on_device(), weights, B, T, radii=radii, centres=c(centres, np.float32), sx=sx, sy=sy,
                             centre_valid=c(centre_valid, np.uint8), lengths=c(lengths, np.int32), matrix=matrix)
    name = k.lib.eve_last_kernel().decode()
    want = ref.luminance(buf, layout, TABLE, weights, B, T, radii, centres, np.float32(sx), np.float32(sy), centre_valid, lengths, matrix)
    for g, w, what in zip(got, want, ('sums', 'counts', 'mean')):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, layout, radii, g, w)
    if form is not None:
        assert name == form, (name, layout)
    return want


@pytest.mark.parametrize('fmt', ['rgb', 'bgra', 'nv12', 'nv21', 'i420', 'yv12', 'yuyv', 'uyvy', 'p010'])
def test_every_format_and_size_with_no_one_and_four_discs(fmt):
    """16 x 12 and 40 x 22 (tight 4:2:0 rows of those widths start on 8 bytes: the vector form), 44 x 22 (they do not: the byte form) and
    an odd 21 x 13 for the formats that take one; three frames, random bytes, R in {0, 1, 4}."""
    sizes = [(16, 12), (40, 22), (44, 22)] + ([(21, 13)] if fmt in ('rgb', 'bgra') else [])
    for W, H in sizes:
        layout = SurfaceLayout(fmt, W, H)
        form = GENERIC if fmt not in YUV420 else VEC if W % 8 == 0 else BYTE
        for R, radii in ((0, ()), (1, (3,)), (4, (1, 2, 5, 9))):
            want = check(layout, 1, 3, radii=radii, centres=centres_for(3, W, H, seed=W + R) if R else None, matrix=('bt601', 'bt709', 'jfif')[R % 3],
                         seed=10 * W + R, form=form)
            assert (want[1][:, 0] == W * H).all()


def test_the_wide_loads_of_nv12_at_64_by_34():
    W, H = 64, 34
    want = check(SurfaceLayout('nv12', W, H), 2, 2, radii=(4, 11), centres=centres_for(4, W, H, 3), seed=5, form=VEC)
    assert want[1][:, 1:].any()
    check(SurfaceLayout('yv12', W, H), 2, 2, radii=(4, 11), centres=centres_for(4, W, H, 3), seed=6, form=VEC)
    # planes at offsets that do not share the luma's alignment: the byte form, the same bits
    odd = SurfaceLayout('nv12', W, H, plane_offsets=(W * H + 2,))
    check(odd, 1, 2, radii=(4,), centres=centres_for(2, W, H, 4), seed=7, form=BYTE)


def test_pitched_and_cropped_surfaces():
    """NV12 with pitch 72, 40 coded rows and a crop at (2, 2): pixel (0, 0) lies 2 bytes behind an 8-byte boundary (skew != 0), the
    first and the last group of a row are partial.  Pitched BGRA with a crop.  Every byte outside the visible region is random."""
    nv12 = SurfaceLayout('nv12', 60, 34, pitch=72, coded_height=40, x0=2, y0=2)
    check(nv12, 1, 3, radii=(2, 7), centres=centres_for(3, 60, 34, 1), seed=11, form=VEC, matrix='bt709')
    i420 = SurfaceLayout('i420', 52, 30, pitch=80, coded_height=36, x0=4, y0=2)
    check(i420, 1, 2, radii=(6,), centres=centres_for(2, 52, 30, 2), seed=12, form=VEC)
    bgra = SurfaceLayout('bgra', 20, 14, pitch=112, coded_height=16, x0=3, y0=1)
    check(bgra, 2, 1, radii=(2, 7), centres=centres_for(2, 20, 14, 3), seed=13, form=GENERIC)
    p010 = SurfaceLayout('p010', 16, 12, pitch=48, coded_height=14, x0=2, y0=2)
    check(p010, 1, 2, seed=14, form=GENERIC)


def test_every_kind_of_centre_in_one_launch():
    """Inside; on a corner; on a half-pixel tie (2.25 -> q 4, 11.75 -> q 24: ties to even); off the screen (count 0, mean NaN); NaN;
    1e9 (|q| > 2^20); centre_valid 0; and scales that are no dyadic numbers."""
    layout = SurfaceLayout('rgb', 16, 12)
    centres = np.array([[8.0, 6.0], [0.0, 0.0], [2.25, 11.75], [-40.0, 3.0], [np.nan, 3.0], [1e9, 3.0], [8.0, 6.0], [8.5, np.inf]], np.float32)
    valid = np.array([1, 1, 1, 1, 1, 1, 0, 1], np.uint8)
    sums, counts, mean = check(layout, 8, 1, radii=(1, 3), centres=centres, centre_valid=valid, seed=21)
    assert counts[:, 1:].tolist() == [[4, 32], [1, 8], [ref.disc_count(16, 12, 1, 4, 24), ref.disc_count(16, 12, 3, 4, 24)]] + [[0, 0]] * 5
    assert np.isnan(mean[3:, 1:]).all() and np.isfinite(mean[:3]).all() and (counts[:, 0] == 192).all()
    check(layout, 8, 1, radii=(1, 3), centres=centres, seed=22)                      # without centre_valid frame 6 has its disc
    check(layout, 2, 4, radii=(2,), centres=centres * 7.3, sx=0.137, sy=1 / 7.0, seed=23)


def test_lengths_drop_frames_and_their_bytes_do_not_matter():
    layout = SurfaceLayout('nv12', 16, 12)
    centres = centres_for(9, 16, 12, 5)
    sums, counts, mean = check(layout, 3, 3, radii=(3,), centres=centres, lengths=[3, 0, 1], seed=31)
    assert counts[:, 0].tolist() == [192] * 3 + [0] * 3 + [192, 0, 0] and np.isnan(mean[3:6]).all() and not sums[4:6].any()
    check(layout, 3, 3, lengths=[7, -2, 2], seed=32)                                 # clamped to 0 .. T


@pytest.mark.parametrize('fmt', ['rgb', 'nv12', 'i420'])
def test_a_disc_across_a_band_boundary(fmt):
    """A frame of more than two bands; discs whose rows straddle the first boundary, lie inside one band, and cover all bands."""
    Hb = kernels.LUM_BAND_ROWS
    W, H = 24, 2 * Hb + 6
    centres = np.array([[12.0, Hb], [12.0, Hb + Hb / 2.0], [3.0, 2 * Hb + 5.5], [12.0, Hb - 0.25]], np.float32)
    sums, counts, _ = check(SurfaceLayout(fmt, W, H), 4, 1, radii=(3, 5, 2 * H), centres=centres, seed=41)
    assert counts[0, 1] == ref.disc_count(W, H, 3, 24, 2 * Hb) > 0 and (counts[:, 3] == W * H).all()


def test_a_white_2048_by_1088_frame_sums_exactly():
    """The accumulator-width case: every pixel 65535, 2.2 million of them, and a disc of 300 pixels."""
    W, H = 2048, 1088
    layout = SurfaceLayout('rgb', W, H)
    buf = np.full((1, layout.frame_bytes), 255, dtype=np.uint8)
    centres = np.array([[1000.3, 500.2]], np.float32)
    sums, counts, mean = check(layout, 1, 1, radii=(300,), centres=centres, buf=buf, form=GENERIC)
    assert sums[0, 0] == 65535 * W * H and mean[0, 0] == 1.0 and mean[0, 1] == 1.0
    assert abs(int(counts[0, 1]) - np.pi * 300 ** 2) < 2000                           # (check() held it against the reference's)


def test_weights_and_tables_of_the_caller():
    layout = SurfaceLayout('yuyv', 16, 12)
    buf, _ = sref.random_surface(layout, 2, seed=51)
    k = default_kernels()
    table = data.display_response('gamma', gamma=2.2)
    for weights in ((65536, 0, 0), (0, 0, 65536), (19595, 38470, 7471)):
        got = k.screen_luminance(cuda(buf), layout, table.cuda(), weights, 2, 1, matrix='jfif')
        want = ref.luminance(buf, layout, table.numpy(), weights, 2, 1, matrix='jfif')
        for g, w in zip(got, want):
            assert g.cpu().numpy().tobytes() == w.tobytes(), weights


# ---------------------------------------------------------------------------------------------------------------- refusals
def raw_call(k, surf, B=1, T=1, src='buf', response='table', weights=ref.REC709, lengths=None, R=0, radii=None, centres=None, sx=1.0, sy=1.0,
             outs=(True, True, True), matrix=0):
    N = max(1, min(int(B) * int(T), 4))
    hold = {'buf': torch.zeros((N * 16 * 12 * 3,), dtype=torch.uint8, device='cuda'), 'table': table_on_device(),
            'sums': torch.zeros((N * 5,), dtype=torch.int64, device='cuda'), 'counts': torch.zeros((N * 5,), dtype=torch.int32, device='cuda'),
            'mean': torch.zeros((N * 5,), dtype=torch.float32, device='cuda'), 'centres': torch.zeros((N, 2), dtype=torch.float32, device='cuda')}
    p = lambda name: None if name is None else ctypes.c_void_p(hold[name].data_ptr())
    arr = None if radii is None else (ctypes.c_int * len(radii))(*radii)
    status = k.lib.eve_screen_luminance(None if surf is None else ctypes.byref(surf), matrix, B, T, p(src), p(response), weights[0], weights[1],
                                        weights[2], lengths, R, arr, p(centres), sx, sy, None, *[p(n) if on else None for n, on in
                                                                                                 zip(('sums', 'counts', 'mean'), outs)],
                                        k._stream())
    k._ck(status)


def test_the_library_refuses_without_a_launch():
    k = default_kernels()
    good = SurfaceLayout('rgb', 16, 12)
    k.screen_area_surface_to_nchw(torch.zeros((1, good.frame_bytes), dtype=torch.uint8, device='cuda'), (6, 8), good)
    last = k.lib.eve_last_kernel().decode()
    assert last and 'luminance' not in last

    def surface(**over):
        s = good.as_ctypes()
        for name, v in over.items():
            if name in ('offset', 'pitch', 'step'):
                getattr(s, name)[v[0]] = v[1]
            else:
                setattr(s, name, v)
        return s

    bad = [dict(surf=None), dict(surf=surface(struct_bytes=8)), dict(surf=surface(kind=7)), dict(surf=surface(xshift=1)), dict(surf=surface(pitch=(1, 0))),
           dict(surf=surface(offset=(2, -1))), dict(surf=surface(frame_bytes=100)), dict(surf=surface(width=0)),
           dict(surf=SurfaceLayout('nv12', 16, 12).as_ctypes(), matrix=5)]
    big = SurfaceLayout('rgb', 16385, 1).as_ctypes()
    tall = SurfaceLayout('rgb', 1, 16385).as_ctypes()
    bad += [dict(surf=big), dict(surf=tall)]
    bad += [dict(src=None), dict(response=None), dict(outs=(False, True, True)), dict(outs=(True, False, True)), dict(outs=(True, True, False))]
    bad += [dict(B=0), dict(T=0), dict(B=-3), dict(B=2 ** 31, T=1), dict(B=2 ** 29, T=4), dict(B=2 ** 29, T=1, R=4, radii=(1, 2, 3, 4), centres='centres')]
    bad += [dict(weights=w) for w in ((65536, 1, -1), (1, 2, 3), (65536, 65536, -65536), (0, 0, 0), (2 ** 31 - 1, 2 ** 31 - 1, 65538))]
    bad += [dict(R=-1), dict(R=5, radii=(1, 2, 3, 4, 5), centres='centres')]
    bad += [dict(R=2, radii=r, centres='centres') for r in ((0, 1), (1, 16385), (2, 2), (3, 2), (-1, 5))]
    bad += [dict(R=1, radii=(1,)), dict(R=0, centres='centres'), dict(R=1, centres='centres'), dict(R=0, radii=(1,))]
    bad += [{name: v, 'R': 1, 'radii': (1,), 'centres': 'centres'} for name in ('sx', 'sy') for v in (0.0, -1.0, float('nan'), float('inf'))]
    for kw in bad:
        with pytest.raises(RuntimeError, match='screen_luminance:'):
            raw_call(k, **dict(dict(surf=good.as_ctypes()), **kw))
        assert k.lib.eve_last_kernel().decode() == last, kw
    raw_call(k, good.as_ctypes(), R=1, radii=(16384,), centres='centres')              # the limits themselves are taken
    assert k.lib.eve_last_kernel().decode() == GENERIC
    # the wrapper's own checks
    buf = torch.zeros((2, good.frame_bytes), dtype=torch.uint8, device='cuda')
    t = table_on_device()
    with pytest.raises(TypeError, match='layout'):
        k.screen_luminance(buf, 'rgb', t, ref.REC709, 2, 1)
    with pytest.raises(ValueError, match='B x T'):
        k.screen_luminance(buf, good, t, ref.REC709, 3, 1)
    with pytest.raises(ValueError, match='frames'):
        k.screen_luminance(buf[:, :-1].contiguous(), good, t, ref.REC709, 2, 1)
    with pytest.raises(TypeError, match='response'):
        k.screen_luminance(buf, good, t.float(), ref.REC709, 2, 1)
    with pytest.raises(TypeError, match='centres'):
        k.screen_luminance(buf, good, t, ref.REC709, 2, 1, radii=(3,))
    with pytest.raises(TypeError, match='centre_valid'):
        k.screen_luminance(buf, good, t, ref.REC709, 2, 1, radii=(3,), centres=torch.zeros(2, 2, device='cuda'), centre_valid=torch.ones(3, dtype=torch.uint8, device='cuda'))
    with pytest.raises(ValueError, match='matrix'):
        k.screen_luminance(buf, good, t, ref.REC709, 2, 1, matrix='rec2020')


def test_the_stand_alone_call_is_the_kernel_call():
    g = np.random.default_rng(3)
    S, T, W, H = 2, 3, 40, 22
    spec = ScreenLuminanceSpec('lum', radii_px=(24, 64), to_pupil=(0.5, 0.0, 0.5))
    screen = (4 * W, 4 * H)
    pog = cuda((centres_for(S * T, W, H, 9) * 4).reshape(S, T, 2))
    valid = cuda(np.array([[1, 1, 0], [1, 1, 1]], dtype=bool))
    lengths = cuda(np.array([3, 2], np.int32))
    k = default_kernels()
    for fmt, shape in (('nv12', (S, T, H * 3 // 2, W)), ('bgr', (S, T, H, W, 4)), ('yuyv', (S, T, H, W, 2))):
        frames = cuda(g.integers(0, 256, size=shape, dtype=np.uint8))
        out = data.screen_luminance(frames, fmt, spec, screen, pog_px=pog, valid=valid, lengths=lengths, matrix='bt709')
        layout = SurfaceLayout('bgra' if fmt == 'bgr' else fmt, W, H)
        sums, counts, mean = k.screen_luminance(frames.reshape(S * T, -1), layout, table_on_device(), ref.REC709, S, T, radii=(6, 16),
                                                centres=pog.reshape(-1, 2), sx=0.25, sy=0.25, centre_valid=valid.view(torch.uint8).reshape(-1),
                                                lengths=lengths, matrix='bt709')
        assert torch.equal(out['sums'].reshape(-1, 3), sums) and torch.equal(out['counts'].reshape(-1, 3), counts)
        m = mean.cpu().numpy()
        assert out['lum'].cpu().numpy().tobytes() == m[:, 0].tobytes() and out['lum_gaze'].cpu().numpy().tobytes() == np.ascontiguousarray(m[:, 1:]).tobytes()
        assert out['lum_covariate'].cpu().numpy().tobytes() == ref.covariate(m, spec.to_pupil).tobytes()
        want = ref.luminance(frames.cpu().numpy().reshape(S * T, -1), layout, TABLE, ref.REC709, S, T, (6, 16), pog.cpu().numpy().reshape(-1, 2),
                             np.float32(0.25), np.float32(0.25), valid.cpu().numpy().reshape(-1), lengths.cpu().numpy(), 'bt709')
        assert sums.cpu().numpy().tobytes() == want[0].tobytes() and counts[5].tolist() == [0, 0, 0] and counts[2].tolist()[1:] == [0, 0]
    surf = SurfaceLayout('nv21', W, H, pitch=48, coded_height=24)
    buf, _ = sref.random_surface(surf, S * T, seed=4)
    out = data.screen_luminance(cuda(buf).reshape(S, T, -1), surf, ScreenLuminanceSpec(), screen)
    assert out['screen_luminance'].cpu().numpy().tobytes() == ref.luminance(buf, surf, TABLE, ref.REC709, S, T)[2][:, 0].tobytes()


# ---------------------------------------------------------------------------------------------------------------- EVEStream
S, TC = 3, 5
IW, IH = 136, 76                          # RefineNet takes no capture below its own 128 x 72 (no upscaling); 76 rows: three bands


class Recording(object):
    """default_kernels() with the names of the methods called through it."""

    def __init__(self, inner):
        self.inner, self.calls = inner, []

    def __getattr__(self, name):
        v = getattr(self.inner, name)
        if callable(v) and not name.startswith('_'):
            self.calls.append(name)
        return v


@pytest.fixture(scope='module')
def rig():
    """One model and one 3 x 10 clip whose screen is an NV12 capture, shared and never modified."""
    model, _ = make_model(refine_net_rnn_type='CGRU')
    _, d, _ = gpu_clip(S, 2 * TC, seed=7)
    d = {k: v for k, v in d.items() if k != 'screen_frame'}
    g = torch.Generator().manual_seed(6)
    d['screen_frame_nv12'] = torch.randint(0, 256, (S, 2 * TC, IH * 3 // 2, IW), generator=g, dtype=torch.uint8).cuda()
    chunk = lambda t0, t1: {k: v[:, t0:t1].contiguous() for k, v in d.items()}
    W = float(model.config.actual_screen_size[0])
    spec = ScreenLuminanceSpec(radii_px=(4 * W / IW, 14 * W / IW, 7000 * W / IW), to_pupil=(0.5, 0.0, 0.0, 0.5))
    return {'model': model, 'chunks': (chunk(0, TC), chunk(TC, 2 * TC)), 'whole': chunk(0, 2 * TC), 'spec': spec}


def keep(out):
    return {k: v.clone() for k, v in out.items()}


def reference_on(model, out, chunk, spec, lengths=None):
    """The reference on the step's OWN point of gaze and validity."""
    cfg = model.config
    T = chunk['screen_frame_nv12'].shape[1]
    sx, sy = IW / float(cfg.actual_screen_size[0]), IH / float(cfg.actual_screen_size[1])
    valid = out['valid'].cpu().numpy().astype(np.uint8).reshape(-1) if 'eye_valid' in out else None
    return ref.luminance(chunk['screen_frame_nv12'].cpu().numpy().reshape(S * T, -1), SurfaceLayout('nv12', IW, IH), spec.response_table().numpy(),
                         spec.weights, S, T, spec.capture_radii(sx), out['PoG_px_final'].float().cpu().numpy().reshape(-1, 2), np.float32(sx),
                         np.float32(sy), valid, lengths, model.refine_net.yuv_matrix)


def luminance_matches(model, out, chunk, spec, lengths=None):
    sums, counts, mean = reference_on(model, out, chunk, spec, lengths)
    T = mean.shape[0] // S
    assert out['screen_luminance'].cpu().numpy().tobytes() == mean[:, 0].tobytes()
    assert out['screen_luminance_gaze'].cpu().numpy().tobytes() == np.ascontiguousarray(mean[:, 1:]).tobytes()
    assert out['screen_luminance_covariate'].cpu().numpy().tobytes() == ref.covariate(mean, spec.to_pupil).tobytes()
    assert tuple(out['screen_luminance_gaze'].shape) == (S, T, 3)
    return counts


@pytest.mark.parametrize('mode', ['lengths', 'eye_mask'])
def test_stream_luminance_eager_and_captured(rig, mode):
    model, chunks, spec = rig['model'], rig['chunks'], rig['spec']
    if mode == 'lengths':
        kw = dict(lengths=[[5, 0, 4], [5, 3, 5]])
    else:
        mask = torch.ones((S, TC, 2), dtype=torch.bool, device='cuda')
        mask[0, 1] = mask[2, 2] = False
        mask[1, 1:3, 1] = False
        kw = dict(eye_mask=mask)
    at = lambda i: {k: (v[i] if k == 'lengths' else v) for k, v in kw.items()}
    pupil = PupilSpec(fps=30.0, min_mm=1e-3, max_mm=1e3, max_speed_mm_s=1e6, light_tau_s=0.1)
    eager_stream, graph_stream = eve_amd.EVEStream(model, S, use_graph=False), eve_amd.EVEStream(model, S)
    eager = [keep(eager_stream.step(c, luminance=spec, pupil=pupil, **at(i))) for i, c in enumerate(chunks)]
    graph = [keep(graph_stream.step(c, luminance=spec, pupil=pupil, **at(i))) for i, c in enumerate(chunks)]
    assert len(graph_stream._graphs) == 1
    total = 0
    for i, (e, g, c) in enumerate(zip(eager, graph, chunks)):
        assert sorted(e) == sorted(g)
        lengths = np.asarray(kw['lengths'][i]) if mode == 'lengths' else None
        for out in (e, g):
            counts = luminance_matches(model, out, c, spec, lengths)
        total += int((counts[:, 3] > 0).sum())
        print('step', i, 'disc counts', counts[:, 1:].tolist())
        if mode == 'lengths':
            live = np.arange(TC)[None, :] < lengths[:, None]
            assert np.array_equal(np.isfinite(e['screen_luminance'].cpu().numpy()), live)
        else:                                                             # the screen does not care about the eyes; the discs do
            assert torch.isfinite(e['screen_luminance']).all() and torch.isnan(e['screen_luminance_gaze'][0, 1]).all()
        for k in e:
            if k.startswith('pupil_'):
                assert e[k].cpu().numpy().tobytes() == g[k].cpu().numpy().tobytes(), k
    assert total >= 1                                                     # some frame's largest disc meets the screen
    # the pupil stage took the covariate: a step fed the same values as pupil_luminance gives the same pupil bits
    fed_stream = eve_amd.EVEStream(model, S, use_graph=False)
    for i, (e, c) in enumerate(zip(eager, chunks)):
        fed = fed_stream.step(dict(c, pupil_luminance=e['screen_luminance_covariate']), pupil=pupil, **at(i))
        for k in fed:
            if k.startswith('pupil_'):
                assert fed[k].cpu().numpy().tobytes() == e[k].cpu().numpy().tobytes(), (i, k)
    assert float(eager_stream.pupil_table()[:, pupil_ref.N].sum()) > 0            # the light regression saw samples


def test_stream_chunks_equal_one_pass_and_a_plain_step_is_the_parents(rig):
    model, chunks, whole, spec = rig['model'], rig['chunks'], rig['whole'], rig['spec']
    s = eve_amd.EVEStream(model, S, use_graph=False)
    parts = [keep(s.step(c, luminance=spec)) for c in chunks]
    one = keep(eve_amd.EVEStream(model, S, use_graph=False).step(whole, luminance=spec))
    luminance_matches(model, one, whole, spec)
    assert torch.cat([p['screen_luminance'] for p in parts], dim=1).cpu().numpy().tobytes() == one['screen_luminance'].cpu().numpy().tobytes()
    for p, c in zip(parts, chunks):
        luminance_matches(model, p, c, spec)
    # without luminance= : the same launches but one, and the same bits
    rec = Recording(default_kernels())
    kernels.set_default_kernels(rec)
    try:
        eve_amd.EVEStream(model, S, use_graph=False).step(chunks[0])       # (the packs are built at a model's first step)
        del rec.calls[:]
        plain = keep(eve_amd.EVEStream(model, S, use_graph=False).step(chunks[0]))
        calls_plain = list(rec.calls)
        del rec.calls[:]
        lit = keep(eve_amd.EVEStream(model, S, use_graph=False).step(chunks[0], luminance=spec))
        calls_lit = list(rec.calls)
    finally:
        kernels.set_default_kernels(None)
    assert 'screen_luminance' not in calls_plain and calls_lit == calls_plain + ['screen_luminance']
    assert sorted(lit) == sorted(list(plain) + list(spec.result_keys()))
    for k in plain:
        assert lit[k].cpu().numpy().tobytes() == plain[k].cpu().numpy().tobytes(), k
    graph_stream = eve_amd.EVEStream(model, S)
    graph_stream.step(chunks[0], luminance=spec)
    graph_stream.reset()
    back = graph_stream.step(chunks[0])
    assert sorted(back) == sorted(plain)
    for k in plain:
        assert back[k].cpu().numpy().tobytes() == plain[k].cpu().numpy().tobytes(), k
