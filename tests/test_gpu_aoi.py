"""GPU: eve_gaze_aoi against the numpy contract of tests/aoi_ref.py, and EVEStream's step(aoi=...) around it (eager and captured).
Every test here needs the entry point, AoiSpec or the aoi argument, so every one fails without them.

Every comparison with the reference is exact equality -- integers, and the bits of every float: nothing but + - * / and comparisons
of doubles leads to any of them."""
import numpy as np
import pytest
import torch

import aoi_ref as ref
import eve_amd
from eve_amd import data
from eve_amd.data import AoiSpec, GazeEventSpec
from eve_amd.kernels import default_kernels
from test_gpu_calibration import cuda, guarded, guards_hold
from test_gpu_stream import gpu_clip, make_model

pytestmark = pytest.mark.gpu
KEYS = ('id', 'mask', 'visit_ms')
OUT_DTYPES = {'id': torch.int32, 'mask': torch.int64, 'visit_ms': torch.float32}
CARRIED = ('state', 'table', 'trans', 'visits', 'count', 'dropped')
NAN_ROW = ref.rect(0, 0, 2000, 2000)
NAN_ROW[5] = np.nan
SEVEN = [(500, 100), (800, 100), (800, 400), (650, 400), (650, 250), (600, 250), (500, 400)]      # concave: a notch from below
FIVE = np.stack([ref.rect(100, 100, 300, 250), ref.ellipse(300, 200, 120, 80), ref.polygon(SEVEN), ref.disabled(), NAN_ROW])
# points on edges and vertices, in the overlap, in the notch, and outside everything
POOL = [(100, 100), (299.5, 249.5), (300, 150), (200, 250), (420, 200), (300, 280), (300, 120), (250, 200), (650, 300), (625, 300), (625, 250),
        (500, 250), (800, 200), (700, 100), (700, 400), (575, 250), (550, 300), (900, 500), (50, 50), (420.01, 200), (180, 180), (720, 180)]


def seventy(seed=11):
    """B = 3, T = 70 (more than one pass of 64), A = 5: a rectangle, an ellipse that overlaps it, a concave 7-gon, a disabled row and a
    NaN row; points from POOL held for one to four frames; a 60 Hz clock with gaps above max_gap_s, a NaN, an infinity, a stall and a
    step backwards; invalid frames through both validity inputs, NaN and infinite points, fixation ids that change inside and
    across AOIs."""
    rng = np.random.RandomState(seed)
    B, T = 3, 70
    pog = np.zeros((B, T, 2), np.float32)
    for b in range(B):
        f = 0
        while f < T:
            n = rng.randint(1, 5)
            pog[b, f:f + n] = POOL[rng.randint(len(POOL))]
            f += n
    dt = rng.uniform(0.014, 0.019, (B, T))
    dt[rng.rand(B, T) < 0.05] = 0.3
    frame_time = np.cumsum(dt, axis=1) + 50.0 * np.arange(B)[:, None]
    frame_time[0, 30], frame_time[0, 44], frame_time[0, 65] = np.nan, np.inf, frame_time[0, 64]
    frame_time[1, 5] = frame_time[1, 4] - 2.0
    valid, valid_key = (rng.rand(B, T) > 0.06).astype(np.uint8), (rng.rand(B, T) > 0.04).astype(np.uint8)
    pog[0, 12, 0], pog[0, 63, 1], pog[1, 7] = np.nan, -np.inf, np.nan
    fixation_id = np.repeat(np.arange(T // 5 + 1), 5)[:T][None].repeat(B, 0).astype(np.int32) + 3
    fixation_id[rng.rand(B, T) < 0.08] = -1
    fixating = (rng.rand(B, T) > 0.25).astype(np.uint8)
    return dict(pog=pog, shapes=np.tile(FIVE[None], (B, 1, 1)), frame_time=frame_time, valid=valid, valid_key=valid_key, fixation_id=fixation_id,
                fixating=fixating)


FRAME_INPUTS = ('frame_time', 'valid', 'valid_key', 'fixation_id', 'fixating')


def ref_run(spec, sc, buffers, t0=0, t1=None, **kw):
    cut = lambda a: a[:, t0:t1]
    return ref.run(spec, cut(sc['pog']), sc['shapes'] if sc['shapes'].ndim == 3 else cut(sc['shapes']), *buffers,
                   **dict({k: cut(sc[k]) for k in FRAME_INPUTS if sc.get(k) is not None}, **kw))


def device_buffers(buffers):
    return [cuda(a) for a in buffers]


def device_run(spec, sc, buffers, t0=0, t1=None, **kw):
    """The wrapper on the device copies of the scene's frames t0 .. t1; buffers: device tensors, updated in place."""
    cut = lambda a: cuda(a[:, t0:t1])
    return default_kernels().gaze_aoi(cut(sc['pog']), cuda(sc['shapes']) if sc['shapes'].ndim == 3 else cut(sc['shapes']), spec, *buffers,
                                      **dict({k: cut(sc[k]) for k in FRAME_INPUTS if sc.get(k) is not None},
                                             **{k: cuda(np.asarray(v, np.int32)) for k, v in kw.items()}))


def assert_same(got, want, buffers, want_buffers):
    for k in KEYS:
        g = got[k].cpu().numpy()
        assert g.dtype == want[k].dtype and g.tobytes() == want[k].tobytes(), k
    for name, g, w in zip(CARRIED, buffers, want_buffers):
        assert g.cpu().numpy().dtype == w.dtype and g.cpu().numpy().tobytes() == w.tobytes(), name


def raw_call(spec, B, T, A, pog, shapes, per_frame, buffers, outs, frame_time=None, valid=None, valid_key=None, fixation_id=None, fixating=None,
             lengths=None, reset=None, flush=None, capacity=None):
    """The C entry point itself, so that everything can lie between guards and bad arguments reach the library."""
    k = default_kernels()
    p = k._p
    state, table, trans, visits, count, dropped = buffers
    k._ck(k.lib.eve_gaze_aoi(B, T, A, p(pog), p(shapes), per_frame, p(frame_time), p(valid), p(valid_key), p(fixation_id), p(fixating), p(lengths),
                             p(reset), p(flush), 0.0 if spec.fps is None else spec.fps, spec.max_gap_s, p(state), p(table), p(trans),
                             (capacity if capacity is not None else 2 if visits is None else visits.shape[1]), p(visits), p(count), p(dropped),
                             *[None if outs is None else p(outs[k_]) for k_ in KEYS], k._stream()))
    assert k.lib.eve_last_kernel().decode() == 'gaze_aoi_kernel'


# ---------------------------------------------------------------------------------------------------------------- the kernel
def test_every_kind_of_frame_and_shape_in_one_launch():
    """Every stream arrives with an open visit (six frames inside the rectangle).  lengths (70, 13, 0); stream 1 is reset (its open
    visit goes to the store, its row starts afresh, the visit counter runs on), stream 0 is flushed, stream 2 gets no frame and keeps
    its row.  Every buffer lies between guards."""
    sc = seventy()
    spec = ref.Spec(max_gap_s=0.075)
    B, T, A, V = 3, 70, 5, 40
    want_buffers = ref.fresh(B, A, V)
    pre = dict(pog=np.tile(np.float32([[200, 200]]), (B, 6, 1)), shapes=sc['shapes'], frame_time=np.tile(np.arange(-6, 0) / 60.0, (B, 1)) + 50.0 * np.arange(B)[:, None])
    ref_run(spec, pre, want_buffers)
    assert (want_buffers[0][:, ref.OPEN] == 1).all() and not want_buffers[4].any()
    lengths, reset, flush = (np.array(a, np.int32) for a in ([70, 13, 0], [0, 1, 0], [1, 0, 0]))
    sentinels = {'state': -777.25, 'table': -777.25, 'trans': -7, 'visits': -777.25, 'count': -7, 'dropped': -7}
    wholes, buffers = {}, []
    for name, a in zip(CARRIED, want_buffers):
        wholes[name], payload = guarded(a.shape, torch.from_numpy(a).dtype, sentinels[name])
        payload.copy_(cuda(a))
        buffers.append(payload)
    outs = {}
    for k, dtype in OUT_DTYPES.items():
        wholes[k], outs[k] = guarded((B, T), dtype, 99)
        sentinels[k] = 99
    want = ref_run(spec, sc, want_buffers, lengths=lengths, reset=reset, flush=flush)
    state, table, trans, visits, count, dropped = want_buffers
    # what the case is meant to hold, asserted on the reference alone
    ids = want['id']
    assert set(ids[0].tolist()) == {-2, -1, 0, 1, 2} and (ids[1, 13:] == -2).all() and (ids[2] == -2).all()
    assert ((want['mask'] & 3) == 3).any() and ids[0, 30] == ids[0, 44] == ids[0, 65] == ids[0, 12] == ids[0, 63] == -2 and ids[1, 5] == ids[1, 7] == -2
    assert state[0, ref.OPEN] == 0 and state[2, ref.OPEN] == 1 and count[1] >= 1 and visits[1, 0, 3] == 6 and state[2, ref.TICKS] == 6 and state[1, ref.TICKS] == 13
    assert (table[0, :3, 5] > 1).all() and count[0] > 8 and not dropped.any() and (trans[0].sum(axis=0)[:3] == table[0, :3, 2]).all()
    raw_call(spec, B, T, A, cuda(sc['pog']), cuda(sc['shapes']), 0, buffers, outs, *[cuda(sc[k]) for k in FRAME_INPUTS], cuda(lengths), cuda(reset), cuda(flush))
    torch.cuda.synchronize()
    assert_same(outs, want, buffers, want_buffers)
    for name, whole in wholes.items():
        assert guards_hold(whole, sentinels[name]), name


def test_sixty_four_aois_and_one():
    spec = ref.Spec(fps=30.0)
    grid = np.stack([ref.rect(10 * (i % 8), 10 * (i // 8), 10 * (i % 8) + 10, 10 * (i // 8) + 10) for i in range(64)])
    sc = dict(pog=np.float32([[[75, 75], [5, 5], [15, 5]]]), shapes=grid[None])
    want_buffers, buffers = ref.fresh(1, 64, 4), device_buffers(ref.fresh(1, 64, 4))
    want = ref_run(spec, sc, want_buffers)
    assert want['id'].tolist() == [[63, 0, 1]] and want['mask'].tolist() == [[-2 ** 63, 1, 2]]      # bit 63 alone: the int64's sign
    assert_same(device_run(spec, sc, buffers), want, buffers, want_buffers)
    assert buffers[2][0, 64, 63] == 1 and buffers[2][0, 63, 0] == 1 and buffers[1][0, 63, 2] == 1
    # all 64 overlapping: every bit set
    sc = dict(pog=np.float32([[[75, 75], [5, 5], [-1, 5]]]), shapes=np.tile(ref.rect(0, 0, 100, 100), (1, 64, 1)))
    want_buffers, buffers = ref.fresh(1, 64, 4), device_buffers(ref.fresh(1, 64, 4))
    want = ref_run(spec, sc, want_buffers)
    assert want['mask'].tolist() == [[-1, -1, 0]] and want['id'].tolist() == [[0, 0, -1]]
    assert_same(device_run(spec, sc, buffers), want, buffers, want_buffers)
    # A = 1: one polygon of 16 vertices (a star: concave at every other vertex)
    star = [(100 + (40 if i % 2 == 0 else 15) * np.cos(i * np.pi / 8), 100 + (40 if i % 2 == 0 else 15) * np.sin(i * np.pi / 8)) for i in range(16)]
    sc = dict(pog=np.float32([[[100, 100], [138, 100], [125, 112]]]), shapes=ref.polygon(star)[None, None])
    want_buffers, buffers = ref.fresh(1, 1, 4), device_buffers(ref.fresh(1, 1, 4))
    want = ref_run(spec, sc, want_buffers)
    assert want['id'].tolist() == [[0, 0, -1]] and want['mask'].tolist() == [[1, 1, 0]]      # the centre, a tip, the gap between two tips
    assert_same(device_run(spec, sc, buffers), want, buffers, want_buffers)


def test_moving_regions():
    """shapes [B, T, A, 36]: a rectangle slides under a still point (stream 0), and over a point that follows it (stream 1)."""
    B, T, A = 2, 9, 2
    spec = ref.Spec(fps=30.0)
    shapes = np.zeros((B, T, A, 36), np.float32)
    for f in range(T):
        shapes[:, f, 0] = ref.rect(10 * f, 40, 10 * f + 15, 60)
        shapes[:, f, 1] = ref.ellipse(500, 500, 30, 30)
    pog = np.zeros((B, T, 2), np.float32)
    pog[0] = (50, 50)
    pog[1, :, 0], pog[1, :, 1] = 10 * np.arange(T) + 5, 50
    sc = dict(pog=pog, shapes=shapes)
    want_buffers, buffers = ref.fresh(B, A, 4), device_buffers(ref.fresh(B, A, 4))
    want = ref_run(spec, sc, want_buffers, flush=np.ones(B, np.int32))
    assert want['id'].tolist() == [[-1, -1, -1, -1, 0, 0, -1, -1, -1], [0] * 9]
    assert want_buffers[3][0, 0].tolist() == [0, 4 / 30.0, 5 / 30.0, 2, 0, 0, 0, 0] and want_buffers[1][1, 0, 0] == 8 / 30.0
    assert_same(device_run(spec, sc, buffers, flush=[1, 1]), want, buffers, want_buffers)


def test_chunks_equal_one_pass_on_the_device():
    sc = seventy()
    spec = ref.Spec(max_gap_s=0.075)
    lengths = np.array([70, 13, 0])
    want_buffers = ref.fresh(3, 5, 40)
    want = ref_run(spec, sc, want_buffers, lengths=lengths, flush=np.ones(3, np.int32))
    whole = device_buffers(ref.fresh(3, 5, 40))
    got = device_run(spec, sc, whole, lengths=lengths, flush=[1, 1, 1])
    assert_same(got, want, whole, want_buffers)
    parts, outs, t0 = device_buffers(ref.fresh(3, 5, 40)), [], 0
    for n in (1, 63, 6):
        more = dict(flush=[1, 1, 1]) if t0 + n == 70 else {}
        outs.append(device_run(spec, sc, parts, t0, t0 + n, lengths=np.clip(lengths - t0, 0, n), **more))
        t0 += n
    assert_same({k: torch.cat([o[k] for o in outs], dim=1) for k in KEYS}, want, parts, want_buffers)
    # counted time: the ticks carry the clock over the cuts
    spec = ref.Spec(fps=60.0)
    sc = {k: v for k, v in sc.items() if k != 'frame_time'}
    want_buffers = ref.fresh(3, 5, 40)
    want = ref_run(spec, sc, want_buffers, lengths=lengths)
    parts, outs, t0 = device_buffers(ref.fresh(3, 5, 40)), [], 0
    for n in (1, 63, 6):
        outs.append(device_run(spec, sc, parts, t0, t0 + n, lengths=np.clip(lengths - t0, 0, n)))
        t0 += n
    assert_same({k: torch.cat([o[k] for o in outs], dim=1) for k in KEYS}, want, parts, want_buffers)
    assert want_buffers[0][:, ref.TICKS].tolist() == [70, 13, 0]


def test_a_full_visit_store_drops_and_counts():
    spec = ref.Spec(fps=30.0)
    two = np.stack([ref.rect(0, 0, 10, 10), ref.rect(20, 0, 30, 10)])[None]
    sc = dict(pog=np.float32([[[5, 5], [5, 5], [25, 5], [5, 5], [25, 5], [25, 5], [5, 5]]]), shapes=two)      # five visits: 0 1 0 1 0
    want_buffers, buffers = ref.fresh(1, 2, 2), device_buffers(ref.fresh(1, 2, 2))
    want = ref_run(spec, sc, want_buffers, flush=np.ones(1, np.int32))
    assert want_buffers[4].tolist() == [2] and want_buffers[5].tolist() == [3]
    assert_same(device_run(spec, sc, buffers, flush=[1]), want, buffers, want_buffers)
    roomy = ref.fresh(1, 2, 8)
    ref_run(spec, sc, roomy, flush=np.ones(1, np.int32))
    assert roomy[4].tolist() == [5] and buffers[1].cpu().numpy().tobytes() == roomy[1].tobytes() and np.array_equal(buffers[2].cpu().numpy(), roomy[2])
    assert np.array_equal(buffers[3].cpu().numpy()[0], roomy[3][0, :2]) and buffers[2].cpu().numpy()[0].tolist() == [[0, 2], [2, 0], [1, 0]]


def test_the_stand_alone_call_is_the_kernel_call():
    sc = seventy()
    spec = AoiSpec('roi', 5, max_gap_s=0.075)
    buffers = device_buffers(ref.fresh(3, 5, 256))
    sc = {k: v for k, v in sc.items() if k != 'valid_key'}
    want = device_run(spec, sc, buffers, flush=[1, 1, 1])
    got = data.gaze_aoi(spec, cuda(sc['pog']), cuda(sc['shapes']), frame_time=cuda(sc['frame_time']), valid=cuda(sc['valid']) != 0,
                        fixation_id=cuda(sc['fixation_id']), fixating=cuda(sc['fixating']))
    assert sorted(got) == sorted(['roi_id', 'roi_mask', 'roi_visit_ms', 'table', 'transitions', 'visits', 'visit_count', 'visit_dropped', 'state'])
    for k in KEYS:
        assert torch.equal(got['roi_' + k], want[k]), k
    for k, b_ in zip(('state', 'table', 'transitions', 'visits', 'visit_count', 'visit_dropped'), buffers):
        assert got[k].cpu().numpy().tobytes() == b_.cpu().numpy().tobytes(), k
    assert int(got['visit_count'].min()) > 5 and not got['state'][:, ref.OPEN].any()
    with pytest.raises(ValueError, match='fps'):
        data.gaze_aoi(spec, cuda(sc['pog']), cuda(sc['shapes']))
    with pytest.raises(TypeError, match='shapes'):
        data.gaze_aoi(AoiSpec(num_aois=4, fps=30), cuda(sc['pog']), cuda(sc['shapes']))
    with pytest.raises(TypeError, match='frame_time'):
        data.gaze_aoi(spec, cuda(sc['pog']), cuda(sc['shapes']), frame_time=torch.zeros((3, 70), device='cuda'))
    with pytest.raises(ValueError, match='fixating'):
        data.gaze_aoi(AoiSpec(num_aois=5, fps=30), cuda(sc['pog']), cuda(sc['shapes']), fixation_id=cuda(sc['fixation_id']))


def test_the_library_refuses_without_a_launch():
    k = default_kernels()
    spec = ref.Spec(fps=30.0)
    B, T, A = 1, 2, 2
    z = lambda *s, dtype=torch.float32: torch.zeros(s, dtype=dtype, device='cuda')
    buffers = device_buffers(ref.fresh(B, A, 2))
    buffers[0][0, ref.NEXT_INDEX] = 5.0
    outs = {k_: z(B, T, dtype=d) for k_, d in OUT_DTYPES.items()}
    pog, shapes, fid, fix = z(B, T, 2), z(B, A, 36), z(B, T, dtype=torch.int32), z(B, T, dtype=torch.uint8)
    call = lambda spec_=spec, B_=B, T_=T, A_=A, pog_=pog, shapes_=shapes, buffers_=buffers, outs_=outs, **kw: raw_call(
        spec_, B_, T_, A_, pog_, shapes_, 0, buffers_, outs_, **kw)
    without = lambda i: [None if j == i else t for j, t in enumerate(buffers)]
    bad = [dict(buffers_=without(i)) for i in range(6)]                                     # null carried buffers
    bad += [dict(B_=0), dict(T_=-1), dict(A_=0), dict(A_=65), dict(capacity=0)]
    bad += [dict(pog_=None), dict(shapes_=None), dict(outs_=dict(outs, id=None)), dict(outs_=dict(outs, mask=None)), dict(outs_=dict(outs, visit_ms=None))]
    bad += [dict(fixation_id=fid), dict(fixating=fix)]                                      # one without the other
    bad += [dict(B_=2 ** 31 // 16), dict(T_=2 ** 30), dict(capacity=2 ** 29)]               # index products past 31 bits
    bad += [dict(spec_=ref.Spec(fps=30.0, max_gap_s=v)) for v in (0.0, -1.0, float('nan'), float('inf'))]
    bad += [dict(spec_=ref.Spec(fps=v)) for v in (0.0, -30.0, float('nan'), float('inf'))]   # no frame_time: fps counts
    for kw in bad:
        with pytest.raises(RuntimeError, match='gaze_aoi'):
            call(**kw)
    with pytest.raises(TypeError, match='state'):
        k.gaze_aoi(pog, shapes, spec, buffers[0].float(), *buffers[1:])
    with pytest.raises(TypeError, match='shapes'):
        k.gaze_aoi(pog, z(B, A, 35), spec, *buffers)
    with pytest.raises(TypeError, match='trans'):
        k.gaze_aoi(pog, shapes, spec, buffers[0], buffers[1], buffers[2].long(), *buffers[3:])
    with pytest.raises(TypeError, match='together'):
        k.gaze_aoi(pog, shapes, spec, *buffers, fixation_id=fid)
    torch.cuda.synchronize()
    want = ref.fresh(B, A, 2)
    want[0][0, ref.NEXT_INDEX] = 5.0
    for g, w in zip(buffers, want):
        assert g.cpu().numpy().tobytes() == w.tobytes()
    # with frame_time a bad fps does not matter; T = 0 needs no frame pointer and only resets and flushes
    call(spec_=ref.Spec(fps=0.0), frame_time=z(B, T, dtype=torch.float64))
    raw_call(ref.Spec(), B, 0, A, None, None, 0, buffers, None, reset=cuda(np.ones(B, np.int32)))
    torch.cuda.synchronize()
    assert buffers[0].cpu().numpy()[0].tolist() == [0.0] * ref.NEXT_INDEX + [5.0] + [0.0] * 4


# ---------------------------------------------------------------------------------------------------------------- EVEStream
S, TC, NA = 3, 5, 6


@pytest.fixture(scope='module')
def rig():
    """One model, one 3 x 10 clip and one table of regions laid around the clip's own points of gaze, shared and never modified: the
    four quadrants around the points' median as rectangles, an ellipse on the median above them in the z-order, and a triangle."""
    model, _ = make_model(refine_net_rnn_type='CGRU')
    _, d, _ = gpu_clip(S, 2 * TC, seed=7)
    chunk = lambda t0, t1: {k: v[:, t0:t1].contiguous() for k, v in d.items()}
    chunks = (chunk(0, TC), chunk(TC, 2 * TC))
    probe = eve_amd.EVEStream(model, S, use_graph=False)
    p = torch.cat([probe.step(c)['PoG_px_final'].clone() for c in chunks], dim=1).double().cpu().numpy().reshape(-1, 2)
    assert np.isfinite(p).all()
    mx, my = np.median(p[:, 0]), np.median(p[:, 1])
    rx, ry = max(np.abs(p[:, 0] - mx).mean() / 2, 1.0), max(np.abs(p[:, 1] - my).mean() / 2, 1.0)
    big = 1e6
    table = data.aoi_shapes([('ellipse', mx, my, rx, ry), ('rect', mx - big, my - big, mx, my), ('rect', mx, my - big, mx + big, my),
                             ('rect', mx - big, my, mx, my + big), ('polygon', [(mx, my), (mx + big, my), (mx + big, my + big)]), None], NA)
    shapes = table[None].repeat(S, 1, 1).cuda()
    return {'model': model, 'chunks': tuple(dict(c, aoi_shapes=shapes) for c in chunks)}


def keep(out):
    return {k: v.clone() for k, v in out.items()}


def two_steps(stream, chunks, lengths=None, **kw):
    outs = []
    for i, chunk in enumerate(chunks):
        if lengths is not None:
            kw['lengths'] = lengths[i]
        outs.append(keep(stream.step(chunk, **kw)))
    return outs


def specified(a, out):
    return a[out['valid']] if 'valid' in out and tuple(a.shape[:2]) == tuple(out['valid'].shape) else a


def stream_buffers(stream, name='aoi'):
    st = stream.get_aoi_state()[name]
    return [st[k] for k in ('state', 'table', 'transitions', 'visits', 'count', 'dropped')]


def reference_on(outs, chunks, spec, source='PoG_px_final', lengths=None, name='aoi', fixations=False, valid_key=None):
    """The reference on the steps' OWN source point (and the events' own outputs), the buffers carried between the steps."""
    buffers = ref.fresh(S, NA, 256)
    for i, (out, chunk) in enumerate(zip(outs, chunks)):
        n = lambda t: t.cpu().numpy()
        kw = {}
        if fixations:
            kw.update(fixation_id=n(out['fixation_id']), fixating=n(out['fixating']))
        if valid_key is not None:
            kw['valid_key'] = n(out[valid_key])
        want = ref.run(spec, n(out[source]), n(chunk['aoi_shapes']), *buffers, valid=n(out['valid']) if 'eye_valid' in out else None,
                       lengths=None if lengths is None else np.asarray(lengths[i]), **kw)
        where = n(out['valid']) if 'valid' in out else np.ones((S, TC), bool)
        for k in KEYS:
            g = n(out['%s_%s' % (name, k)])
            assert g.dtype == want[k].dtype and g[where].tobytes() == want[k][where].tobytes(), (i, k)
    return buffers


@pytest.mark.parametrize('mode', ['lengths', 'eye_mask'])
def test_stream_aoi_eager_and_captured(rig, mode):
    model, chunks = rig['model'], rig['chunks']
    spec = AoiSpec(num_aois=NA, fps=30)
    if mode == 'lengths':
        kw = dict(lengths=[[5, 0, 4], [5, 3, 5]])
    else:
        mask = torch.ones((S, TC, 2), dtype=torch.bool, device='cuda')
        mask[0, 1, 0] = mask[0, 3, 1] = mask[2, 2, 0] = mask[2, 2, 1] = False
        mask[1, :, 1] = False
        kw = dict(eye_mask=mask)
    eager_stream, graph_stream = eve_amd.EVEStream(model, S, use_graph=False), eve_amd.EVEStream(model, S)
    first_eager = keep(eager_stream.step(chunks[0], aoi=spec, **{k: (v[0] if k == 'lengths' else v) for k, v in kw.items()}))
    first_graph = keep(graph_stream.step(chunks[0], aoi=spec, **{k: (v[0] if k == 'lengths' else v) for k, v in kw.items()}))
    # the tallies after the FIRST captured step of a shape: the capture's two warm-up steps were put back (_carried())
    for e, g in zip(stream_buffers(eager_stream), stream_buffers(graph_stream)):
        assert e.cpu().numpy().tobytes() == g.cpu().numpy().tobytes()
    second = {k: (v[1] if k == 'lengths' else v) for k, v in kw.items()}
    eager = [first_eager, keep(eager_stream.step(chunks[1], aoi=spec, **second))]
    graph = [first_graph, keep(graph_stream.step(chunks[1], aoi=spec, **second))]
    for e, g in zip(eager, graph):
        assert sorted(e) == sorted(g)
        for k in e:
            assert specified(e[k], e).cpu().numpy().tobytes() == specified(g[k], e).cpu().numpy().tobytes(), k
    assert len(graph_stream._graphs) == 1                                # the second step replayed the first one's graph
    buffers = reference_on(eager, chunks, spec, lengths=kw.get('lengths'))
    for s_ in (eager_stream, graph_stream):
        for name, g, w in zip(CARRIED, stream_buffers(s_), buffers):
            assert g.cpu().numpy().tobytes() == w.tobytes(), name
    assert buffers[0][:, ref.TICKS].tolist() == ([10, 3, 9] if mode == 'lengths' else [10, 10, 10])
    assert buffers[1][:, :, 1].sum() >= 20 and len(set(torch.cat([e['aoi_id'] for e in eager]).flatten().tolist()) - {-2, -1}) >= 2
    # without aoi= the same EVEStream returns the plain step's bits and leaves the tallies alone
    plain = keep(eve_amd.EVEStream(model, S).step(chunks[0], **{k: (v[0] if k == 'lengths' else v) for k, v in kw.items()}))
    graph_stream.reset()
    back = graph_stream.step(chunks[0], **{k: (v[0] if k == 'lengths' else v) for k, v in kw.items()})
    assert sorted(back) == sorted(plain)
    for k in plain:
        assert specified(back[k], plain).cpu().numpy().tobytes() == specified(plain[k], plain).cpu().numpy().tobytes(), k
    assert graph_stream.aoi_table().cpu().numpy().tobytes() == buffers[1].tobytes()


def test_stream_fixation_based_aoi_with_events(rig):
    model, chunks = rig['model'], rig['chunks']
    events = GazeEventSpec(fps=30, saccade_deg_s=1e9, min_fixation_s=0.03)     # everything fixates: one fixation per stream from frame 1 on
    spec = AoiSpec('fix', NA, source='fixation_px', valid_key='fixating', fps=30)
    eager = two_steps(eve_amd.EVEStream(model, S, use_graph=False), chunks, events=events, aoi=spec)
    graph_stream = eve_amd.EVEStream(model, S)
    graph = two_steps(graph_stream, chunks, events=events, aoi=spec)
    for e, g in zip(eager, graph):
        for k in e:
            assert e[k].cpu().numpy().tobytes() == g[k].cpu().numpy().tobytes(), k
    buffers = reference_on(eager, chunks, spec, source='fixation_px', name='fix', fixations=True, valid_key='fixating')
    for name, g, w in zip(CARRIED, stream_buffers(graph_stream, 'fix'), buffers):
        assert g.cpu().numpy().tobytes() == w.tobytes(), name
    assert eager[0]['fix_id'][:, :2].tolist() == [[-2, -2]] * S and (eager[1]['fix_id'] >= -1).all()
    assert buffers[1][:, :NA, 5].sum() >= S              # every stream's one fixation was counted in at least one AOI


def test_stream_reset_closes_the_visit_and_keeps_the_tallies(rig):
    model, chunks = rig['model'], rig['chunks']
    whole = data.aoi_shapes([('rect', -1e7, -1e7, 1e7, 1e7)], 1)[None].repeat(S, 1, 1).cuda()      # one region that holds every point
    chunks = [dict(c, aoi_shapes=whole) for c in chunks]
    spec = AoiSpec(num_aois=1, fps=30)
    stream = eve_amd.EVEStream(model, S, visit_capacity=4)
    first = keep(stream.step(chunks[0], aoi=spec))
    assert first['aoi_id'].tolist() == [[0] * 5] * S and stream.aoi_visit_counts()[0].tolist() == [0, 0, 0]
    stream.reset([1])
    second = keep(stream.step(chunks[1], aoi=spec))
    count, dropped = stream.aoi_visit_counts()
    assert count.tolist() == [0, 1, 0] and dropped.tolist() == [0, 0, 0]
    assert stream.aoi_visits([1])[0].tolist() == [[0, 0.0, 4 / 30.0, 5, 0, 0, 0, 0]]
    assert np.allclose(second['aoi_visit_ms'][:, 4].cpu().numpy(), [1000 * 9 / 30.0, 1000 * 4 / 30.0, 1000 * 9 / 30.0])
    table = stream.aoi_table().cpu().numpy()
    assert table[:, 0, 1].tolist() == [10, 10, 10] and table[:, 0, 2].tolist() == [1, 2, 1]      # the tallies ran on over the reset
    t, dwell = np.arange(5) / 30.0, np.float64(0.0)
    for _ in range(2):                                   # stream 1: two visits of five samples, each on a clock that starts at 0
        for i in range(1, 5):
            dwell = dwell + (t[i] - t[i - 1])
    assert table[1, 0, 0] == dwell
    assert stream.aoi_transitions()[:, 1, 0].tolist() == [1, 2, 1]
    state = stream.get_aoi_state()['aoi']['state'].cpu().numpy()
    assert state[:, ref.TICKS].tolist() == [10, 5, 10] and state[:, ref.NEXT_INDEX].tolist() == [1, 2, 1]
    # a reset before a step without aoi= still ends the visit; flush ends the others
    stream.reset([0])
    stream.step(chunks[0])
    assert stream.aoi_visit_counts()[0].tolist() == [1, 1, 0] and stream.get_aoi_state()['aoi']['state'][0, ref.OPEN] == 0
    stream.flush_aoi_visits()
    assert stream.aoi_visit_counts()[0].tolist() == [1, 2, 1] and [v[-1, 3] for v in stream.aoi_visits()] == [10, 5, 10]
    stream.clear_aoi(streams=[1])
    assert stream.aoi_visit_counts()[0].tolist() == [1, 0, 1] and not stream.aoi_table()[1].any()
