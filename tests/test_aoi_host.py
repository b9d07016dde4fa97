"""CPU: areas of interest -- the numpy contract (tests/aoi_ref.py) against an independent, slow formulation and its own properties,
point placement, chunk splits, eve_amd.AoiSpec, data.aoi_shapes, and the EVEStream plumbing (step(aoi=...), the refusals, the graph
key, reset, the readouts) over a stand-in whose gaze_aoi is the reference itself.  The GPU suite (test_gpu_aoi.py) checks the HIP
kernel."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import aoi_ref as ref
import eve_amd
from eve_amd import data, kernels
from eve_amd.data import AoiSpec, GazeEventSpec
from test_gaze_events_host import EventOverlayFakes
from test_stream_host import chunk_of, clip, make_model

KEYS = ('id', 'mask', 'visit_ms')


# ---------------------------------------------------------------------------------------------------------------- the slow formulation
def slow_contains(row, x, y):
    """The hit test in exact rational arithmetic (integer-valued coordinates and points)."""
    kind = int(row[0])
    c = [Fraction(int(v)) for v in row[4:]]
    x, y = Fraction(int(x)), Fraction(int(y))
    if kind == 1:
        return c[0] <= x < c[2] and c[1] <= y < c[3]
    if kind == 2:
        return ((x - c[0]) / c[2]) ** 2 + ((y - c[1]) / c[3]) ** 2 <= 1
    if kind == 3:
        n, crossings = int(row[1]), 0
        for i in range(n):
            (xi, yi), (xj, yj) = (c[2 * i], c[2 * i + 1]), (c[2 * ((i - 1) % n)], c[2 * ((i - 1) % n) + 1])
            if (yi > y) != (yj > y) and x < xi + (xj - xi) * (y - yi) / (yj - yi):      # the edge crosses the ray to +x at this height
                crossings += 1
        return crossings % 2 == 1
    return False


def slow_run(spec, pog, shapes, A, capacity, frame_time, valid, fixation_id, fixating, lengths):
    """From fresh state, no reset, flushed at the end: per-frame brute force, then the tallies from the list of samples -- runs of
    connected samples in one AOI are the visits."""
    B, T = pog.shape[:2]
    ids, masks, ms = np.full((B, T), -2, np.int32), np.zeros((B, T), np.int64), np.zeros((B, T), np.float32)
    table, trans = np.zeros((B, A + 1, 8)), np.zeros((B, A + 1, A), np.int32)
    visits, count = np.zeros((B, capacity, 8)), np.zeros(B, np.int32)
    for b in range(B):
        samples, t_prev = [], None
        for f in range(int(lengths[b])):
            tt = frame_time[b, f]
            x, y = pog[b, f]
            if not valid[b, f] or not np.isfinite([x, y, tt]).all() or (t_prev is not None and not tt > t_prev):
                continue
            hits = [a for a in range(A) if slow_contains(shapes[b, a], x, y)]
            samples.append((f, tt, hits[0] if hits else -1, None if t_prev is None else tt - t_prev))
            masks[b, f] = sum(1 << a for a in hits)
            ids[b, f] = hits[0] if hits else -1
            t_prev = tt
        runs = []                                        # [aoi, [(f, tt, dt or None)]]: maximal, connected, one AOI
        for f, tt, a, dt in samples:
            connected = dt is not None and not dt > spec.max_gap_s
            if runs and connected and runs[-1][0] == a:
                runs[-1][1].append((f, tt, dt))
            else:
                runs.append([a, [(f, tt, None)]])
        last, counted, index = A, None, 0
        for a, members in runs:
            row = table[b, a if a >= 0 else A]
            row[1] += len(members)
            for _, _, dt in members[1:]:
                row[0] = row[0] + dt                     # (in time order: the contract's order of additions)
            if a < 0:
                continue
            t_enter, t_last = members[0][1], members[-1][1]
            if row[2] == 0:
                row[3] = t_enter
            row[2] += 1
            row[4] = t_last
            trans[b, last, a] += 1
            last = a
            fixations = 0
            for f, tt, _ in members:
                ms[b, f] = np.float32(np.float64(1000.0) * (tt - t_enter))
                if fixating[b, f] and fixation_id[b, f] >= 0 and counted != (int(fixation_id[b, f]), a):
                    counted = (int(fixation_id[b, f]), a)
                    if row[5] == 0:
                        row[6] = tt
                    row[5] += 1
                    fixations += 1
            visits[b, count[b]] = (a, t_enter, t_last, len(members), fixations, index, 0, 0)
            count[b] += 1
            index += 1
    return {'id': ids, 'mask': masks, 'visit_ms': ms}, table, trans, visits, count


def random_scene(seed, B=3, T=90, A=6):
    """Integer-valued points on a 40 x 30 grid of pixels that the shapes cover in part and overlap on; a jittered clock with gaps,
    a stall and a step backwards; invalid frames, NaN points, fixation ids that change inside and across AOIs."""
    rng = np.random.RandomState(seed)
    rows = [ref.rect(2, 3, 14, 12), ref.ellipse(14, 12, 6, 5), ref.polygon([(20, 2), (36, 2), (36, 20), (30, 20), (30, 8), (26, 8), (26, 20), (20, 20)]),
            ref.disabled(), ref.polygon([(5, 18), (15, 28), (1, 28)]), ref.rect(28, 10, 40, 30)]
    shapes = np.tile(np.stack(rows)[None], (B, 1, 1))
    pog = np.zeros((B, T, 2), np.float32)
    for b in range(B):                                   # a walk that lingers: steps of at most 3 px, a jump now and then
        p = rng.randint(0, 30, 2).astype(np.float64)
        for f in range(T):
            p = rng.randint(0, [40, 30]) if rng.rand() < 0.08 else np.clip(p + rng.randint(-3, 4, 2), 0, [39, 29])
            pog[b, f] = p
    e = shapes[0, 1].astype(np.float64)
    on_rim = (((pog[..., 0] - e[4]) / e[6]) ** 2 + ((pog[..., 1] - e[5]) / e[7]) ** 2 == 1.0) & (pog[..., 0] != e[4]) & (pog[..., 1] != e[5])
    pog[on_rim] = (e[4], e[5])                           # (a rational point exactly on the rim is at the mercy of the roundings)
    dt = rng.uniform(0.010, 0.022, (B, T))
    dt[rng.rand(B, T) < 0.06] = 0.2                      # gaps above max_gap_s
    frame_time = np.cumsum(dt, axis=1) + 100.0 * np.arange(B)[:, None]
    frame_time[0, 40] = frame_time[0, 39]                # a stall
    frame_time[1, 50] = frame_time[1, 49] - 1.0          # a step backwards
    frame_time[2, 10] = np.nan
    valid = (rng.rand(B, T) > 0.08).astype(np.uint8)
    pog[0, 20, 0], pog[1, 21, 1] = np.nan, np.inf
    fixation_id = np.repeat(np.arange(T // 6 + 1), 6)[:T][None].repeat(B, 0).astype(np.int32)
    fixation_id[rng.rand(B, T) < 0.1] = -1
    fixating = (rng.rand(B, T) > 0.3).astype(np.uint8)
    lengths = np.array([T, T - 17, 31], np.int32)[:B]
    return dict(pog=pog, shapes=shapes.astype(np.float32), frame_time=frame_time, valid=valid, fixation_id=fixation_id, fixating=fixating, lengths=lengths)


def run_ref(spec, sc, buffers, cut=None, flush=True, reset=None):
    B = sc['pog'].shape[0]
    c = (lambda a: a) if cut is None else (lambda a: a[:, cut[0]:cut[1]])
    lengths = sc['lengths'] if cut is None else np.clip(sc['lengths'] - cut[0], 0, cut[1] - cut[0]).astype(np.int32)
    return ref.run(spec, c(sc['pog']), sc['shapes'] if sc['shapes'].ndim == 3 else c(sc['shapes']), *buffers, frame_time=c(sc['frame_time']),
                   valid=c(sc['valid']), fixation_id=c(sc['fixation_id']), fixating=c(sc['fixating']), lengths=lengths,
                   flush=np.ones(B, np.int32) if flush else None, reset=reset)


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_the_contract_equals_the_slow_formulation(seed):
    sc = random_scene(seed)
    spec = ref.Spec(max_gap_s=0.075)
    B, A = sc['pog'].shape[0], sc['shapes'].shape[1]
    buffers = ref.fresh(B, A, 128)
    got = run_ref(spec, sc, buffers)
    state, table, trans, visits, count, dropped = buffers
    want, w_table, w_trans, w_visits, w_count = slow_run(spec, sc['pog'], sc['shapes'], A, 128, sc['frame_time'], sc['valid'], sc['fixation_id'],
                                                         sc['fixating'], sc['lengths'])
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
    assert table.tobytes() == w_table.tobytes() and np.array_equal(trans, w_trans)
    assert np.array_equal(count, w_count) and not dropped.any() and visits.tobytes() == w_visits.tobytes()
    assert (count > 5).all() and (table[:, :, 5].sum(axis=1) > 3).all() and not state[:, ref.OPEN].any()
    assert len(set(got['id'].ravel().tolist())) >= 6       # not a sample, outside, and at least four of the five live AOIs
    # the properties: the visits' durations are the dwell (to the sum's own rounding), the transitions' columns are the visits
    for b in range(B):
        rows = visits[b, :count[b]]
        for a in range(A):
            mine = rows[rows[:, 0] == a]
            bound = table[b, a, 1] * 2.0 ** -52 * np.abs(sc['frame_time'][b][np.isfinite(sc['frame_time'][b])]).max()
            assert abs(float(np.sum(mine[:, 2] - mine[:, 1])) - table[b, a, 0]) <= bound
            assert trans[b, :, a].sum() == table[b, a, 2] == len(mine)
            assert mine[:, 3].sum() == table[b, a, 1] and mine[:, 4].sum() == table[b, a, 5]
        assert np.array_equal(rows[:, 5], np.arange(count[b])) and trans[b, A].sum() == 1


@pytest.mark.parametrize('sizes', [[1, 89], [89, 1], [7] * 12 + [6], [64, 26], [33, 57]], ids=['1+rest', 'rest+1', 'sevens', '64+26', '33'])
def test_any_split_into_chunks_equals_one_pass(sizes):
    sc = random_scene(4)
    spec = ref.Spec(max_gap_s=0.075)
    B, A = sc['pog'].shape[0], sc['shapes'].shape[1]
    whole, parts = ref.fresh(B, A, 128), ref.fresh(B, A, 128)
    want = run_ref(spec, sc, whole)
    got, t0 = [], 0
    for i, n in enumerate(sizes):
        got.append(run_ref(spec, sc, parts, cut=(t0, t0 + n), flush=i == len(sizes) - 1))
        t0 += n
    assert t0 == sc['pog'].shape[1]
    for k in KEYS:
        assert np.concatenate([g[k] for g in got], axis=1).tobytes() == want[k].tobytes(), k
    for a, b_ in zip(whole, parts):
        assert a.tobytes() == b_.tobytes()
    # counted time (fps) through the ticks, and per-frame shape tables cut with the frames
    sc = dict(sc, shapes=np.tile(sc['shapes'][:, None], (1, 90, 1, 1)))
    sc['shapes'][:, 45:, 0, 4:8] += 3.0                   # the first rectangle moves at frame 45
    spec = ref.Spec(fps=60.0)
    whole, parts = ref.fresh(B, A, 128), ref.fresh(B, A, 128)
    want = ref.run(spec, sc['pog'], sc['shapes'], *whole, valid=sc['valid'], lengths=sc['lengths'], flush=np.ones(B, np.int32))
    got, t0 = [], 0
    for i, n in enumerate(sizes):
        lengths = np.clip(sc['lengths'] - t0, 0, n).astype(np.int32)
        got.append(ref.run(spec, sc['pog'][:, t0:t0 + n], sc['shapes'][:, t0:t0 + n], *parts, valid=sc['valid'][:, t0:t0 + n], lengths=lengths,
                           flush=np.ones(B, np.int32) if i == len(sizes) - 1 else None))
        t0 += n
    for k in KEYS:
        assert np.concatenate([g[k] for g in got], axis=1).tobytes() == want[k].tobytes(), k
    for a, b_ in zip(whole, parts):
        assert a.tobytes() == b_.tobytes()
    assert whole[0][:, ref.TICKS].tolist() == sc['lengths'].tolist()


def test_point_placement():
    inside = lambda row, x, y: ref.contains(row, np.float64(x), np.float64(y))
    r = ref.rect(10, 20, 30, 40)
    assert inside(r, 10, 20) and inside(r, 29.999, 39.999) and not inside(r, 30, 25) and not inside(r, 15, 40) and not inside(r, 9.999, 25)
    e = ref.ellipse(0, 0, 4, 2)
    assert inside(e, 4, 0) and inside(e, 0, -2) and inside(e, 0, 0) and not inside(e, 4, 0.001) and not inside(e, 3, 1.5)
    assert not inside(ref.ellipse(0, 0, 0, 2), 0, 0) and not inside(ref.ellipse(0, 0, -1, 2), 0, 0)
    # a point at a vertex's y: the (y_i > y) != (y_j > y) rule counts a vertex once, on the upper edge
    tri = ref.polygon([(0, 0), (10, 5), (0, 10)])
    assert inside(tri, 5, 5) and not inside(tri, 10, 5) and not inside(tri, 11, 5) and inside(tri, 0, 5) and not inside(tri, 0, 0) and not inside(tri, 0, 10)
    diamond = ref.polygon([(5, 0), (10, 5), (5, 10), (0, 5)])
    assert inside(diamond, 5, 5) and inside(diamond, 1, 5) and not inside(diamond, -1, 5) and not inside(diamond, 11, 5)
    # a concave notch (a "U"): inside the arms, not in the notch between them
    u = ref.polygon([(0, 0), (9, 0), (9, 9), (6, 9), (6, 3), (3, 3), (3, 9), (0, 9)])
    assert inside(u, 1, 8) and inside(u, 7, 8) and not inside(u, 4.5, 8) and inside(u, 4.5, 1) and not inside(u, 4.5, 3)
    # z-order on overlap, disabled and NaN rows, unknown kinds and vertex counts
    nan_row = ref.rect(0, 0, 100, 100)
    nan_row[6] = np.nan
    bad_n = ref.polygon([(0, 0), (10, 0), (0, 10)])
    bad_n[1] = 2
    frac_n = ref.polygon([(0, 0), (10, 0), (0, 10)])
    frac_n[1] = 3.5
    odd = ref.rect(0, 0, 100, 100)
    odd[0] = 4
    nan_tail = ref.polygon([(0, 0), (10, 0), (0, 10)])
    nan_tail[4 + 6] = np.nan                             # a coordinate the triangle does not use
    rows = [ref.disabled(), nan_row, bad_n, frac_n, odd, ref.rect(0, 0, 10, 10), ref.ellipse(5, 5, 20, 20), nan_tail]
    assert ref.hit_mask(rows, np.float64(2), np.float64(2)) == 0b11100000 and ref.lowest_bit(0b11100000) == 5
    assert ref.hit_mask(rows, np.float64(12), np.float64(2)) == 0b01000000 and ref.hit_mask(rows, np.float64(200), np.float64(2)) == 0
    assert ref.lowest_bit(0) == -1 and ref.lowest_bit(1 << 63) == 63
    # bit 63 is the sign of the int64 output
    spec = ref.Spec(fps=30.0)
    buffers = ref.fresh(1, 64, 4)
    shapes = np.stack([ref.disabled()] * 63 + [ref.rect(0, 0, 10, 10)])[None]
    out = ref.run(spec, np.array([[[2, 2]]], np.float32), shapes, *buffers)
    assert out['id'][0, 0] == 63 and out['mask'][0, 0] == np.iinfo(np.int64).min


# ---------------------------------------------------------------------------------------------------------------- the spec, the shapes
def test_the_spec_compares_by_value_and_refuses_nonsense():
    a, b_ = AoiSpec(num_aois=4, fps=30), AoiSpec('aoi', 4, fps=30.0)
    assert a == b_ and hash(a) == hash(b_) and a != AoiSpec(num_aois=5, fps=30) and a != AoiSpec(num_aois=4, fps=60) and a != 4
    assert a != AoiSpec(num_aois=4, fps=30, source='PoG_px_initial') and a != AoiSpec(num_aois=4, fps=30, use_fixations=False)
    assert a != AoiSpec('other', 4, fps=30) and a != AoiSpec(num_aois=4, fps=30, valid_key='fixating') and a != AoiSpec(num_aois=4, fps=30, max_gap_s=0.1)
    assert len({a, b_, AoiSpec(num_aois=4)}) == 2 and eve_amd.AoiSpec is AoiSpec and 'AoiSpec' in eve_amd.__all__
    assert eval(repr(a)) == a and a.key() == ('aoi', 4, None, None, 30.0, 0.075, None)
    for bad in (None, 0, 65, 2.0, True, '4'):
        with pytest.raises(ValueError, match='num_aois'):
            AoiSpec(num_aois=bad)
    for name in ('fps', 'max_gap_s'):
        for bad in (0, -1.0, float('nan'), float('inf'), '30', True):
            with pytest.raises(ValueError, match=name):
                AoiSpec(num_aois=2, **{name: bad})
    with pytest.raises(ValueError, match='source'):
        AoiSpec(num_aois=2, source='heatmap_final')
    with pytest.raises(ValueError, match='name'):
        AoiSpec('', 2)
    with pytest.raises(ValueError, match='valid_key'):
        AoiSpec(num_aois=2, valid_key=3)
    with pytest.raises(ValueError, match='use_fixations'):
        AoiSpec(num_aois=2, use_fixations=1)
    assert AoiSpec(num_aois=64, source='fixation_px', valid_key='fixating').num_aois == 64


def test_aoi_shapes_builds_the_rows_and_refuses_bad_ones():
    t = data.aoi_shapes([('rect', 1, 2, 3, 4), None, ('ellipse', 5, 6, 7, 8), ('polygon', [(0, 0), (4, 0), (0, 4)])], 6)
    assert t.dtype == torch.float32 and tuple(t.shape) == (6, 36)
    want = np.stack([ref.rect(1, 2, 3, 4), ref.disabled(), ref.ellipse(5, 6, 7, 8), ref.polygon([(0, 0), (4, 0), (0, 4)]), ref.disabled(), ref.disabled()])
    assert np.array_equal(t.numpy(), want)
    g = data.aoi_shapes([('rect', 1, 2, 3, 4), ('ellipse', 5, 6, 7, 8)], 2, margin_px=1.5).numpy()
    assert g[0, 4:8].tolist() == [-0.5, 0.5, 4.5, 5.5] and g[1, 4:8].tolist() == [5, 6, 8.5, 9.5]
    assert not data.aoi_shapes([], 1).any()
    sixteen = [(float(np.cos(i)), float(np.sin(i))) for i in range(16)]
    assert data.aoi_shapes([('polygon', sixteen)], 1)[0, 1] == 16
    for bad, match in (([('rect', 1, 2, 3, 4)] * 3, 'num_aois'), ([('rect', 3, 2, 1, 4)], 'x0 < x1'), ([('rect', 1, 2, 3)], 'four'),
                       ([('ellipse', 0, 0, 0, 1)], 'rx > 0'), ([('ellipse', 0, 0, float('nan'), 1)], 'finite'), ([('circle', 0, 0, 1, 1)], 'rect'),
                       ([('polygon', [(0, 0), (1, 1)])], '3 .. 16'), ([('polygon', sixteen + [(2, 2)])], '3 .. 16'),
                       ([('polygon', [(0, 0), (1, 1), (2, float('inf'))])], 'finite'), ([('rect', 0, 0, 1e39, 1)], 'float32'), (['rect'], 'start with')):
        with pytest.raises(ValueError, match=match):
            data.aoi_shapes(bad, 2)
    with pytest.raises(ValueError, match='margin on a polygon'):
        data.aoi_shapes([('polygon', [(0, 0), (4, 0), (0, 4)])], 1, margin_px=2)
    for bad in (-1, float('nan'), '2'):
        with pytest.raises(ValueError, match='margin_px'):
            data.aoi_shapes([], 1, margin_px=bad)
    with pytest.raises(ValueError, match='num_aois'):
        data.aoi_shapes([], 65)


# ---------------------------------------------------------------------------------------------------------------- EVEStream
class AoiFakes(EventOverlayFakes):
    """The events' and the overlay's stand-ins plus gaze_aoi, evaluated by tests/aoi_ref.py."""

    def gaze_aoi(self, pog, shapes, spec, state, table, trans, visits, count, dropped, frame_time=None, valid=None, valid_key=None,
                 fixation_id=None, fixating=None, lengths=None, reset=None, flush=None):
        self.calls.append('gaze_aoi')
        n = lambda t: None if t is None else t.detach().numpy()
        carried = [n(t) for t in (state, table, trans, visits, count, dropped)]
        if pog is None:
            B, A = state.shape[0], table.shape[1] - 1
            ref.run(spec, np.zeros((B, 0, 2), np.float32), np.zeros((B, A, 36), np.float32), *carried, reset=n(reset), flush=n(flush))
            return {}
        out = ref.run(spec, n(pog), n(shapes), *carried, frame_time=n(frame_time), valid=n(valid), valid_key=n(valid_key),
                      fixation_id=n(fixation_id), fixating=n(fixating), lengths=n(lengths), reset=n(reset), flush=n(flush))
        return {k: torch.from_numpy(v) for k, v in out.items()}


@pytest.fixture()
def fake():
    k = AoiFakes()
    kernels.set_default_kernels(k)
    yield k
    kernels.set_default_kernels(None)
    eve_amd.reset_standalone_config()


B, T, A = 2, 3, 3


@pytest.fixture()
def scene(fake):
    """The model, two chunks, and regions: stream 0 has a rectangle that holds every point (AOI 1) and an ellipse below it in the z-order;
    stream 1 a small box around its first frame's own point of gaze (AOI 1) and one far away, so its later frames are outside."""
    model, _ = make_model(dict(refine_net_rnn_type='CGRU'))
    batch = clip(B, 2 * T, size=32)
    c0, c1 = chunk_of(batch, 0, T), chunk_of(batch, T, 2 * T)
    probe = eve_amd.EVEStream(model, B, use_graph=False)
    p = torch.cat([probe.step(c0)['PoG_px_final'].clone(), probe.step(c1)['PoG_px_final'].clone()], dim=1).numpy().astype(np.float64)
    assert np.isfinite(p).all()
    del fake.calls[:]
    far = p[1, 1] + 1e4
    tables = [data.aoi_shapes([None, ('rect', -1e7, -1e7, 1e7, 1e7), ('ellipse', 0.0, 0.0, 1e7, 1e7)], A),
              data.aoi_shapes([('rect', far[0], far[1], far[0] + 1, far[1] + 1), ('rect', p[1, 0, 0] - 0.25, p[1, 0, 1] - 0.25, p[1, 0, 0] + 0.25,
                                                                                  p[1, 0, 1] + 0.25), None], A)]
    assert np.abs(p[1, 1:] - p[1, 0]).max(axis=1).min() > 0.5          # stream 1 leaves its small box after the first frame
    return model, dict(c0, aoi_shapes=torch.stack(tables)), dict(c1, aoi_shapes=torch.stack(tables))


def run(stream, chunk, **kw):
    return {k: v.clone() for k, v in stream.step(chunk, **kw).items()}


def reference_on(out, chunk, spec, buffers, source='PoG_px_final', **kw):
    n = lambda t: None if t is None else (t.numpy() if torch.is_tensor(t) else t)
    return ref.run(spec, out[source].numpy(), chunk['aoi_shapes'].numpy(), *buffers, **{k: n(v) for k, v in kw.items()})


def test_a_step_with_aoi_adds_three_keys_and_one_launch(fake, scene):
    model, c0, c1 = scene
    plain = run(eve_amd.EVEStream(model, B, use_graph=False), c0)
    assert 'gaze_aoi' not in fake.calls and not [k for k in plain if k.startswith('aoi_')]
    calls_plain = list(fake.calls)
    # ... and the plain step's calls are those of a chunk without the regions: a step without aoi= makes the calls it always made
    del fake.calls[:]
    bare = run(eve_amd.EVEStream(model, B, use_graph=False), {k: v for k, v in c0.items() if k != 'aoi_shapes'})
    assert fake.calls == calls_plain and sorted(bare) == sorted(plain)
    del fake.calls[:]
    s = eve_amd.EVEStream(model, B, use_graph=False, visit_capacity=8)
    spec = AoiSpec(num_aois=A, fps=30)
    out = run(s, c0, aoi=spec)
    assert fake.calls == calls_plain + ['gaze_aoi']                      # the plain step's launches, then one more
    assert sorted(out) == sorted(list(plain) + ['aoi_id', 'aoi_mask', 'aoi_visit_ms'])
    for k in plain:
        assert torch.equal(out[k], plain[k]), k
    for k, dtype in (('aoi_id', torch.int32), ('aoi_mask', torch.int64), ('aoi_visit_ms', torch.float32)):
        assert tuple(out[k].shape) == (B, T) and out[k].dtype == dtype, k
    assert out['aoi_id'].tolist() == [[1, 1, 1], [1, -1, -1]] and out['aoi_mask'].tolist() == [[6, 6, 6], [2, 0, 0]]
    buffers = ref.fresh(B, A, 8)
    want = reference_on(out, c0, spec, buffers)
    for k in KEYS:
        assert out['aoi_' + k].numpy().tobytes() == want[k].tobytes(), k
    out1 = run(s, c1, aoi=spec)
    want1 = reference_on(out1, c1, spec, buffers)
    for k in KEYS:
        assert out1['aoi_' + k].numpy().tobytes() == want1[k].tobytes(), k
    state = s.get_aoi_state()['aoi']
    for got, want_ in zip((state['state'], state['table'], state['transitions'], state['visits'], state['count'], state['dropped']), buffers):
        assert got.numpy().tobytes() == want_.tobytes()
    assert s.aoi_table()[0, 1, :3].tolist() == [5 / 30.0, 6.0, 1.0] and s.aoi_table('aoi')[1, A, 1] == 5
    assert s.aoi_transitions()[:, A].tolist() == [[0, 1, 0], [0, 1, 0]] and s.aoi_visit_counts()[0].tolist() == [0, 1]
    assert [v.shape for v in s.aoi_visits()] == [(0, 8), (1, 8)] and s.aoi_visits([1])[0][0].tolist() == [1, 0, 0, 1, 0, 0, 0, 0]
    # explicit times win over fps; an explicit source; a valid_key of the chunk; moving regions as [B, Tc, A, 36]
    s2 = eve_amd.EVEStream(model, B, use_graph=False)
    ft = torch.tensor([[0.0, 0.011, 0.5], [5.0, 5.01, 5.02]], dtype=torch.float64)
    ok = torch.tensor([[1, 1, 1], [0, 1, 1]], dtype=torch.uint8)
    moving = c0['aoi_shapes'][:, None].repeat(1, T, 1, 1).contiguous()
    moving[0, 1, 1, 0] = 0                               # stream 0, frame 1: AOI 1 is switched off, the ellipse below it shows
    spec2 = AoiSpec('roi', A, source='PoG_px_initial', valid_key='looked', fps=30)
    out2 = run(s2, dict(c0, frame_time=ft, looked=ok, aoi_shapes=moving), aoi=spec2)
    b2 = ref.fresh(B, A, 256)
    want2 = ref.run(spec2, out2['PoG_px_initial'].numpy(), moving.numpy(), *b2, frame_time=ft.numpy(), valid_key=ok.numpy())
    for k in KEYS:
        assert out2['roi_' + k].numpy().tobytes() == want2[k].tobytes(), k
    assert out2['roi_id'][1, 0] == -2 and s2.aoi_table('roi').numpy().tobytes() == b2[1].tobytes() and 'aoi_id' not in out2


def test_aoi_with_events_counts_fixations_and_follows_lengths_and_masks(fake, scene):
    model, c0, c1 = scene
    events = GazeEventSpec(fps=30, saccade_deg_s=1e9, min_fixation_s=0.02)      # each stream: one fixation from its second sample on
    spec = AoiSpec(num_aois=A, fps=30)
    s = eve_amd.EVEStream(model, B, use_graph=False)
    out = run(s, c0, events=events, aoi=spec)
    assert fake.calls[-2:] == ['gaze_events', 'gaze_aoi']
    buffers = ref.fresh(B, A, 256)
    want = reference_on(out, c0, spec, buffers, fixation_id=out['fixation_id'], fixating=out['fixating'])
    for k in KEYS:
        assert out['aoi_' + k].numpy().tobytes() == want[k].tobytes(), k
    assert s.aoi_table().numpy().tobytes() == buffers[1].tobytes() and s.aoi_table()[0, 1, 5] == 1 and s.aoi_table()[0, 1, 6] == 2 / 30.0
    # use_fixations=False keeps them out; the fixation-based analysis reads fixation_px where fixating
    s = eve_amd.EVEStream(model, B, use_graph=False)
    run(s, c0, events=events, aoi=AoiSpec(num_aois=A, fps=30, use_fixations=False))
    assert not s.aoi_table()[:, :, 5].any()
    s = eve_amd.EVEStream(model, B, use_graph=False)
    fspec = AoiSpec(num_aois=A, fps=30, source='fixation_px', valid_key='fixating')
    out = run(s, c0, events=events, aoi=fspec)
    buffers = ref.fresh(B, A, 256)
    want = reference_on(out, c0, fspec, buffers, source='fixation_px', valid_key=out['fixating'], fixation_id=out['fixation_id'], fixating=out['fixating'])
    for k in KEYS:
        assert out['aoi_' + k].numpy().tobytes() == want[k].tobytes(), k
    assert out['aoi_id'][:, :2].tolist() == [[-2, -2]] * B and s.aoi_table().numpy().tobytes() == buffers[1].tobytes()
    # ragged and masked steps
    s = eve_amd.EVEStream(model, B, use_graph=False)
    out = run(s, c0, aoi=spec, lengths=[2, 0])
    buffers = ref.fresh(B, A, 256)
    want = reference_on(out, c0, spec, buffers, lengths=np.array([2, 0]))
    for k in KEYS:
        assert out['aoi_' + k][0, :2].numpy().tobytes() == want[k][0, :2].tobytes(), k
    assert (out['aoi_id'][1] == -2).all() and out['aoi_id'][0, 2] == -2 and s.get_aoi_state()['aoi']['state'][:, 0].tolist() == [2.0, 0.0]
    mask = torch.ones(B, T, 2, dtype=torch.bool)
    mask[0, 1] = False
    s = eve_amd.EVEStream(model, B, use_graph=False)
    out = run(s, c0, aoi=AoiSpec(num_aois=A, fps=30, valid_key='valid'), eye_mask=mask)
    buffers = ref.fresh(B, A, 256)
    want = reference_on(out, c0, spec, buffers, valid=out['valid'])
    for k in KEYS:
        assert out['aoi_' + k].numpy().tobytes() == want[k].tobytes(), k
    assert out['aoi_id'][0].tolist()[1] == -2 and buffers[0][0, ref.TICKS] == T


def test_refusals_come_before_any_launch(fake, scene):
    model, c0, _ = scene
    s = eve_amd.EVEStream(model, B, use_graph=False)
    spec = AoiSpec(num_aois=A, fps=30)
    without = lambda key: {k: v for k, v in c0.items() if k != key}
    with pytest.raises(ValueError, match='AoiSpec'):
        s.step(c0, aoi=dict(num_aois=A))
    with pytest.raises(ValueError, match='aoi_shapes'):
        s.step(without('aoi_shapes'), aoi=spec)
    shapes = c0['aoi_shapes']
    for bad in (shapes.double(), shapes[:, :2].contiguous(), shapes[:, None].repeat(1, T + 1, 1, 1), shapes.numpy(), shapes[..., :35].contiguous(),
                shapes[:1].contiguous()):
        with pytest.raises(ValueError, match='aoi_shapes'):
            s.step(dict(c0, aoi_shapes=bad), aoi=spec)
    with pytest.raises(ValueError, match='aoi_shapes'):
        s.step(c0, aoi=AoiSpec(num_aois=A + 1, fps=30))
    for source in ('PoG_px_filtered', 'fixation_px'):
        with pytest.raises(ValueError, match='events'):
            s.step(c0, aoi=AoiSpec(num_aois=A, fps=30, source=source))
    with pytest.raises(ValueError, match='valid_key'):
        s.step(c0, aoi=AoiSpec(num_aois=A, fps=30, valid_key='fixating'))
    with pytest.raises(ValueError, match='valid_key'):
        s.step(c0, aoi=AoiSpec(num_aois=A, fps=30, valid_key='valid'))      # not a masked step
    with pytest.raises(ValueError, match='valid_key'):
        s.step(dict(c0, looked=torch.zeros(B, T)), aoi=AoiSpec(num_aois=A, fps=30, valid_key='looked'))
    with pytest.raises(ValueError, match='use_fixations'):
        s.step(c0, aoi=AoiSpec(num_aois=A, fps=30, use_fixations=True))
    with pytest.raises(ValueError, match='frame_time'):
        s.step(c0, aoi=AoiSpec(num_aois=A))
    with pytest.raises(ValueError, match='frame_time'):
        s.step(dict(c0, frame_time=torch.zeros(B, T)), aoi=spec)
    with pytest.raises(ValueError, match='inv_camera_transformation'):
        s.step(without('inv_camera_transformation'), aoi=spec)
    with pytest.raises(ValueError, match='name'):
        s.step(dict(c0, aoi_id=torch.zeros(B, T)), aoi=spec)
    with pytest.raises(ValueError, match='name'):
        s.step(c0, aoi=AoiSpec('fixation', A, fps=30))                     # fixation_id is the events' key
    with pytest.raises(ValueError, match='visit_capacity'):
        eve_amd.EVEStream(model, B, use_graph=False, visit_capacity=0)
    with pytest.raises(ValueError, match='no areas of interest'):
        s.aoi_table()
    assert fake.calls == [] and s._aoi == {}
    eye_only, _ = make_model(dict(refine_net_enabled=False))
    s = eve_amd.EVEStream(eye_only, B, use_graph=False)
    with pytest.raises(ValueError, match='RefineNet'):
        s.step(c0, aoi=AoiSpec(num_aois=A, fps=30, source='PoG_px_final'))
    assert fake.calls == []
    out = s.step(without('screen_frame'), aoi=spec)      # source None without a RefineNet: PoG_px_initial
    want = reference_on(out, c0, spec, ref.fresh(B, A, 256), source='PoG_px_initial')
    assert out['aoi_id'].numpy().tobytes() == want['id'].tobytes() and 'PoG_px_final' not in out
    # the tallies are tied to their spec
    with pytest.raises(ValueError, match='another spec'):
        s.step(without('screen_frame'), aoi=AoiSpec(num_aois=A, fps=60))
    s.clear_aoi('aoi')
    s.step(without('screen_frame'), aoi=AoiSpec(num_aois=A, fps=60))
    assert s.get_aoi_state()['aoi']['spec'].fps == 60.0


def test_the_graph_key_holds_the_spec_and_the_shapes(fake, scene):
    model, c0, _ = scene
    s = eve_amd.EVEStream(model, B, use_graph=False)
    plan = lambda spec, ch=c0, events=None: s._check_aoi(ch, spec, events, None, False, B, T)
    bare = s._graph_key(c0, False)
    a = s._graph_key(c0, False, aoi=plan(AoiSpec(num_aois=A, fps=30)))
    assert a != bare and a == s._graph_key(dict(c0), False, aoi=plan(AoiSpec(num_aois=A, fps=30.0)))
    assert a != s._graph_key(c0, False, aoi=plan(AoiSpec(num_aois=A, fps=30, max_gap_s=0.1)))
    assert a != s._graph_key(c0, False, aoi=plan(AoiSpec(num_aois=A, fps=30, source='PoG_px_initial')))
    moving = dict(c0, aoi_shapes=c0['aoi_shapes'][:, None].repeat(1, T, 1, 1))
    assert a != s._graph_key(moving, False, aoi=plan(AoiSpec(num_aois=A, fps=30), moving))
    ev = s._check_events(c0, GazeEventSpec(fps=30), B, T)
    assert s._graph_key(c0, False, events=ev, aoi=plan(AoiSpec(num_aois=A, fps=30), events=ev)) != \
        s._graph_key(c0, False, events=ev, aoi=plan(AoiSpec(num_aois=A, fps=30, use_fixations=False), events=ev))
    captured = []
    s._capture = lambda chunk, *a_, **k_: captured.append((a_, k_)) or {'n': len(captured)}
    first = s._graph_for(c0, False, aoi=plan(AoiSpec(num_aois=A, fps=30)))
    assert s._graph_for(c0, False, aoi=plan(AoiSpec(num_aois=A, fps=30))) is first and len(captured) == 1 and 'aoi' in captured[0][1]
    assert s._graph_for(c0, False) is not first and len(captured) == 2 and len(captured[1][0]) == 4 and captured[1][1] == {}
    # the buffers exist before a capture could run, and _carried() returns them: a capture's warm-up steps are put back
    s._aoi_entry(AoiSpec(num_aois=A, fps=30))
    ids = {id(t) for t in s._carried()}
    assert all(id(t) in ids for t in s._aoi['aoi']['buffers'])


def test_reset_closes_the_visit_and_keeps_the_tallies(fake, scene):
    model, c0, c1 = scene
    spec = AoiSpec(num_aois=A, fps=30)
    s = eve_amd.EVEStream(model, B, use_graph=False, visit_capacity=4)
    run(s, c0, aoi=spec)
    assert s.aoi_visit_counts()[0].tolist() == [0, 1] and s.get_aoi_state()['aoi']['state'][0, ref.OPEN] == 1
    table = s.aoi_table()
    s.reset([0])
    out = run(s, c1, aoi=spec)
    count, dropped = s.aoi_visit_counts()
    assert count.tolist() == [1, 1] and dropped.tolist() == [0, 0]
    assert s.aoi_visits([0])[0][0].tolist() == [1, 0.0, 2 / 30.0, 3, 0, 0, 0, 0]          # closed as it stood
    after = s.get_aoi_state()['aoi']
    assert after['state'][:, ref.TICKS].tolist() == [T, 2 * T] and after['state'][0, ref.NEXT_INDEX] == 2 and after['state'][0, ref.V_INDEX] == 1
    assert out['aoi_visit_ms'][0].tolist() == [0.0, np.float32(1000 / 30.0), np.float32(2000 / 30.0)]
    now = s.aoi_table()
    assert now[0, 1, 2] == 2 and now[0, 1, 1] == 6 and now[0, 1, 0] == table[0, 1, 0] + 2 / 30.0 and now[0, 1, 3] == 0.0      # the tallies ran on
    assert s.aoi_transitions()[0].tolist() == [[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 2, 0]]      # both visits were a first visit since a reset
    # a reset before a step WITHOUT aoi= still ends the visit: one launch with no frames, then the plain step
    s.reset([0])
    del fake.calls[:]
    run(s, c0)
    assert fake.calls.count('gaze_aoi') == 1 and fake.calls[0] == 'gaze_aoi'
    assert s.aoi_visit_counts()[0].tolist() == [2, 1] and not s.get_aoi_state()['aoi']['state'][0, :ref.NEXT_INDEX].any()
    assert torch.equal(s.aoi_table(), now)
    s.flush_aoi_visits([1])
    assert s.aoi_visit_counts()[0].tolist() == [2, 1]    # stream 1 ended outside everything: nothing was open
    s.clear_aoi(streams=[0])
    assert s.aoi_visit_counts()[0].tolist() == [0, 1] and not s.aoi_table()[0].any() and s.aoi_table()[1].any()
    # the state round-trips, and get_state() does not hold it
    saved = s.get_aoi_state()
    s.clear_aoi()
    assert not s.aoi_table().any() and not s.aoi_transitions().any()
    s.set_aoi_state(saved)
    again = s.get_aoi_state()['aoi']
    for k, v in saved['aoi'].items():
        assert (again[k] == v) if k == 'spec' else torch.equal(again[k], v), k
    assert not any('aoi' in k for k in s.get_state())
    with pytest.raises(ValueError, match='spec'):
        s.set_aoi_state({'aoi': {k: v for k, v in saved['aoi'].items() if k != 'spec'}})
    with pytest.raises(ValueError, match='table'):
        s.set_aoi_state({'aoi': dict(saved['aoi'], table=torch.zeros(B, A, 8))})
    fresh = eve_amd.EVEStream(model, B, use_graph=False, visit_capacity=4)
    fresh.set_aoi_state(saved)
    assert torch.equal(fresh.aoi_table(), s.aoi_table())
    # a load that names tallies held under another spec is refused whole: the names before it are not loaded either
    other = AoiSpec('other', A, fps=30)
    two = eve_amd.EVEStream(model, B, use_graph=False, visit_capacity=4)
    two._aoi_entry(AoiSpec(num_aois=A, fps=60))
    mixed = {'other': dict(saved['aoi'], spec=other), 'aoi': saved['aoi']}
    with pytest.raises(ValueError, match='another spec'):
        two.set_aoi_state(mixed)
    assert 'other' not in two._aoi and not two.aoi_table('aoi').any()
