"""GPU: eve_eye_pose_normalize (csrc/eye_pose.hip) against its contract in numpy (tests/eye_pose_ref.py) -- head_R and h within one
float32 ulp (sin / cos / asin / atan2 of identical bits in two libms), o, R, warp and valid bit for bit from the device's own
head_R -- and the pose form (camera_frame + eye_pose) through EVEStream, eager and under graph replay, against the warp form fed
data.normalize_eyes of the same rows."""
import ctypes
import math

import numpy as np
import pytest
import torch

import eve_amd
from eve_amd import data
from eve_amd.kernels import default_kernels
import eye_pose_ref as pref
from test_eye_pose_host import NO_EYES, degenerate_rows
from test_gpu_stream import gpu_clip, make_model

pytestmark = pytest.mark.gpu
GUARD = 64                    # elements behind every output that no launch may touch
SENTINEL, SENTINEL8 = -7.0, 0x5A
HW = (16, 24)                 # (OH, OW) of the kernel cases: the 24 x 16 patch the issue's random poses were checked with
OUTPUTS = (('head_R', 9, 1), ('o', 3, 2), ('R', 9, 2), ('warp', 9, 2), ('h', 2, 2))          # name, floats per row, eyes
CAM = (270, 480)              # (IH, IW) of the end-to-end frames


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def ordered(a):
    """float32 array -> int64 whose difference counts float32 steps (+0 and -0 coincide)."""
    i = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def ulps(a, b):
    return int(np.abs(ordered(a) - ordered(b)).max())


def launch(k, P, hw):
    """One raw launch into sentinel-guarded buffers -> dict of numpy outputs; the guards and the kernel's name checked."""
    N = P.shape[0]
    pose = torch.from_numpy(P).cuda()
    bufs = {name: torch.full((eyes * N * width + GUARD,), SENTINEL, dtype=torch.float32, device='cuda') for name, width, eyes in OUTPUTS}
    valid = torch.full((2 * N + GUARD,), SENTINEL8, dtype=torch.uint8, device='cuda')
    status = k.lib.eve_eye_pose_normalize(N, ptr(pose), hw[0], hw[1], ptr(bufs['head_R']), ptr(bufs['o']), ptr(bufs['R']), ptr(bufs['warp']),
                                          ptr(bufs['h']), ptr(valid), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert status == 0, k.lib.eve_last_error()
    assert k.lib.eve_last_kernel() == b'eye_pose_normalize_kernel'
    out = {}
    for name, width, eyes in OUTPUTS:
        got = bufs[name].cpu().numpy()
        assert (got[eyes * N * width:] == SENTINEL).all(), 'guard of %s overwritten' % name
        shape = ((N,) if eyes == 1 else (2, N)) + ((3, 3) if width == 9 else (width,))
        out[name] = got[:eyes * N * width].reshape(shape)
    got = valid.cpu().numpy()
    assert (got[2 * N:] == SENTINEL8).all(), 'guard of valid overwritten'
    out['valid'] = got[:2 * N].reshape(2, N)
    return out


def check(k, P, hw=HW):
    """Two launches, each compared: head_R within 1 float32 ulp of the contract's; o, R, warp, valid == the contract evaluated from
    the device's head_R; h within 1 ulp of it.  -> (the device's outputs, that contract)"""
    for _ in range(2):
        got = launch(k, P, hw)
        assert ulps(got['head_R'], pref.normalize(P, hw)['head_R']) <= 1
        want = pref.normalize(P, hw, head_R=got['head_R'])
        assert np.array_equal(got['valid'], want['valid']), (got['valid'], want['valid'])
        for name in ('o', 'R', 'warp'):
            g, w = got[name].view(np.uint32), want[name].view(np.uint32)
            assert np.array_equal(g, w), '%s: %d of %d elements differ, first at %s' % (name, int((g != w).sum()), g.size, np.argwhere(g != w)[0])
        assert ulps(got['h'], want['h']) <= 1
    return got, want


# ------------------------------------------------------------------------------------------------ the kernel against its contract
@pytest.mark.parametrize('N', [1, 67])
def test_kernel_equals_the_contract_on_random_poses(N):
    """N = 67: 134 threads, past the first and the second 64-thread block.  The issue's poses: the contract alone keeps every
    corner of a 24 x 16 patch inside the 96 x 128 frame with Wd > 0, so the device's bits are a usable warp."""
    k = default_kernels()
    P = pref.random_poses(N, seed=N)
    got, want = check(k, P)
    assert want['valid'].all() and pref.patch_corners_inside(want, pref.FRAME, HW) == (True, True)
    assert pref.patch_corners_inside(got, pref.FRAME, HW) == (True, True)
    assert not np.array_equal(got['warp'][0], got['warp'][1]) and not np.array_equal(got['o'][0], got['o'][1])       # two eyes, two results
    via = k.eye_pose_normalize(torch.from_numpy(P).cuda(), HW)                       # the tensor-level wrapper
    assert [tuple(t.shape) for t in via] == [(N, 3, 3), (2, N, 3), (2, N, 3, 3), (2, N, 3, 3), (2, N, 2), (2, N)]
    assert via[5].dtype == torch.uint8 and all(t.dtype == torch.float32 for t in via[:5])
    for t, name in zip(via, ('head_R', 'o', 'R', 'warp', 'h', 'valid')):
        assert np.array_equal(t.cpu().numpy(), got[name]), name
    if N == 67:                                                                      # the patch size enters through Kn^-1 only
        big, _ = check(k, P, (128, 128))
        assert np.array_equal(big['R'], got['R']) and not np.array_equal(big['warp'], got['warp'])


def test_degenerate_rows_in_pairs():
    """Every degenerate row of the host test in a launch of N = 2 beside a sound row, in either order: theta = 0, 1e-8 and next to pi,
    a NaN / Inf in each field, o = 0, o_z < 0, one eye behind the camera, zero or negative focal lengths and distances, a head x
    axis next to the line of sight (valid).  The exactly parallel axis has the next test to itself."""
    k = default_kernels()
    sound = pref.random_poses(1, seed=5)[0]
    rows = dict(degenerate_rows())
    rows['head x axis next to forward'] = (pref.pose_row(r=(0, -math.pi / 2, 0), t=(0, 0, 600), eyes=NO_EYES), (1, 1), False)
    for i, (name, (row, valid, ident)) in enumerate(rows.items()):
        first = i % 2
        P = np.stack([row, sound] if first == 0 else [sound, row])
        got, want = check(k, P)
        n = 0 if first == 0 else 1
        assert got['valid'][:, n].tolist() == list(valid) and got['valid'][:, 1 - n].tolist() == [1, 1], name
        assert np.array_equal(got['head_R'][n], np.eye(3, dtype=np.float32)) == ident, name
        for e in range(2):
            if not valid[e]:
                assert not got['warp'][e, n].any() and not got['o'][e, n].any() and not got['h'][e, n].any(), name
                assert np.array_equal(got['R'][e, n], np.eye(3, dtype=np.float32)), name
        assert all(np.isfinite(got[key]).all() for key in ('head_R', 'o', 'R', 'warp', 'h')), name


def test_refused_requests_launch_nothing():
    k = default_kernels()
    k.stream_state_rows(torch.zeros((2, 8), device='cuda'), torch.zeros((2, 8), device='cuda'))     # the last named launch
    before = k.lib.eve_last_kernel()
    assert b'eye_pose' not in before
    pose = torch.from_numpy(pref.random_poses(1, seed=1)).cuda()
    outs = [torch.full((32,), SENTINEL, device='cuda') for _ in range(5)] + [torch.full((32,), SENTINEL8, dtype=torch.uint8, device='cuda')]
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda N, OH, OW, p=ptr(pose), o=None: k.lib.eve_eye_pose_normalize(N, p, OH, OW, *(o or [ptr(t) for t in outs]), s)
    for args, word in (((0, 16, 24), 'bad arguments'), ((1, 0, 24), 'bad arguments'), ((1, 16, 4097), 'patch too large'),
                       ((1, 4097, 24), 'patch too large'), ((1 << 30, 16, 24), '31 bits')):
        assert call(*args) != 0
        msg = k.lib.eve_last_error().decode()
        assert msg.startswith('eye_pose_normalize:') and word in msg and k.lib.eve_last_kernel() == before, msg
    assert call(1, 16, 24, p=None) != 0 and k.lib.eve_last_kernel() == before
    for i in range(6):
        o = [ptr(t) for t in outs]
        o[i] = None
        assert call(1, 16, 24, o=o) != 0 and k.lib.eve_last_kernel() == before, i
    torch.cuda.synchronize()
    assert all((t.cpu() == (SENTINEL8 if t.dtype == torch.uint8 else SENTINEL)).all() for t in outs)
    for bad in (pose.double(), pose[:, :17].contiguous(), pose.view(18), pose.cpu().numpy()):
        with pytest.raises(TypeError, match='pose'):
            k.eye_pose_normalize(bad, HW)
    with pytest.raises(RuntimeError):
        k.eye_pose_normalize(pose.cpu(), HW)
    with pytest.raises(RuntimeError):
        k.eye_pose_normalize(torch.zeros((2, 36), device='cuda')[:, :18], HW)
    assert k.lib.eve_last_kernel() == before
    assert call(1, 16, 24) == 0 and k.lib.eve_last_kernel() == b'eye_pose_normalize_kernel'       # the same call with sound arguments


def test_exactly_parallel_rows_and_the_asin_clamp():
    """A head x axis EXACTLY along forward, from plain float32 rows (tests/eye_pose_ref.py parallel_rows): both cross products are
    zero, the normalisations are 0 / 0, and the kernel must select warp = 0, R = I, o = 0, h = 0 -- bit for bit the contract from the
    device's own head_R, as everywhere.  The rows are built from numpy's head_R; where the device's sits an ulp away the origin is a
    hair off the axis and the row is valid on both sides, so there are several candidates and at least one must be invalid on the
    device.  Likewise clamp_rows: rounding carries m_1 past -1, and at least one row must show it on the device's head_R and
    come out as h = (-pi/2, 0) instead of asin's NaN."""
    k = default_kernels()
    sound = pref.random_poses(1, seed=6)[0]
    rejected = 0
    for row in pref.parallel_rows():
        assert np.isfinite(row).all() and row[9] > 0
        got, want = check(k, np.stack([row, sound]))
        assert got['valid'][:, 1].tolist() == [1, 1] and np.isfinite(got['warp']).all() and np.isfinite(got['R']).all()
        if not got['valid'][:, 0].any():
            rejected += 1
            assert not want['valid'][:, 0].any() and (want['d'][:, 0] > 0).all()
            assert not got['warp'][:, 0].any() and not got['o'][:, 0].any() and not got['h'][:, 0].any()
            assert all(np.array_equal(got['R'][e, 0], np.eye(3, dtype=np.float32)) for e in range(2))
    assert rejected >= 1, 'no candidate was exactly parallel on the device'
    clamped = 0
    for row in pref.clamp_rows():
        got, want = check(k, np.stack([sound, row]))
        assert got['valid'].all() and np.isfinite(got['h']).all()
        if (np.abs(want['m64'][:, 1, 1]) > 1).all():
            clamped += 1
            assert (got['h'][:, 1, 0] == np.float32(-math.pi / 2)).all() and np.abs(got['h'][:, 1, 1]).max() < 1e-6
    assert clamped >= 1, 'no candidate drove m_1 past 1 on the device'


# ------------------------------------------------------------------------------------------------ EVEStream
def cam_poses(B, T, seed, invalid=()):
    """Poses whose 128 x 128 patches look into CAM-sized frames (f = 430, the head 500..700 mm away) -> float32 [B, T, 18]."""
    g = np.random.default_rng(seed)
    rows = [pref.pose_row(K=(430.0 + g.uniform(-10, 10), 430.0 + g.uniform(-10, 10), CAM[1] / 2 + g.uniform(-5, 5), CAM[0] / 2 + g.uniform(-5, 5)),
                          r=g.uniform(-0.3, 0.3, 3), t=(g.uniform(-40, 40), g.uniform(0, 40), g.uniform(500, 700)), focal_norm=600.0)
            for _ in range(B * T)]
    P = np.stack(rows)
    res = pref.normalize(P, (128, 128))
    assert res['valid'].all() and pref.patch_corners_inside(res, CAM, (128, 128)) == (True, True)
    P = torch.from_numpy(P).view(B, T, 18).clone()
    for b, t in invalid:
        P[b, t, 5] = float('nan')
    return P


def cam_lens(B, T):
    """One mild barrel camera for every frame, the intrinsics of cam_poses' nominal camera -> float32 [B, T, 12]."""
    row = torch.tensor([430.0, 430.0, CAM[1] / 2, CAM[0] / 2, -0.25, 0.08, 1e-3, -5e-4, -0.01, 0, 0, 0])
    return row.expand(B, T, 12).contiguous()


def test_stream_replays_a_graph_over_pose_rows():
    """B = 2, Tc = 2, refine_net config, a 6-frame clip in three chunks, the third ragged.  The pose form under graph replay equals
    the eager pose form and the warp form (a graph stream of its own, fed data.normalize_eyes of the same rows) bit for bit in
    every prediction key; the second step REPLAYS the first one's graph with other pose rows and gives the second chunk's result,
    not the first rows' (the launch sits inside the graph and reads the graph's input buffer); frame (0, 1) of the first chunk has
    a NaN pose: pose_valid False for both eyes, a black patch, finite outputs; one more chunk carries camera_lens."""
    model, _ = make_model()
    _, d, _ = gpu_clip(2, 6, seed=5)
    rest = {k_: v for k_, v in d.items() if k_ not in ('left_eye_patch', 'right_eye_patch', 'left_h', 'right_h', 'left_o', 'right_o',
                                                      'left_R', 'right_R', 'head_R')}
    g0 = torch.Generator().manual_seed(6)
    frames = torch.randint(0, 256, (2, 6) + CAM + (3,), generator=g0, dtype=torch.uint8).cuda()
    P = cam_poses(2, 6, seed=7, invalid=[(0, 1)]).cuda()
    pose = dict(rest, camera_frame=frames, eye_pose=P)
    ch = lambda src, i: {k_: v[:, 2 * i:2 * i + 2].contiguous() for k_, v in src.items()}

    def warp_form(chunk):
        derived = data.normalize_eyes(chunk['eye_pose'])
        valid = derived.pop('pose_valid')
        return dict({k_: v for k_, v in chunk.items() if k_ != 'eye_pose'}, **derived), valid

    g, e, w = eve_amd.EVEStream(model, 2), eve_amd.EVEStream(model, 2, use_graph=False), eve_amd.EVEStream(model, 2)
    outs = []
    for i, lengths in enumerate((None, None, [1, 2])):
        og = {k_: v.clone() for k_, v in g.step(ch(pose, i), return_heatmaps=True, lengths=lengths).items()}
        oe = e.step(ch(pose, i), return_heatmaps=True, lengths=lengths)
        wf, valid = warp_form(ch(pose, i))
        ow = w.step(wf, return_heatmaps=True, lengths=lengths)
        assert set(og) == set(oe) == set(ow) | {'pose_valid'} and 'heatmap_final' in og and 'PoG_px_final' in og
        assert og['pose_valid'].dtype == torch.bool and torch.equal(og['pose_valid'], valid) and torch.equal(oe['pose_valid'], valid)
        for k_ in ow:
            assert torch.equal(og[k_], oe[k_]), (i, k_)
            assert torch.equal(og[k_], ow[k_]), (i, k_)
            assert torch.isfinite(og[k_].float()).all(), (i, k_)
        outs.append(og)
    assert len(g._graphs) == 2 and len(w._graphs) == 2                # one uniform graph replayed twice, one ragged
    assert outs[0]['pose_valid'].tolist() == [[[True, True], [False, False]], [[True, True], [True, True]]]
    assert outs[1]['pose_valid'].all() and outs[2]['pose_valid'].all()
    # the invalid frame: a zero warp, so a black patch
    wf, _ = warp_form(ch(pose, 0))
    assert not wf['left_eye_warp'][0, 1].any() and not wf['right_eye_warp'][0, 1].any()
    black = data.warp_eye_patches(wf['camera_frame'], wf['left_eye_warp'])
    assert (black[0, 1] == -1.0).all() and not (black[0, 0] == -1.0).all()
    # the second chunk's frames under the FIRST chunk's pose rows give another result: the replay read the rows of the chunk at hand
    e2 = eve_amd.EVEStream(model, 2, use_graph=False)
    e2.step(ch(pose, 0))
    other = e2.step(dict(ch(pose, 1), eye_pose=ch(pose, 0)['eye_pose']))
    assert not torch.equal(other['g_initial'], outs[1]['g_initial'])
    # raw frames: camera_lens beside the pose rows, graph against the eager warp form
    g.reset()
    lens = cam_lens(2, 2).cuda()
    ol = {k_: v.clone() for k_, v in g.step(dict(ch(pose, 1), camera_lens=lens)).items()}
    assert len(g._graphs) == 3
    e3 = eve_amd.EVEStream(model, 2, use_graph=False)
    wf, valid = warp_form(ch(pose, 1))
    ow = e3.step(dict(wf, camera_lens=lens))
    for k_ in ow:
        assert torch.equal(ol[k_], ow[k_]), k_
    assert torch.equal(ol['pose_valid'], valid)
    g.reset()
    plain = g.step(ch(pose, 1))
    assert not torch.equal(plain['g_initial'], ol['g_initial'])
