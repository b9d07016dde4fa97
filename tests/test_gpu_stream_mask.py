"""GPU: masked EVEStream steps (step(chunk, eye_mask=..., skip_invalid_pose=...)) -- the two HIP entry points behind them
(eve_stream_mask_plan, eve_stream_permute_rows) bit for bit against their restatements, and the contract on the HIP kernels:
every eye sequence consumes exactly its usable frames, nothing a masked-out eye supplied reaches a valid output, one captured
graph per chunk shape serves every mask pattern."""
import ctypes

import numpy as np
import pytest
import torch

import eve_amd
from eve_amd.kernels import default_kernels
from test_gpu_eye_pose import CAM, cam_poses
from test_gpu_stream import gpu_clip, maxdiff
from test_gpu_stream_ragged import clone, make_model, padded
from test_stream_mask_host import (B_CLIP, MASK, T_CLIP, TC, junk_unusable, masked_reference, numpy_plan, run_masked, step_masks,
                                   where_defined)
from test_stream_ragged_host import CONFIGS, flat_state

pytestmark = pytest.mark.gpu
GUARD = 64                    # elements behind every output that no launch may touch
ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
cur_stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def guarded(n, dtype, fill):
    """-> (the whole buffer, its first n elements): GUARD elements of `fill` behind them."""
    whole = torch.full((n + GUARD,), fill, dtype=dtype).cuda()
    return whole, whole[:n]


# ------------------------------------------------------------------------------------------------ 1. the plan kernel
def plan_cases():
    g = np.random.default_rng(5)
    rnd = lambda B, T, p=0.6: (g.random((B, T, 2)) < p)
    long_mask = rnd(2, 70)
    long_mask[0, 60:68, 0] = [1, 0, 0, 1, 1, 0, 1, 1]                 # usable and unusable frames on both sides of frame 64
    return {
        'B3-T5': (3, 5, rnd(3, 5), None, None),
        'T1': (4, 1, rnd(4, 1, 0.5), None, None),
        'B2-T70': (2, 70, long_mask, None, None),
        'all-usable': (3, 5, np.ones((3, 5, 2), dtype=bool), None, None),
        'none-usable': (3, 5, np.zeros((3, 5, 2), dtype=bool), None, None),
        'mask-null': (3, 5, None, None, None),
        'mask-null-lengths': (3, 5, None, None, [2, 0, 5, 2, 0, 5]),
        'wild-lengths': (3, 5, rnd(3, 5, 0.8), None, [7, -3, 1 << 30, 7, -3, 1 << 30]),
        'pose-valid': (3, 5, rnd(3, 5, 0.8), rnd(3, 5, 0.7), [5, 4, 2, 5, 4, 2]),
        'pose-valid-only': (2, 6, None, rnd(2, 6, 0.5), None),
        'uint8-values': (2, 4, g.integers(0, 3, (2, 4, 2)) * 127, None, None),    # any non-zero byte is usable
    }


@pytest.mark.parametrize('name', sorted(plan_cases()))
def test_mask_plan_is_bit_exact(name):
    """eve_stream_mask_plan against numpy_plan: count, perm, inv, eye_valid and valid bit for bit; perm is a permutation with the
    usable frames first and ascending, inv its inverse; the guard behind every output is untouched; twice gives the same bytes."""
    B, T, mask, pose, lengths = plan_cases()[name]
    k = default_kernels()
    dev = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dt))).cuda()
    m, p, n = dev(mask, np.uint8), dev(pose, np.uint8), dev(lengths, np.int32)
    S = 3 * B
    outs = [guarded(S, torch.int32, -77), guarded(S * T, torch.int32, -77), guarded(S * T, torch.int32, -77),
            guarded(B * T * 2, torch.uint8, 0x5A), guarded(B * T, torch.uint8, 0x5A)]
    want = numpy_plan(B, T, mask, pose, lengths)
    first = None
    for _ in range(2):
        assert k.lib.eve_stream_mask_plan(B, T, ptr(m), ptr(p), ptr(n), *[ptr(o[1]) for o in outs], cur_stream()) == 0
        got = [o[0].cpu().numpy() for o in outs]
        first = got if first is None else first
        for a, b, w in zip(got, first, want):
            assert np.array_equal(a, b)
            assert np.array_equal(a[:w.size], w.reshape(-1)), name
            assert (a[w.size:] == (0x5A if a.dtype == np.uint8 else -77)).all(), name
    assert b'stream_mask_plan_kernel' in k.lib.eve_last_kernel()
    count, perm, inv = got[0][:S], got[1][:S * T].reshape(S, T), got[2][:S * T].reshape(S, T)
    for s in range(S):
        assert sorted(perm[s].tolist()) == list(range(T)), s
        assert np.array_equal(inv[s][perm[s]], np.arange(T)), s
        head, tail = perm[s][:count[s]], perm[s][count[s]:]
        assert np.array_equal(head, np.sort(head)) and np.array_equal(tail, np.sort(tail)), s
    # the wrapper returns the same plan
    plan = k.stream_mask_plan(B, T, None if m is None else m.view(B, T, 2), None if p is None else p.view(B, T, 2) != 0, n,
                              device=torch.device('cuda'))
    for key, w in zip(('count', 'perm', 'inv', 'eye_valid', 'valid'), want):
        assert np.array_equal(plan[key].cpu().numpy(), w), (name, key)


def test_mask_plan_refuses_without_launching():
    k = default_kernels()
    B, T = 2, 3
    bufs = [torch.zeros(n, dtype=dt).cuda() for n, dt in ((3 * B, torch.int32), (3 * B * T, torch.int32), (3 * B * T, torch.int32),
                                                        (2 * B * T, torch.uint8), (B * T, torch.uint8))]
    k.stream_state_rows(torch.zeros((2, 8), device='cuda'), torch.zeros((2, 8), device='cuda'))     # the last named launch
    cases = {'T = 0': (B, 0, bufs), 'B = 0': (0, T, bufs), 'T too large': (1 << 20, 1 << 20, bufs)}
    for i in range(5):
        cases['output %d NULL' % i] = (B, T, bufs[:i] + [None] + bufs[i + 1:])
    for name, (B_, T_, o) in cases.items():
        assert k.lib.eve_stream_mask_plan(B_, T_, None, None, None, *[ptr(t) for t in o], cur_stream()) != 0, name
        assert k.lib.eve_last_error().decode().startswith('stream_mask_plan:'), name
        assert b'stream_state_rows_kernel' in k.lib.eve_last_kernel(), name


# ------------------------------------------------------------------------------------------------ 2. the row gather
S_ROWS, T_ROWS = 5, 4
INDEX = [[2, 0, 3, 1], [3, 2, 1, 0], [0, 1, 2, 3], [1, 1, 1, 1], [1, 3, 0, 2]]              # one row repeats: any index works


def gather(src, index, offset_bytes=0):
    """eve_stream_permute_rows on a [S, T, row] view through the C entry with a guarded, optionally misaligned destination;
    checks the guard and a second launch; -> dst [S, T, row]."""
    k = default_kernels()
    S, T, row = src.shape
    es = src.element_size()
    off = offset_bytes // es
    whole = torch.full((off + S * T * row + GUARD,), -7, dtype=src.dtype).cuda()
    dst = whole[off:off + S * T * row]
    for _ in range(2):
        assert k.lib.eve_stream_permute_rows(S, T, row * es, src.stride(1) * es, src.stride(0) * es, ptr(src), ptr(dst), ptr(index),
                                             cur_stream()) == 0, k.lib.eve_last_error()
        assert (whole[:off] == -7).all() and (whole[off + S * T * row:] == -7).all()
    assert b'stream_permute_rows_kernel' in k.lib.eve_last_kernel()
    return dst.view(S, T, row)


def expect(src, index):
    idx = index.long().clamp(0, src.shape[1] - 1)
    return torch.stack([src[s][idx[s]] for s in range(src.shape[0])], dim=0)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_permute_rows_is_bit_exact(dtype):
    """dst[s][j] = src[s][index[s][j]], S = 5, T = 4: rows of 4 bytes (pupil), 8 bytes (gaze, head pose), 2048 bytes (feats) and
    the bottleneck's 40 * C elements for C = 32, 64, 128; 130-element rows inside wider ones (frame stride 160, sequence stride
    4 * 160 + 32); a base 4 bytes off a 16-byte boundary (the dword path) on both sides; indices outside 0..T-1 clamped; the
    wrapper on a strided column."""
    k = default_kernels()
    g = torch.Generator().manual_seed(3)
    index = torch.tensor(INDEX, dtype=torch.int32).cuda()
    es = torch.empty((), dtype=dtype).element_size()
    for row_bytes in (4, 8, 2048):
        src = torch.randn((S_ROWS, T_ROWS, row_bytes // es), generator=g).to(dtype).cuda()
        assert torch.equal(gather(src, index), expect(src, index)), row_bytes
    for C in (32, 64, 128):
        src = torch.randn((S_ROWS, T_ROWS, 40 * C), generator=g).to(dtype).cuda()
        assert torch.equal(gather(src, index), expect(src, index)), C
        assert torch.equal(gather(src, index, offset_bytes=4), expect(src, index)), C          # dst off the 16-byte grid
        assert torch.equal(k.stream_permute_rows(src.view(S_ROWS, T_ROWS, 5, 8, C), index).view(S_ROWS, T_ROWS, -1), expect(src, index))
    fstride, sstride = 160, 4 * 160 + 32
    flat = torch.randn((S_ROWS * sstride,), generator=g).to(dtype).cuda()
    src = flat.as_strided((S_ROWS, T_ROWS, 130), (sstride, fstride, 1))
    assert torch.equal(gather(src, index), expect(src, index))
    off = 4 // es                                                                            # src off the 16-byte grid
    flat = torch.randn((off + S_ROWS * T_ROWS * 256,), generator=g).to(dtype).cuda()
    src = flat[off:].view(S_ROWS, T_ROWS, 256)
    assert torch.equal(gather(src, index), expect(src, index))
    wild = torch.tensor([[7, -3, 1 << 30, 0], [-(1 << 31), 2, 4, -1], [0, 1, 2, 3], [3, 3, 3, 3], [100, -100, 1, 2]], dtype=torch.int32).cuda()
    src = torch.randn((S_ROWS, T_ROWS, 130), generator=g).to(dtype).cuda()
    assert torch.equal(gather(src, wild), expect(src, wild))
    if dtype == torch.float32:                                                                # the pupil column of a [N, 4] layer output
        wide = torch.randn((S_ROWS * T_ROWS, 4), generator=g).cuda()
        col = wide[:, 0].view(S_ROWS, T_ROWS)
        assert torch.equal(k.stream_permute_rows(col, index), expect(col[..., None], index)[..., 0])


def test_permute_rows_refuses_without_launching():
    k = default_kernels()
    S, T, row = S_ROWS, T_ROWS, 520
    src = torch.randn((S, T, row // 4)).cuda()
    dst = torch.full((S, T, row // 4), -7.0).cuda()
    index = torch.tensor(INDEX, dtype=torch.int32).cuda()
    k.stream_state_rows(torch.zeros((2, 8), device='cuda'), torch.zeros((2, 8), device='cuda'))     # the last named launch
    call = lambda S_, T_, rb, fs, ss, a, b, i: k.lib.eve_stream_permute_rows(S_, T_, rb, fs, ss, a, b, i, cur_stream())
    whole = torch.randn((2 * S * T * row // 4,)).cuda()
    inside = ctypes.c_void_p(whole.data_ptr() + S * T * row - row)                                 # dst begins inside src's span
    cases = {'src NULL': (S, T, row, row, T * row, None, ptr(dst), ptr(index)),
             'dst NULL': (S, T, row, row, T * row, ptr(src), None, ptr(index)),
             'index NULL': (S, T, row, row, T * row, ptr(src), ptr(dst), None),
             'T = 0': (S, 0, row, row, T * row, ptr(src), ptr(dst), ptr(index)),
             'T < 0': (S, -1, row, row, T * row, ptr(src), ptr(dst), ptr(index)),
             'S = 0': (0, T, row, row, T * row, ptr(src), ptr(dst), ptr(index)),
             'row_bytes % 4': (S, T, 518, 520, T * 520, ptr(src), ptr(dst), ptr(index)),
             'row_bytes = 0': (S, T, 0, row, T * row, ptr(src), ptr(dst), ptr(index)),
             'stride < row': (S, T, row, row - 4, T * row, ptr(src), ptr(dst), ptr(index)),
             'in place': (S, T, row, row, T * row, ptr(src), ptr(src), ptr(index)),
             'overlap': (S, T, row, row, T * row, ptr(whole), inside, ptr(index))}
    for name, args in cases.items():
        assert call(*args) != 0, name
        msg = k.lib.eve_last_error().decode()
        assert msg.startswith('stream_permute_rows:'), (name, msg)
        assert b'stream_state_rows_kernel' in k.lib.eve_last_kernel(), name
    assert 'overlap' in k.lib.eve_last_error().decode()
    torch.cuda.synchronize()
    assert (dst == -7.0).all()
    assert call(S, T, row, row, T * row, ptr(src), ptr(dst), ptr(index)) == 0                       # sound arguments are taken
    assert torch.equal(dst, expect(src, index))


# ------------------------------------------------------------------------------------------------ 3. end to end
def stream_run(model, d, **kw):
    return run_masked(eve_amd.EVEStream(model, B_CLIP, use_graph=kw.pop('use_graph', True)), d, pad=padded, **kw)


@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_masked_stream_float32_matches_the_reference(name):
    """B = 3, T = 10 in steps of 4 under MASK (hipGraph; the partial last step padded with junk and cut by lengths) against
    masked_reference on the same kernels, under the bounds of test_ragged_split_float32_matches_the_whole_clip: 1e-5 rad / 1e-2
    px / 1e-3 cm, five times that on the refined keys; EyeNet's states within 1e-5, RefineNet's within 5e-5 -- that test's bounds
    for states computed by the same tail arithmetic on both sides.  The reference runs the layer-by-layer tail, so with
    stream_fused_tail RefineNet's states are printed and not bounded: the fused tail's own distance from the layer-by-layer one
    (1-2e-6 rad on the initial gaze, test_gpu_stream.py) reaches them through the heat-map of that gaze (3.0e-4 measured), which
    no like-for-like bound covers; that configuration's states are held by the bit-exact tests below."""
    over, fused = CONFIGS[name]
    model, _ = make_model(**over)
    model.eye_net.stream_fused_tail = fused
    _, d, _ = gpu_clip(B_CLIP, T_CLIP, seed=9)
    want, want_state = masked_reference(model, d, MASK.cuda())
    got, state = stream_run(model, d)
    assert torch.equal(got.pop('eye_valid').cpu(), MASK) and torch.equal(got.pop('valid').cpu(), MASK.any(-1))
    assert set(got) == set(want)
    report = {}
    for k_, v in got.items():
        at = where_defined(k_).cuda()
        assert torch.isfinite(v[at]).all(), k_
        report[k_] = maxdiff(v[at], want[k_][at])
    print('masked vs reference (%s): %s' % (name, ', '.join('%s %.1e' % kv for kv in sorted(report.items()))))
    for k_, e in report.items():
        amp = 5.0 if k_.endswith('_final') else 1.0
        assert e <= amp * (1e-2 if 'px' in k_ else (1e-3 if 'cm' in k_ else 1e-5)), (k_, e)
    for (k_, i, a), (k2, _, b) in zip(flat_state(state), flat_state(want_state)):
        e = maxdiff(a, b)
        print('state %s[%d]: masked vs reference %.1e' % (k_, i, e))
        assert k_ == k2 and (e <= (5e-5 if k_.startswith('refinenet') else 1e-5) or (fused and k_.startswith('refinenet'))), (k_, i, e)


@pytest.mark.parametrize('name', ['gru-cgru', 'cgru-x2-w32'])
def test_masked_stream_bf16_matches_the_reference(name):
    """The same in bf16 under test_ragged_split_half_precision_matches_the_same_dtype_whole_clip's bound: the masked stream's
    deviation from the bf16 reference stays inside that reference's own distance to the float32 one (the frame-by-frame
    reference folds fewer frames into a launch, which selects other tiles and so other 16-bit roundings), outputs and states."""
    over, fused = CONFIGS[name]
    model, _ = make_model(dtype=torch.bfloat16, **over)
    m32, _ = make_model(**over)
    _, d, _ = gpu_clip(B_CLIP, T_CLIP, seed=9)
    (want, want_state), (w32, state32) = masked_reference(model, d, MASK.cuda()), masked_reference(m32, d, MASK.cuda())
    got, state = stream_run(model, d)
    for k_ in ('g_initial', 'g_final', 'PoG_px_initial', 'PoG_px_final'):
        at = where_defined(k_).cuda()
        noise, dev = maxdiff(want[k_][at], w32[k_][at]), maxdiff(got[k_][at], want[k_][at])
        print('bf16 %s %s: masked vs reference %.2e, dtype noise %.2e' % (name, k_, dev, noise))
        assert dev <= noise + (1e-2 if 'px' in k_ else 1e-5), (k_, dev, noise)
    for (k_, i, a), (_, _, b), (_, _, c) in zip(flat_state(state), flat_state(want_state), flat_state(state32)):
        e, noise = maxdiff(a, b), maxdiff(b, c)
        print('bf16 %s state %s[%d]: masked vs reference %.2e, dtype noise %.2e' % (name, k_, i, e, noise))
        assert e <= noise + 1e-5, (k_, i, e, noise)


@pytest.mark.parametrize('name,dtype', [(n, torch.float32) for n in sorted(CONFIGS)] + [('gru-cgru', torch.bfloat16), ('cgru-x2-w32', torch.bfloat16)],
                         ids=lambda v: v if isinstance(v, str) else str(v).split('.')[-1])
def test_masked_out_inputs_reach_no_valid_output(name, dtype):
    """Every masked-out eye's patch, h, o and R and every input of a frame without a usable eye replaced by random finite values:
    the valid outputs and the carried states do not change by a bit."""
    over, fused = CONFIGS[name]
    model, _ = make_model(dtype=dtype, **over)
    model.eye_net.stream_fused_tail = fused
    _, d, _ = gpu_clip(B_CLIP, T_CLIP, seed=9)
    clean, clean_state = stream_run(model, d)
    dirty, dirty_state = stream_run(model, d, junk=junk_unusable)
    for k_, v in clean.items():
        at = where_defined(k_).cuda() if k_ not in ('valid', 'eye_valid') else torch.ones(MASK.shape[:2], dtype=torch.bool).cuda()
        assert torch.equal(v[at], dirty[k_][at]), k_
        assert torch.isfinite(v[at].float()).all(), k_
    for (k_, i, a), (_, _, b) in zip(flat_state(clean_state), flat_state(dirty_state)):
        assert torch.equal(a, b), (k_, i)


@pytest.mark.parametrize('name,dtype', [(n, torch.float32) for n in sorted(CONFIGS)] + [('gru-cgru', torch.bfloat16), ('cgru-x2-w32', torch.bfloat16)],
                         ids=lambda v: v if isinstance(v, str) else str(v).split('.')[-1])
def test_all_ones_mask_gives_the_unmasked_bits(name, dtype):
    over, fused = CONFIGS[name]
    model, _ = make_model(dtype=dtype, **over)
    model.eye_net.stream_fused_tail = fused
    _, d, _ = gpu_clip(B_CLIP, 2 * TC, seed=9)
    a, b = eve_amd.EVEStream(model, B_CLIP), eve_amd.EVEStream(model, B_CLIP)
    ones = torch.ones((B_CLIP, TC, 2), dtype=torch.bool).cuda()
    for t0 in (0, TC):
        ch = {k_: v[:, t0:t0 + TC].contiguous() for k_, v in d.items()}
        plain, masked = a.step(ch), b.step(ch, eye_mask=ones)
        assert masked.pop('valid').all() and masked.pop('eye_valid').all()
        for k_ in plain:
            assert torch.equal(plain[k_], masked[k_]), (t0, k_)
    for (k_, i, x), (_, _, y) in zip(flat_state(a.get_state()), flat_state(b.get_state())):
        assert torch.equal(x, y), (k_, i)


# ------------------------------------------------------------------------------------------------ 4. one graph per shape
def test_one_masked_graph_serves_every_mask_pattern():
    """Three mask patterns of one chunk shape (three 4-frame windows of MASK), handed over as nested lists, a numpy array and a
    device tensor: one captured graph, outputs and states bit-identical to use_graph=False; a device-resident mask and a host list give the
    same bits."""
    model, _ = make_model(refine_net_rnn_type='CGRU')
    _, d, _ = gpu_clip(B_CLIP, 3 * TC, seed=7)
    ch = lambda i: {k_: v[:, TC * i:TC * i + TC].contiguous() for k_, v in d.items()}
    patterns = [MASK[:, 0:4], MASK[:, 4:8], MASK[:, 6:10]]
    g, e, dev = eve_amd.EVEStream(model, B_CLIP), eve_amd.EVEStream(model, B_CLIP, use_graph=False), eve_amd.EVEStream(model, B_CLIP)
    for i, m in enumerate(patterns):
        og, oe, od = g.step(ch(i), eye_mask=m.tolist()), e.step(ch(i), eye_mask=m.numpy()), dev.step(ch(i), eye_mask=m.cuda())
        assert set(og) == set(oe) == set(od) and torch.equal(og['eye_valid'].cpu(), m)
        for k_ in og:
            assert torch.equal(og[k_], oe[k_]) and torch.equal(og[k_], od[k_]), (i, k_)
        for (k_, j, x), (_, _, y), (_, _, z) in zip(flat_state(g.get_state()), flat_state(e.get_state()), flat_state(dev.get_state())):
            assert torch.equal(x, y) and torch.equal(x, z), (i, k_, j)
    assert len(g._graphs) == 1 and len(dev._graphs) == 1 and [key[2] for key in g._graphs] == [True]
    # a uint8 device mask, and the unmasked graph next to the masked one
    m8 = (patterns[1].to(torch.uint8) * 200).cuda()
    og, oe = g.step(ch(0), eye_mask=m8), e.step(ch(0), eye_mask=patterns[1])
    for k_ in og:
        assert torch.equal(og[k_], oe[k_]), k_
    assert 'valid' not in g.step(ch(1)) and sorted(key[2] for key in g._graphs) == [False, True]


# ------------------------------------------------------------------------------------------------ 5. the pose form
def test_skip_invalid_pose_folds_pose_valid_into_the_mask():
    """B = 2, Tc = 3, camera_frame + eye_pose; frame (0, 1) holds a NaN, frame (1, 2) has the head behind the camera.  With
    skip_invalid_pose=True eye_valid == pose_valid and the carried states are those of the same step under the explicit mask
    pose_valid; without the flag -- plain, or masked with an all-ones mask through the same captured graph -- the outputs are the
    unmasked step's bits and pose_valid is folded into nothing."""
    model, _ = make_model()
    _, d, _ = gpu_clip(2, 3, seed=5)
    rest = {k_: v for k_, v in d.items() if k_ not in ('left_eye_patch', 'right_eye_patch', 'left_h', 'right_h', 'left_o', 'right_o',
                                                      'left_R', 'right_R', 'head_R')}
    frames = torch.randint(0, 256, (2, 3) + CAM + (3,), generator=torch.Generator().manual_seed(6), dtype=torch.uint8).cuda()
    P = cam_poses(2, 3, seed=7, invalid=[(0, 1)])
    P[1, 2, 9] = -P[1, 2, 9]                                          # tvec z < 0: the head behind the camera
    chunk = dict(rest, camera_frame=frames, eye_pose=P.cuda())
    want_valid = torch.tensor([[[True] * 2, [False] * 2, [True] * 2], [[True] * 2, [True] * 2, [False] * 2]]).cuda()
    plain_stream, g, explicit = eve_amd.EVEStream(model, 2), eve_amd.EVEStream(model, 2), eve_amd.EVEStream(model, 2)
    plain = clone(plain_stream.step(chunk))
    assert 'valid' not in plain and torch.equal(plain['pose_valid'], want_valid)
    start = g.get_state()
    skipped = clone(g.step(chunk, skip_invalid_pose=True))
    assert torch.equal(skipped['eye_valid'], want_valid) and torch.equal(skipped['pose_valid'], want_valid)
    assert torch.equal(skipped['valid'], want_valid.any(-1))
    same = clone(explicit.step(chunk, eye_mask=want_valid))
    for k_ in same:
        at = torch.ones((2, 3), dtype=torch.bool).cuda() if k_ in ('valid', 'eye_valid', 'pose_valid') else want_valid.any(-1)
        assert torch.equal(skipped[k_][at], same[k_][at]), k_
    for (k_, j, x), (_, _, y), (_, _, z) in zip(flat_state(g.get_state()), flat_state(explicit.get_state()), flat_state(plain_stream.get_state())):
        assert torch.equal(x, y), (k_, j)
        assert not torch.equal(x, z), (k_, j)                         # the black patches of the plain step did move the states
    # the same masked graph without the flag: pose_valid stays out of the mask, the bits are the unmasked step's
    g.set_state(start)
    ones = clone(g.step(chunk, eye_mask=torch.ones((2, 3, 2), dtype=torch.bool).cuda()))
    assert len(g._graphs) == 1 and ones.pop('eye_valid').all() and ones.pop('valid').all()
    for k_ in plain:
        assert torch.equal(ones[k_], plain[k_]), k_
    for (k_, j, x), (_, _, z) in zip(flat_state(g.get_state()), flat_state(plain_stream.get_state())):
        assert torch.equal(x, z), (k_, j)
    with pytest.raises(ValueError):
        g.step({k_: v for k_, v in d.items()}, skip_invalid_pose=True)
