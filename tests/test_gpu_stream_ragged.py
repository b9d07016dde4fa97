"""GPU: ragged EVEStream steps (step(chunk, lengths=...)) -- the two HIP entry points behind them (eve_stream_state_rows_at,
eve_eye_tail_stream_fwd_len) and the contract: every stream's states and valid outputs are those of exactly its own frames,
whatever the other streams and the frames nobody delivered hold, from one captured graph per chunk shape."""
import ctypes
import os

import pytest
import torch

import eve_amd
from eve_amd.kernels import default_kernels, dt_code
from oracle import detweights
from test_gpu_stream import gpu_clip, maxdiff
from test_stream_host import StreamFakes
from test_stream_ragged_host import CONFIGS, PACES, T_CLIP, TC, flat_state

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def make_model(dtype=torch.float32, **over):
    """test_gpu_stream.make_model for refine_net.json, also for the keys only eve_amd's configuration has; -> (model, None)"""
    cfg = eve_amd.reset_standalone_config()
    cfg.import_json(os.path.join(REPO, 'configs', 'refine_net.json'))
    cfg.import_dict(dict(eye_net_load_pretrained=False, **over))
    model = eve_amd.EVE(output_predictions=True)
    for m, seed in ((model.eye_net, 0), (model.refine_net, 1)):
        m.compute_dtype = dtype
        detweights.fill_module(m, seed)
    return model.cuda().eval(), None


def clone(d):
    return {k: v.clone() for k, v in d.items()}


# ------------------------------------------------------------------------------------------------ 1. the commit kernel
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
def test_state_rows_at_is_bit_exact(dtype):
    """dst[s] = src[s, lengths[s] - 1] for S = 5, T = 4, lengths 0, 1, 4, 2, 0: a RefineNet state's rows (5*8*64 elements, dense)
    and 130-element rows inside wider ones (frame stride 160, sequence stride 4*160 + 32, destination stride 140).  Rows of
    length 0, the gaps between the strided rows and a guard region after dst keep their contents; twice in a row."""
    k = default_kernels()
    g = torch.Generator().manual_seed(3)
    S, T = 5, 4
    n = [0, 1, 4, 2, 0]
    lengths = torch.tensor(n, dtype=torch.int32).cuda()
    for row, fstride, sstride, dstride in ((5 * 8 * 64, 5 * 8 * 64, 4 * 5 * 8 * 64, 5 * 8 * 64), (130, 160, 4 * 160 + 32, 140)):
        src_flat = torch.randn((S * sstride,), generator=g).to(dtype).cuda()
        src = src_flat.as_strided((S, T, row), (sstride, fstride, 1))
        guard = 256
        dst_flat = torch.randn((S * dstride + guard,), generator=g).to(dtype).cuda()
        dst = dst_flat.as_strided((S, row), (dstride, 1))
        if row == 5 * 8 * 64:
            src, dst = src.view(S, T, 5, 8, 64), dst.view(S, 5, 8, 64)
        want_flat = dst_flat.clone()
        want = want_flat.as_strided(dst.shape, dst.stride())
        for s in range(S):
            if n[s] > 0:
                want[s] = src[s, n[s] - 1]
        for _ in range(2):
            k.stream_state_rows_at(src, dst, lengths)
            assert torch.equal(dst_flat, want_flat), (dtype, row)      # rows, kept rows, gaps and the guard in one comparison
        for s in range(S):
            if n[s] > 0:
                assert torch.equal(dst[s], src[s, n[s] - 1]), s
    # a device length outside 0..T reads nothing outside src: above T it is the last frame, below 0 the row is kept
    wild = torch.tensor([7, -3, 1 << 30, 4, -(1 << 31)], dtype=torch.int32).cuda()
    hs = torch.randn((S, T, 130), generator=g).to(dtype).cuda()
    out = torch.randn((S, 130), generator=g).to(dtype).cuda()
    before = out.clone()
    k.stream_state_rows_at(hs, out, wild)
    for s, keep in enumerate([False, True, False, False, True]):
        assert torch.equal(out[s], before[s] if keep else hs[s, -1]), s


def test_state_rows_at_refuses_without_launching():
    k = default_kernels()
    S, T, row = 5, 4, 130
    src = torch.randn((S, T, row)).cuda()
    dst = torch.randn((S, row)).cuda()
    lengths = torch.full((S,), 2, dtype=torch.int32).cuda()
    k.stream_state_rows(dst, dst)                                  # the last launch the library has seen
    assert b'stream_state_rows_kernel' in k.lib.eve_last_kernel()
    before = dst.clone()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda T_, a, b, n: k.lib.eve_stream_state_rows_at(dt_code(torch.float32), S, T_, row, row, T * row, row, a, b, n, stream)
    whole = torch.randn((S * T * row + S * row,)).cuda()           # dst inside the span of src
    cases = {'src NULL': (T, None, p(dst), p(lengths)), 'dst NULL': (T, p(src), None, p(lengths)),
             'lengths NULL': (T, p(src), p(dst), None), 'T = 0': (0, p(src), p(dst), p(lengths)),
             'T < 0': (-1, p(src), p(dst), p(lengths)), 'in place': (T, p(src), p(src), p(lengths)),
             'overlap': (T, p(whole), ctypes.c_void_p(whole.data_ptr() + 4 * (S * T * row - row)), p(lengths))}
    for name, args in cases.items():
        assert call(*args) != 0, name
        msg = k.lib.eve_last_error().decode()
        assert msg.startswith('stream_state_rows_at:'), (name, msg)
        assert b'stream_state_rows_at' not in k.lib.eve_last_kernel(), name
    assert 'overlap' in k.lib.eve_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(dst, before)
    assert call(T, p(src), p(dst), p(lengths)) == 0                 # the same call with sound arguments is taken
    assert torch.equal(dst, src[:, 1])


# ------------------------------------------------------------------------------------------------ 2. the fused tail with lengths
def test_fused_tail_with_lengths():
    """eve_eye_tail_stream_fwd_len, S = 7 sequences of T = 35 frames (three 16-frame sub-chunks) with lengths 0, 1, 15, 16, 17,
    32, 35 -- none, inside, on and across the sub-chunks -- and reset flags on row 4 (17 frames) and row 0 (none): h[s] is hs[s,
    lengths[s] - 1] bit for bit (kept for no frames; zero when reset), and gaze / pupil / hs at the valid frames are the bits of
    the launch without lengths and within test_fused_tail_kernel_matches_float64's bounds of the float64 evaluation."""
    S, T = 7, 35
    n = [0, 1, 15, 16, 17, 32, 35]
    eve_amd.reset_standalone_config()
    net = eve_amd.EyeNet()
    net.compute_dtype = torch.float32
    detweights.fill_module(net, 0)
    net = net.cuda().eval()
    P = net._get_packs()
    w = net._stream_tail_weights(P)
    k = default_kernels()
    g = torch.Generator().manual_seed(S)
    small = detweights.eyenet_batch(1, T, seed=S + T)              # 2 eyes x 35 real frames; the 7 sequences mix their features
    batch = {kk: v.cuda() for kk, v in small.items()}
    with torch.no_grad():
        f2, _, _ = net._sequence_features(batch, P)                # [2 * T, 512]
    hp2 = torch.cat([batch['left_h'].reshape(-1, 2), batch['right_h'].reshape(-1, 2)], 0)
    rows = torch.stack([torch.roll(torch.arange(2 * T), 5 * s)[:T] for s in range(S)]).reshape(-1).cuda()
    feats, hp = f2[rows].contiguous(), hp2[rows].contiguous()
    h0 = torch.rand((S, 128), generator=g) - 0.5
    lengths = torch.tensor(n, dtype=torch.int32).cuda()
    for reset in (None, torch.tensor([1, 0, 0, 0, 1, 0, 0], dtype=torch.int32)):
        rdev = None if reset is None else reset.cuda()
        h_full = h0.clone().cuda()
        fg, fp, fhs = k.eye_tail_stream_fwd(feats, hp, w, h_full, rdev, want_hs=True)
        h = h0.clone().cuda()
        gaze, pupil, hs = k.eye_tail_stream_fwd_len(feats, hp, w, h, lengths, rdev, want_hs=True)
        hr = h0.clone()
        rg, rp, _ = StreamFakes().eye_tail_stream_fwd(feats.cpu(), hp.cpu(), tuple(t.cpu() for t in w), hr, reset, want_hs=True)
        h_in = h0.clone()
        if reset is not None:
            h_in[reset != 0] = 0
        with torch.no_grad():
            ug, _, _ = net._tail(feats, hp, S, T, [h_in.cuda()], P)
        ug = ug.view(S, T, 2)
        valid = (torch.arange(T)[None, :] < torch.tensor(n)[:, None]).cuda()
        for s in range(S):
            if n[s] == 0:
                zero = reset is not None and int(reset[s]) != 0
                assert torch.equal(h[s].cpu(), torch.zeros(128) if zero else h0[s]), s
            else:
                assert torch.equal(h[s], hs[s, n[s] - 1]), s
        assert torch.equal(gaze[valid], fg[valid]) and torch.equal(pupil[valid], fp[valid]) and torch.equal(hs[valid], fhs[valid])
        vc = valid.cpu()
        err, uerr = maxdiff(gaze.cpu()[vc], rg[vc]), maxdiff(ug.cpu()[vc], rg[vc])
        print('fused tail with lengths: |gaze - float64| %.2e rad over the valid frames (unfused float32 tail %.2e)' % (err, uerr))
        assert err <= max(1e-6, 1.5 * uerr), (err, uerr)
        assert maxdiff(gaze[valid], ug[valid]) <= max(2e-6, err + uerr)
        assert maxdiff(pupil.cpu()[vc], rp[vc]) <= 1e-5 * max(1.0, float(rp.abs().max()))
        assert torch.equal(h_full, fhs[:, -1].contiguous())


# ------------------------------------------------------------------------------------------------ model-level helpers
def padded(d, starts, Tc, seed):
    """A [B, Tc, ...] chunk on the GPU: stream b holds the clip's frames from starts[b] on, and seeded random finite values of the
    input's own dtype where the clip has no such frame (nobody delivered it)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, v in d.items():
        T = v.shape[1]
        rows = []
        for b, t0 in enumerate(starts):
            have = v[b, t0:min(T, t0 + Tc)]
            shape = (Tc - have.shape[0],) + tuple(v.shape[2:])
            pad = (torch.randint(0, 256, shape, generator=g, dtype=torch.uint8) if v.dtype == torch.uint8 else
                   torch.randn(shape, generator=g).to(v.dtype))
            rows.append(torch.cat([have, pad.cuda()], dim=0))
        out[k] = torch.stack(rows, dim=0).contiguous()
    return out


def repad(chunk, n, seed):
    """The same chunk with other random finite values in the frames t >= n[b] of stream b."""
    g = torch.Generator().manual_seed(seed)
    out = clone(chunk)
    for k, v in out.items():
        for b in range(v.shape[0]):
            shape = tuple(v[b, n[b]:].shape)
            pad = (torch.randint(0, 256, shape, generator=g, dtype=torch.uint8) if v.dtype == torch.uint8 else
                   3.0 * torch.randn(shape, generator=g).to(v.dtype))
            v[b, n[b]:] = pad.cuda()
    return out


def to_uint8_patches(d):
    """The clip with its eye patches as decoded uint8 NHWC frames (the other input form step() takes)."""
    d = dict(d)
    for side in ('left', 'right'):
        p = d[side + '_eye_patch']                                  # float NCHW [B, T, C, H, W]
        lo, hi = p.amin(), p.amax()
        d[side + '_eye_patch'] = ((p - lo) / (hi - lo) * 255).round().to(torch.uint8).permute(0, 1, 3, 4, 2).contiguous()
    return d


# ------------------------------------------------------------------------------------------------ 3. isolation, bit-exact
@pytest.mark.parametrize('dtype,use_graph,uint8', [(torch.float32, False, False), (torch.float32, True, True),
                                                   (torch.bfloat16, False, True), (torch.bfloat16, True, False)],
                         ids=['f32-eager-float', 'f32-graph-uint8', 'bf16-eager-uint8', 'bf16-graph-float'])
def test_streams_are_isolated_bit_exactly(dtype, use_graph, uint8):
    """B = 3, Tc = 4, three steps.  Stream 0 delivers every frame: its outputs and states are the bits of a run without lengths.
    Streams 1 and 2 are ragged (a step without frames among them): their valid outputs and committed states do not change by a
    bit when the frames they did not deliver hold other values."""
    model, _ = make_model(dtype=dtype)
    _, d, _ = gpu_clip(3, 12, seed=6)
    if uint8:
        d = to_uint8_patches(d)
    ns = [[4, 2, 0], [4, 0, 3], [4, 1, 4]]
    chunks = [{k: v[:, 4 * i:4 * i + 4].contiguous() for k, v in d.items()} for i in range(3)]
    plain = eve_amd.EVEStream(model, 3, use_graph=use_graph)
    a = eve_amd.EVEStream(model, 3, use_graph=use_graph)
    b = eve_amd.EVEStream(model, 3, use_graph=use_graph)
    for i, n in enumerate(ns):
        want = clone(plain.step(chunks[i]))
        oa = clone(a.step(repad(chunks[i], n, 20 + i), lengths=n))
        ob = clone(b.step(repad(chunks[i], n, 40 + i), lengths=torch.tensor(n)))
        assert oa.pop('valid').tolist() == ob.pop('valid').tolist() == [[t < n[s] for t in range(4)] for s in range(3)]
        for k in want:
            assert torch.equal(oa[k][0], want[k][0]), (i, k)
            for s in (1, 2):
                assert torch.equal(oa[k][s, :n[s]], ob[k][s, :n[s]]), (i, k, s)
        sa, sb, sp = flat_state(a.get_state()), flat_state(b.get_state()), flat_state(plain.get_state())
        for (k, j, x), (_, _, y), (_, _, z) in zip(sa, sb, sp):
            assert torch.equal(x[0], z[0]), (i, k, j)
            assert torch.equal(x[1:], y[1:]), (i, k, j)
            assert torch.isfinite(x).all(), (i, k, j)


# ------------------------------------------------------------------------------------------------ 4. a ragged split is a split
def run_paces(stream, d, paces, Tc, seed=11):
    B = len(paces[0])
    pos, parts = [0] * B, [[] for _ in range(B)]
    for i, n in enumerate(paces):
        out = stream.step(padded(d, pos, Tc, seed + i), lengths=list(n))
        out.pop('valid')
        for b in range(B):
            parts[b].append({k: v[b, :n[b]].clone() for k, v in out.items()})
            pos[b] += n[b]
    return {k: torch.stack([torch.cat([p[k] for p in parts[b]], dim=0) for b in range(B)], dim=0) for k in parts[0][0]}


def uniform_states(model, d):
    s = eve_amd.EVEStream(model, 3, use_graph=False)
    for t0 in range(0, T_CLIP, TC):
        s.step({k: v[:, t0:t0 + TC].contiguous() for k, v in d.items()})
    return flat_state(s.get_state())


@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_ragged_split_float32_matches_the_whole_clip(name):
    """Three streams consume one 10-frame clip at different paces in steps of 4 frames (hipGraph; one stream idle in one step, a
    partial last step, random values in the frames nobody delivered), against one EVE.eval() pass of the whole clip under the
    bounds of test_stream_float32_matches_the_whole_clip: 1e-5 rad / 1e-2 px / 1e-3 cm, five times that on the refined keys.
    The carried states afterwards equal those of the uniform run of the same frames: EyeNet's under the initial gaze's bound,
    RefineNet's (behind the heat-map of that gaze, on the refined keys' path) under the refined keys'."""
    over, fused = CONFIGS[name]
    model, _ = make_model(**over)
    model.eye_net.stream_fused_tail = fused
    _, d, full = gpu_clip(3, T_CLIP, seed=9)
    with torch.no_grad():
        whole = model(dict(full))
        feats = model.eye_net.forward_sequence(d)
    whole.update({k: feats[k] for k in ('left_g_initial', 'right_g_initial')})
    ragged = eve_amd.EVEStream(model, 3)
    got = run_paces(ragged, d, PACES, TC)
    assert len(ragged._graphs) == 1
    report = {}
    for k, v in got.items():
        if k in whole:
            report[k] = maxdiff(v, whole[k])
    print('ragged vs whole clip (%s): %s' % (name, ', '.join('%s %.1e' % kv for kv in sorted(report.items()))))
    for k, e in report.items():
        amp = 5.0 if k.endswith('_final') else 1.0
        assert e <= amp * (1e-2 if 'px' in k else (1e-3 if 'cm' in k else 1e-5)), (k, e)
    assert len(report) >= 6
    for (k, i, a), (_, _, b) in zip(flat_state(ragged.get_state()), uniform_states(model, d)):
        e = maxdiff(a, b)
        print('state %s[%d]: ragged vs uniform %.1e' % (k, i, e))
        assert e <= (5e-5 if k.startswith('refinenet') else 1e-5), (k, i, e)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_ragged_split_half_precision_matches_the_same_dtype_whole_clip(dtype):
    """The shipped pipeline in bf16 / fp16 under test_stream_half_precision_matches_the_same_dtype_whole_clip's bound: the ragged
    stream's deviation from the same dtype's whole-clip pass stays inside that pass's own distance to float32; and each carried
    state's deviation from the uniform run of the same frames inside that state's own distance to the float32 model's."""
    model, _ = make_model(dtype=dtype)
    m32, _ = make_model()
    _, d, full = gpu_clip(3, T_CLIP, seed=9)
    with torch.no_grad():
        whole, w32 = model(dict(full)), m32(dict(full))
    ragged = eve_amd.EVEStream(model, 3)
    got = run_paces(ragged, d, PACES, TC)
    for k in ('g_initial', 'g_final', 'PoG_px_initial', 'PoG_px_final'):
        noise = maxdiff(whole[k], w32[k])
        dev = maxdiff(got[k], whole[k])
        print('%s %s: ragged vs whole %.2e, dtype noise %.2e' % (dtype, k, dev, noise))
        assert dev <= noise + (1e-2 if 'px' in k else 1e-5), (k, dev, noise)
    for (k, i, a), (_, _, b), (_, _, c) in zip(flat_state(ragged.get_state()), uniform_states(model, d), uniform_states(m32, d)):
        e, noise = maxdiff(a, b), maxdiff(b, c)
        print('%s state %s[%d]: ragged vs uniform %.2e, dtype noise %.2e' % (dtype, k, i, e, noise))
        assert e <= noise + 1e-5, (k, i, e, noise)


# ------------------------------------------------------------------------------------------------ 5. one graph per shape
def test_one_ragged_graph_serves_every_length_pattern():
    model, _ = make_model(refine_net_rnn_type='CGRU')
    _, d, _ = gpu_clip(3, 16, seed=7)
    ch = lambda i: {k: v[:, 4 * i:4 * i + 4].contiguous() for k, v in d.items()}
    g, e = eve_amd.EVEStream(model, 3), eve_amd.EVEStream(model, 3, use_graph=False)
    never = eve_amd.EVEStream(model, 3)
    for i, n in enumerate(([4, 1, 0], [0, 4, 2], [3, 3, 4])):
        og, oe = g.step(ch(i), lengths=n), e.step(ch(i), lengths=n)
        assert set(og) == set(oe) and 'valid' in og
        for k in og:
            assert torch.equal(og[k], oe[k]), (i, k)
        for (k, j, x), (_, _, y) in zip(flat_state(g.get_state()), flat_state(e.get_state())):
            assert torch.equal(x, y), (i, k, j)
    assert [key[1] for key in g._graphs] == [True]                  # one ragged graph, lengths not baked in
    never.set_state(g.get_state())
    og, on = g.step(ch(3)), never.step(ch(3))
    assert 'valid' not in og and sorted(key[1] for key in g._graphs) == [False, True] and len(never._graphs) == 1
    for k in on:
        assert torch.equal(og[k], on[k]), k
    for (k, j, x), (_, _, y) in zip(flat_state(g.get_state()), flat_state(never.get_state())):
        assert torch.equal(x, y), (k, j)


# ------------------------------------------------------------------------------------------------ 6. reset without frames
@pytest.mark.parametrize('fused', [False, True], ids=['layers', 'fused-tail'])
def test_reset_reaches_a_stream_without_frames(fused):
    model, _ = make_model(refine_net_rnn_type='CGRU')
    model.eye_net.stream_fused_tail = fused
    _, d, _ = gpu_clip(3, 8, seed=6)
    ch = lambda t0, t1: {k: v[:, t0:t1].contiguous() for k, v in d.items()}
    s, plain = eve_amd.EVEStream(model, 3), eve_amd.EVEStream(model, 3)
    s.step(ch(0, 4))
    plain.step(ch(0, 4))
    s.reset([1])
    a = clone(s.step(ch(4, 8), lengths=[4, 0, 4]))
    want = clone(plain.step(ch(4, 8)))
    for k in want:
        assert torch.equal(a[k][[0, 2]], want[k][[0, 2]]), k
    for (k, j, x), (_, _, y) in zip(flat_state(s.get_state()), flat_state(plain.get_state())):
        assert torch.equal(x[[0, 2]], y[[0, 2]]), (k, j)
        assert not x[1].any() and y[1].any(), (k, j)
