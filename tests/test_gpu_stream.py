"""GPU: streaming EVE inference (eve_amd.EVEStream) -- the two HIP entry points behind it (eve_eye_tail_stream_fwd,
eve_stream_state_rows) and the contract: a clip streamed in chunks of any sizes equals one eval pass of the whole clip."""
import os

import pytest
import torch

import eve_amd
from eve_amd.kernels import default_kernels
from oracle import detweights
from oracle import eve as oracle_eve
from oracle.config import OracleConfig
from test_stream_host import CHUNKS, StreamFakes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
INPUT_KEYS = ('left_eye_patch', 'right_eye_patch', 'left_h', 'right_h', 'left_o', 'right_o', 'left_R', 'right_R', 'head_R',
              'camera_transformation', 'inv_camera_transformation', 'pixels_per_millimeter', 'millimeters_per_pixel', 'screen_frame')


def make_model(config='refine_net.json', dtype=torch.float32, seeds=(0, 1), **over):
    json_path = os.path.join(REPO, 'configs', config)
    cfg = eve_amd.reset_standalone_config()
    cfg.import_json(json_path)
    cfg.import_dict(dict(eye_net_load_pretrained=False, **over))
    model = eve_amd.EVE(output_predictions=True)
    for m, seed in zip((model.eye_net, model.refine_net), seeds):
        if m is not None:
            m.compute_dtype = dtype
            detweights.fill_module(m, seed)
    return model.cuda().eval(), OracleConfig(json_path, eye_net_load_pretrained=False, **over)


def gpu_clip(B, T, seed=4):
    """-> (the CPU batch, the stream's chunk keys on the GPU, every key on the GPU for EVE.forward)"""
    b = detweights.eve_batch(B, T, seed=seed)
    return b, {k: b[k].cuda() for k in INPUT_KEYS if k in b}, {k: v.cuda() for k, v in b.items()}


def run_chunks(stream, d, sizes):
    outs, t0 = [], 0
    for n in sizes:
        outs.append({k: v.clone() for k, v in stream.step({k: v[:, t0:t0 + n].contiguous() for k, v in d.items()}).items()})
        t0 += n
    return {k: torch.cat([o[k] for o in outs], dim=1) for k in outs[0]}


def maxdiff(a, b):
    return float((a.float() - b.float()).abs().max())


# ------------------------------------------------------------------------------------------------ 1. the fused tail kernel
@pytest.mark.parametrize('S', [2, 64])
def test_fused_tail_kernel_matches_float64(S):
    """eve_eye_tail_stream_fwd against the float64 evaluation of the same tail (tests/test_stream_host.py StreamFakes) on the
    trunk's features of real patches, for Tc = 1, 7, 30 and 37 (> the kernel's 16-frame LDS sub-chunk), with and without reset
    flags: gaze within 1e-6 rad of float64 -- or, on the frames where the unfused float32 tail itself is further than that
    (0.96-1.13e-6 rad measured), within 1.5 x its distance -- the state written back equals hs[:, -1] bit for bit; and within
    2e-6 rad (or the two distances added) of the unfused layer-by-layer `_tail`."""
    eve_amd.reset_standalone_config()
    net = eve_amd.EyeNet()
    net.compute_dtype = torch.float32
    detweights.fill_module(net, 0)
    net = net.cuda().eval()
    P = net._get_packs()
    w = net._stream_tail_weights(P)
    k = default_kernels()
    ref = StreamFakes()
    g = torch.Generator().manual_seed(S)
    worst, worst_unfused = 0.0, 0.0
    for T in (1, 7, 30, 37):
        batch = {kk: v.cuda() for kk, v in detweights.eyenet_batch(S // 2, T, seed=S + T).items()}
        with torch.no_grad():
            feats, _, _ = net._sequence_features(batch, P)
        hp = torch.cat([batch['left_h'].reshape(-1, 2), batch['right_h'].reshape(-1, 2)], 0).contiguous()
        h0 = (torch.rand((S, 128), generator=g) - 0.5)
        fc, hpc = feats.cpu(), hp.cpu()
        for reset in (None, torch.tensor([i % 3 == 1 for i in range(S)], dtype=torch.int32)):
            h = h0.clone().cuda()
            gaze, pupil, hs = k.eye_tail_stream_fwd(feats, hp, w, h, None if reset is None else reset.cuda(), want_hs=True)
            hr = h0.clone()
            rg, rp, rhs = ref.eye_tail_stream_fwd(fc, hpc, tuple(t.cpu() for t in w), hr, reset, want_hs=True)
            h_in = h0.clone()
            if reset is not None:
                h_in[reset != 0] = 0
            with torch.no_grad():
                ug, up, _ = net._tail(feats, hp, S, T, [h_in.cuda()], P)
            err, uerr = maxdiff(gaze.cpu(), rg), maxdiff(ug.cpu(), rg.view(-1, 2))
            worst, worst_unfused = max(worst, err), max(worst_unfused, uerr)
            assert err <= max(1e-6, 1.5 * uerr), (T, reset is not None, err, uerr)
            assert maxdiff(gaze.view(-1, 2), ug) <= max(2e-6, err + uerr), T
            assert maxdiff(pupil.cpu(), rp) <= 1e-5 * max(1.0, float(rp.abs().max()))
            assert torch.equal(h, hs[:, -1].contiguous())
            assert maxdiff(h.cpu(), hr) <= 1e-5
    print('fused tail, S = %d: worst |gaze - float64| %.2e rad (unfused float32 tail: %.2e)' % (S, worst, worst_unfused))


# ------------------------------------------------------------------------------------------------ 2. the state kernel
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
def test_state_rows_are_bit_exact(dtype):
    k = default_kernels()
    g = torch.Generator().manual_seed(3)
    hs = torch.randn((5, 4, 5, 8, 64), generator=g).to(dtype).cuda()         # [S, T, ...]: the last frame is a strided view
    buf = torch.randn((5, 5, 8, 64), generator=g).to(dtype).cuda()
    k.stream_state_rows(hs[:, -1], buf)
    assert torch.equal(buf, hs[:, -1])
    flags = torch.tensor([0, 1, 0, 0, 1], dtype=torch.int32).cuda()
    before = buf.clone()
    k.stream_state_rows(buf, buf, flags)                                      # in place: resets
    for s in range(5):
        assert torch.equal(buf[s], torch.zeros_like(buf[s]) if s in (1, 4) else before[s])
    out = torch.empty_like(buf)
    k.stream_state_rows(hs[:, 2], out, flags)
    for s in range(5):
        assert torch.equal(out[s], torch.zeros_like(out[s]) if s in (1, 4) else hs[s, 2])


# ------------------------------------------------------------------------------------------------ 3. continuity, float32
@pytest.mark.parametrize('config,over,fused', [('refine_net.json', dict(refine_net_rnn_type='CGRU'), True),
                                               ('refine_net.json', {}, False), ('eye_net.json', {}, False)],
                         ids=['cgru-fused-tail', 'clstm', 'eyenet'])
def test_stream_float32_matches_the_whole_clip(config, over, fused):
    """30 frames of 2 streams, streamed (hipGraph) in chunks of 7, 1, 1, 13, 8 and frame by frame, against one EVE.eval() pass
    of the whole clip: <= 1e-5 rad on the initial gaze, <= 1e-2 px on its PoG; five times that on the refined keys, whose
    soft-argmax of a sharp heat-map (beta 100) amplifies the streamed pass's last-bit differences from the whole-clip one about
    tenfold (with the fused tail: 1.6-1.7e-6 rad on the initial gaze, PoG_px_final 1.1-1.8e-2 px).  For the CGRU pipeline also against the float64 oracle on the
    whole clip: <= 1e-4 rad (the project's parity statement; g_final with the float32 oracle's own deviation as slack)."""
    model, ocfg = make_model(config, **over)
    model.eye_net.stream_fused_tail = fused
    b, d, full = gpu_clip(2, 30)
    with torch.no_grad():
        whole = model(dict(full))
        feats = model.eye_net.forward_sequence(d)
    whole.update({k: feats[k] for k in ('left_g_initial', 'right_g_initial')})
    chunked = run_chunks(eve_amd.EVEStream(model, 2), d, CHUNKS)
    frames = run_chunks(eve_amd.EVEStream(model, 2), d, [1] * 30)
    report = {}
    for name, got in (('chunks', chunked), ('frames', frames)):
        for k, v in got.items():
            if k in whole:
                e = maxdiff(v, whole[k])
                report['%s %s' % (name, k)] = e
                amp = 5.0 if k.endswith('_final') else 1.0
                assert e <= amp * (1e-2 if 'px' in k else (1e-3 if 'cm' in k else 1e-5)), (name, k, e)
    print('stream vs whole clip (%s %s): %s' % (config, over, ', '.join('%s %.1e' % kv for kv in sorted(report.items()))))
    if over.get('refine_net_rnn_type') == 'CGRU':
        from oracle.eye_net import EyeNet as OracleEyeNet
        from oracle.refine_net import RefineNet as OracleRefineNet
        b1 = {k: v[:1] for k, v in b.items()}
        torch.set_default_dtype(torch.float64)
        try:
            oeye = detweights.fill_module(OracleEyeNet(ocfg), 0).double()
            oref = detweights.fill_module(OracleRefineNet(ocfg), 1).double()
            with torch.no_grad():
                _, w64, _ = oracle_eve.eve_forward(oeye, oref, {k: (v.double() if v.is_floating_point() else v) for k, v in b1.items()},
                                                   ocfg, False)
        finally:
            torch.set_default_dtype(torch.float32)
        with torch.no_grad():
            _, w32, _ = oracle_eve.eve_forward(detweights.fill_module(OracleEyeNet(ocfg), 0),
                                               detweights.fill_module(OracleRefineNet(ocfg), 1), dict(b1), ocfg, False)
        for k in ('g_initial', 'g_final'):
            slack = float((w32[k].double() - w64[k]).abs().max()) if k == 'g_final' else 0.0
            e = float((chunked[k][:1].cpu().double() - w64[k]).abs().max())
            print('%s vs float64 oracle: %.2e rad (float32 oracle: %.2e)' % (k, e, float((w32[k].double() - w64[k]).abs().max())))
            assert e <= 1e-4 + slack, (k, e)


# ------------------------------------------------------------------------------------------------ 4. continuity, 16-bit
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_stream_half_precision_matches_the_same_dtype_whole_clip(dtype):
    """Streamed vs the same dtype's whole-clip pass (shipped CLSTM pipeline): the deviation stays inside the dtype's own noise on
    this network, taken as its whole-clip pass against the float32 one (the envelope test_gpu_bf16_parity.py's end-to-end tests
    bound the kernels by).  It is not zero: a chunk folds fewer frames into the trunk's image batch, which selects other
    convolution tiles and so other 16-bit roundings.  Measured on g_initial: bf16 6.7e-3 rad (noise 2.2e-2), fp16 1.2e-3 rad
    (noise 3.8e-3)."""
    model, _ = make_model(dtype=dtype)
    m32, _ = make_model()
    _, d, full = gpu_clip(2, 30, seed=5)
    with torch.no_grad():
        whole, w32 = model(dict(full)), m32(dict(full))
    got = run_chunks(eve_amd.EVEStream(model, 2), d, CHUNKS)
    for k in ('g_initial', 'g_final', 'PoG_px_initial', 'PoG_px_final'):
        noise = maxdiff(whole[k], w32[k])
        dev = maxdiff(got[k], whole[k])
        print('%s %s: stream vs whole %.2e, dtype noise %.2e' % (dtype, k, dev, noise))
        assert dev <= noise + (1e-2 if 'px' in k else 1e-5), (k, dev, noise)


# ------------------------------------------------------------------------------------------------ 5. reset
def test_reset_restarts_exactly_one_stream():
    model, _ = make_model(refine_net_rnn_type='CGRU')
    _, d, _ = gpu_clip(3, 6, seed=6)
    ch = lambda t0, t1: {k: v[:, t0:t1].contiguous() for k, v in d.items()}
    plain = eve_amd.EVEStream(model, 3)
    plain.step(ch(0, 3))
    a = {k: v.clone() for k, v in plain.step(ch(3, 6)).items()}
    s = eve_amd.EVEStream(model, 3)
    s.step(ch(0, 3))
    s.reset([1])
    b = {k: v.clone() for k, v in s.step(ch(3, 6)).items()}
    fresh = eve_amd.EVEStream(model, 3, use_graph=False).step(ch(3, 6))
    for k in b:
        assert torch.equal(b[k][[0, 2]], a[k][[0, 2]]), k
        assert torch.equal(b[k][1], fresh[k][1]), k


# ------------------------------------------------------------------------------------------------ 6. graph
def test_graph_replay_equals_eager_and_follows_new_weights():
    model, _ = make_model(refine_net_rnn_type='CGRU')
    _, d, _ = gpu_clip(2, 12, seed=7)
    sizes = [3, 3, 3, 3]                                     # one captured shape, replayed with refilled inputs
    g = run_chunks(eve_amd.EVEStream(model, 2), d, sizes)
    e = run_chunks(eve_amd.EVEStream(model, 2, use_graph=False), d, sizes)
    for k in g:
        assert torch.equal(g[k], e[k]), k
    other, _ = make_model(refine_net_rnn_type='CGRU', seeds=(2, 3))
    s = eve_amd.EVEStream(model, 2)
    ch = lambda t0, t1: {k: v[:, t0:t1].contiguous() for k, v in d.items()}
    s.step(ch(0, 3))
    state = s.get_state()
    model.load_state_dict(other.state_dict())
    got = s.step(ch(3, 6))
    ref = eve_amd.EVEStream(other, 2, use_graph=False)
    ref.set_state(state)
    want = ref.step(ch(3, 6))
    for k in want:
        assert torch.equal(got[k], want[k]), k


# ------------------------------------------------------------------------------------------------ 7. a non-fused variant
def test_lstm_eyenet_with_crnn_refinenet():
    model, _ = make_model(eye_net_rnn_type='LSTM', refine_net_rnn_type='CRNN')
    _, d, full = gpu_clip(2, 10, seed=8)
    with torch.no_grad():
        whole = model(dict(full))
    got = run_chunks(eve_amd.EVEStream(model, 2), d, [4, 1, 5])
    for k in ('g_initial', 'g_final', 'PoG_px_final'):
        e = maxdiff(got[k], whole[k])
        print('LSTM + CRNN %s: %.2e' % (k, e))
        assert e <= (1e-2 if 'px' in k else 1e-5), (k, e)
