"""CPU: the host logic of eve_amd.EVEStream and of the state plumbing under it (RefineNet.forward_sequence(initial_states=...),
EVE._predict_sequence), with the torch-CPU stand-in of tests/fake_kernels.py extended by float64 restatements of the two
streaming entry points (eve_eye_tail_stream_fwd, eve_stream_state_rows).  The GPU suite (test_gpu_stream.py) checks the HIP
kernels and the graph mode."""
import math
import os

import numpy as np
import pytest
import torch

import eve_amd
from eve_amd import kernels
from fake_kernels import FakeKernels
from oracle import detweights
from oracle.config import OracleConfig
from oracle.eye_net import EyeNet as OracleEyeNet
from oracle.refine_net import RefineNet as OracleRefineNet

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNKS = [7, 1, 1, 13, 8]


def tol(k):
    # chunked (float64 stand-in of the fused tail) vs whole clip (float32 tail): rad, px (PoG ~ 1 000 px), cm; the refined keys
    # come through the soft-argmax of a sharp heat-map (beta 100), which amplifies the initial gaze's last-bit differences
    amp = 10.0 if k.endswith('final') else 1.0
    return amp * (1e-2 if 'px' in k else (1e-3 if 'cm' in k else 1e-5))
PRED = ('left_g_initial', 'right_g_initial', 'left_pupil_size', 'right_pupil_size', 'g_initial', 'PoG_px_initial', 'PoG_cm_initial')
FINAL = ('g_final', 'PoG_px_final', 'PoG_cm_final')


class StreamFakes(FakeKernels):
    """FakeKernels plus include/eve_hip.h eve_eye_tail_stream_fwd (evaluated in float64) and eve_stream_state_rows."""

    def __init__(self):
        self.calls = []

    def eye_tail_stream_fwd(self, feats, head_pose, weights, h, reset=None, want_hs=False):
        self.calls.append('eye_tail_stream_fwd')
        w = [t.double().reshape(t.shape[0], -1) for t in weights]       # [in, out]
        fc_w, fc_b, c0_w, c0_b, c2_w, c2_b, ih_w, ih_b, hh_w, hh_b, g0_w, g0_b, g2_w, p0_w, p0_b, p2_w, p2_b = w
        fc_b, c0_b, c2_b, ih_b, hh_b, g0_b, p0_b, p2_b = (b.reshape(-1) for b in (fc_b, c0_b, c2_b, ih_b, hh_b, g0_b, p0_b, p2_b))
        selu = torch.nn.functional.selu
        S = h.shape[0]
        T = feats.shape[0] // S
        f = feats.double() @ fc_w + fc_b
        f = torch.cat([f, head_pose.double()], 1)
        f = torch.nn.functional.pad(f, (0, c0_w.shape[0] - f.shape[1]))
        f = selu(f @ c0_w + c0_b) @ c2_w + c2_b
        gi = (f @ ih_w + ih_b).view(S, T, 384)
        hh = h.double().clone()
        if reset is not None:
            hh[reset[:S] != 0] = 0
        hs = []
        for t in range(T):
            gh = hh @ hh_w + hh_b
            r = torch.sigmoid(gi[:, t, :128] + gh[:, :128])
            z = torch.sigmoid(gi[:, t, 128:256] + gh[:, 128:256])
            n = torch.tanh(gi[:, t, 256:] + r * gh[:, 256:])
            hh = (1 - z) * n + z * hh
            hs.append(hh)
        hs = torch.stack(hs, 1)
        x = hs.reshape(S * T, 128)
        g = torch.tanh(selu(x @ g0_w + g0_b) @ g2_w[:, :2]) * (0.5 * math.pi)
        p = torch.relu(selu(x @ p0_w + p0_b) @ p2_w[:, :1] + p2_b)
        h.copy_(hh.float())
        return g.float().view(S, T, 2), p.float().view(S, T), (hs.float() if want_hs else None)

    def stream_state_rows(self, src, dst, reset=None):
        self.calls.append('stream_state_rows')
        v = src.clone()
        if reset is not None:
            v[reset[:dst.shape[0]] != 0] = 0
        dst.copy_(v)
        return dst


@pytest.fixture()
def fake():
    k = StreamFakes()
    kernels.set_default_kernels(k)
    yield k
    kernels.set_default_kernels(None)
    eve_amd.reset_standalone_config()


def make_model(over, seed_eye=0, seed_ref=1):
    json_path = os.path.join(REPO, 'configs', 'refine_net.json')
    cfg = eve_amd.reset_standalone_config()
    cfg.import_json(json_path)
    cfg.import_dict(dict(eye_net_load_pretrained=False, **over))
    model = eve_amd.EVE(output_predictions=True)
    detweights.fill_module(model.eye_net, seed_eye)
    if model.refine_net is not None:
        detweights.fill_module(model.refine_net, seed_ref)
    for m in (model.eye_net, model.refine_net):
        if m is not None:
            m.compute_dtype = torch.float32
    return model.eval(), OracleConfig(json_path, eye_net_load_pretrained=False, **over)


INPUT_KEYS = ('left_eye_patch', 'right_eye_patch', 'left_h', 'right_h', 'left_o', 'right_o', 'left_R', 'right_R', 'head_R',
              'camera_transformation', 'inv_camera_transformation', 'pixels_per_millimeter', 'millimeters_per_pixel', 'screen_frame')


def clip(B, T, seed=4, size=64):
    b = detweights.eve_batch(B, T, seed=seed)
    for side in ('left', 'right'):                 # small patches keep the CPU trunk quick (any size >= 32 is a valid input)
        b[side + '_eye_patch'] = b[side + '_eye_patch'][..., :size, :size].contiguous()
    return b


def chunk_of(batch, t0, t1):
    return {k: batch[k][:, t0:t1].contiguous() for k in INPUT_KEYS if k in batch}


def run_chunks(stream, batch, sizes):
    outs, t0 = [], 0
    for n in sizes:
        outs.append({k: v.clone() for k, v in stream.step(chunk_of(batch, t0, t0 + n)).items()})
        t0 += n
    return {k: torch.cat([o[k] for o in outs], dim=1) for k in outs[0]}


@pytest.mark.parametrize('over,fused', [(dict(refine_net_rnn_type='CGRU'), True), (dict(refine_net_rnn_type='CGRU'), False),
                                        (dict(refine_net_rnn_type='CLSTM'), False)], ids=['cgru-fused', 'cgru', 'clstm'])
def test_chunked_stream_matches_the_whole_clip_and_the_oracle(fake, over, fused):
    """Chunks of 7, 1, 1, 13 and 8 frames through EVEStream equal one eval pass of the 30-frame clip (same kernels), and the
    oracle's per-frame evaluation of the reference's data flow on the whole clip; with the EyeNet tail layer by layer (the
    default) and as the one fused launch."""
    from oracle import eve as oracle_eve
    model, ocfg = make_model(over)
    model.eye_net.stream_fused_tail = fused
    batch = clip(1, 30)
    got = run_chunks(eve_amd.EVEStream(model, 1, use_graph=False), batch, CHUNKS)
    assert ('eye_tail_stream_fwd' in fake.calls) == fused
    with torch.no_grad():
        whole = model(dict(batch))
    for k in PRED + FINAL:
        if k in whole:                  # (the per-eye gaze is not an output of EVE.forward; the oracle check below covers it)
            assert float((got[k] - whole[k]).abs().max()) < tol(k), k
    oeye = detweights.fill_module(OracleEyeNet(ocfg), 0)
    oref = detweights.fill_module(OracleRefineNet(ocfg), 1)
    with torch.no_grad():
        _, winter, _ = oracle_eve.eve_forward(oeye, oref, dict(batch), ocfg, False)
    for k in PRED + FINAL:
        assert float((got[k] - winter[k]).abs().max()) < (0.5 if 'px' in k else (2e-2 if 'cm' in k else 4e-3)), k   # (float32 fakes, soft-argmax beta 100)


def test_non_fused_variants_carry_their_state(fake):
    """EyeNet LSTM (two stacked cells: the per-cell scans with the stream_state_rows hand-over) with RefineNet CRNN, and a STATIC
    EyeNet without RefineNet: chunked equals whole clip."""
    for over in (dict(eye_net_rnn_type='LSTM', eye_net_rnn_num_cells=2, refine_net_rnn_type='CRNN'),
                 dict(eye_net_use_rnn=False, refine_net_enabled=False)):
        fake.calls.clear()
        model, _ = make_model(over)
        batch = clip(1, 9, seed=6)
        got = run_chunks(eve_amd.EVEStream(model, 1, use_graph=False), batch, [4, 1, 4])
        assert 'eye_tail_stream_fwd' not in fake.calls
        with torch.no_grad():
            whole = model(dict(batch))
        for k in got:
            if k in whole:
                assert float((got[k] - whole[k]).abs().max()) < tol(k), (over, k)


def test_reset_restarts_one_stream_and_leaves_the_others(fake):
    model, _ = make_model(dict(refine_net_rnn_type='CGRU'))
    batch = clip(2, 6, seed=7)
    plain = eve_amd.EVEStream(model, 2, use_graph=False)
    a = plain.step(chunk_of(batch, 0, 3)), plain.step(chunk_of(batch, 3, 6))
    st = eve_amd.EVEStream(model, 2, use_graph=False)
    st.step(chunk_of(batch, 0, 3))
    st.reset([1])
    b = st.step(chunk_of(batch, 3, 6))
    fresh = eve_amd.EVEStream(model, 2, use_graph=False).step(chunk_of(batch, 3, 6))
    for k in b:
        assert torch.equal(b[k][0], a[1][k][0]), k               # stream 0: untouched by the reset
        assert torch.equal(b[k][1], fresh[k][1]), k              # stream 1: as if it had started at this chunk
        assert not torch.equal(b[k][1], a[1][k][1]) or k.endswith('pupil_size'), k
    st.reset(np.array([True, False]))                            # masks work too, and a reset does not leak into the next step
    st.step(chunk_of(batch, 0, 1))
    assert not st._flags.any()


def test_get_state_set_state_round_trip(fake):
    model, _ = make_model(dict(refine_net_rnn_type='CLSTM'))
    batch = clip(2, 5, seed=8)
    a = eve_amd.EVEStream(model, 2, use_graph=False)
    a.step(chunk_of(batch, 0, 3))
    st = a.get_state()
    assert tuple(st['left_eye_rnn_states_0'].shape) == (2, 128) and tuple(st['right_eye_rnn_states_0'].shape) == (2, 128)
    h, c = st['refinenet_rnn_states_0']
    assert tuple(h.shape) == tuple(c.shape) == (2, 64, 5, 8) and h.dtype == torch.float32
    b = eve_amd.EVEStream(model, 2, use_graph=False)
    b.set_state(st)
    for k, v in b.get_state().items():
        for x, y in zip(v if isinstance(v, tuple) else (v,), st[k] if isinstance(st[k], tuple) else (st[k],)):
            assert torch.equal(x, y), k
    oa, ob = a.step(chunk_of(batch, 3, 5)), b.step(chunk_of(batch, 3, 5))
    for k in oa:
        assert torch.equal(oa[k], ob[k]), k


def test_refinenet_initial_states_and_default_path(fake):
    """forward_sequence's default arguments give what they gave before (bit-identical to initial_states=None), and a clip split
    in two with the first half's last state (reference layout, or the internal one) as initial_states equals the whole clip."""
    for rnn in ('CGRU', 'CRNN', 'CLSTM'):
        model, _ = make_model(dict(refine_net_rnn_type=rnn))
        net = model.refine_net
        rb = detweights.refinenet_batch(2, 6, seed=3)
        with torch.no_grad():
            hf, st = net.forward_sequence(rb['heatmap_initial'], rb['screen_frame'])
            hf2, st2 = net.forward_sequence(rb['heatmap_initial'], rb['screen_frame'], initial_states=None)
            assert torch.equal(hf, hf2)
            a, sa = net.forward_sequence(rb['heatmap_initial'][:, :4], rb['screen_frame'][:, :4])
            last = [tuple(t[:, -1] for t in s_) if isinstance(s_, tuple) else s_[:, -1] for s_ in sa]
            b, sb = net.forward_sequence(rb['heatmap_initial'][:, 4:], rb['screen_frame'][:, 4:], initial_states=last)
            internal = [tuple(t.permute(0, 2, 3, 1).contiguous() for t in s_) if isinstance(s_, tuple) else
                        s_.permute(0, 2, 3, 1).contiguous() for s_ in last]
            b2, _ = net.forward_sequence(rb['heatmap_initial'][:, 4:], rb['screen_frame'][:, 4:], initial_states=internal)
        assert float((torch.cat([a, b], 1) - hf).abs().max()) < 1e-5, rnn
        assert float((b2 - b).abs().max()) < 1e-6, rnn
        s_whole = st[0][0] if isinstance(st[0], tuple) else st[0]
        s_b = sb[0][0] if isinstance(sb[0], tuple) else sb[0]
        assert float((s_b - s_whole[:, 4:]).abs().max()) < 1e-5, rnn


def test_stream_needs_eval_mode(fake):
    model, _ = make_model(dict(refine_net_rnn_type='CGRU'))
    with pytest.raises(ValueError):
        eve_amd.EVEStream(model.train(), 1, use_graph=False)
    with pytest.raises(ValueError):
        eve_amd.EVEStream(model.eval(), 1, use_graph=True)          # graphs need the GPU
    s = eve_amd.EVEStream(model, 1, use_graph=False)
    model.train()
    with pytest.raises(ValueError):
        s.step(chunk_of(clip(1, 1), 0, 1))
