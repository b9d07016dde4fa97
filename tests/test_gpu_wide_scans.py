"""GPU: the wide recurrent scans (csrc/recurrent_wide.hip; 256 < H <= 1024, H % 16 == 0) -- EyeNet with
eye_net_rnn_num_features above 256, from the kernels up to training and streaming.

Kernel level: the pattern of test_gru_scan / test_rnn_and_lstm_scans in tests/test_gpu_kernels.py, with that file's
CPU stand-in (tests/fake_kernels.py) and its close() helper, float32 bound included.
"""
import pytest
import torch

from fake_kernels import FakeKernels
from test_gpu_kernels import close, dev, rnd

pytestmark = pytest.mark.gpu

WIDTH_RULE = 'H <= 256, or a multiple of 16 up to 1024'


@pytest.fixture(scope='module')
def hip():
    from eve_amd.kernels import HipKernels
    assert torch.cuda.is_available(), 'GPU suite needs a GPU'
    return HipKernels()


@pytest.fixture(scope='module')
def ref():
    return FakeKernels()


def last_kernel(hip):
    return hip.lib.eve_last_kernel().decode()


# ------------------------------------------------------------------------------------------------ 1. kernel level
# S = 5: a partial tile of 16 sequences; 16: exactly one tile; 37: two tiles and a partial one.
@pytest.mark.parametrize('S', [5, 16, 37])
@pytest.mark.parametrize('H', [272, 512, 1024])
def test_wide_gru_scan(hip, ref, H, S):
    T = 7
    gi = rnd((S, T, 3 * H), torch.float32, 31)
    whh = rnd((3 * H, H), torch.float32, 32, scale=H ** -0.5)
    bhh = rnd((3 * H,), torch.float32, 33, scale=0.1)
    for h0 in (None, rnd((S, H), torch.float32, 34, scale=0.5)):
        hs_w, g_w, hn_w = ref.gru_scan_fwd(gi, whh.t().contiguous(), bhh, h0)
        hs_g, g_g, hn_g = hip.gru_scan_fwd(dev(gi), dev(whh.t().contiguous()), dev(bhh), dev(h0))
        assert last_kernel(hip) == 'gru_scan_wide_fwd_kernel'
        close(hs_g, hs_w, torch.float32, 'gru hs')
        close(g_g, g_w, torch.float32, 'gru gates')
        close(hn_g, hn_w, torch.float32, 'gru hn_pre')
        dhs = rnd((S, T, H), torch.float32, 35)
        w_ = ref.gru_scan_bwd(dhs, whh, h0, hs_w, g_w, hn_w, h0 is not None)
        g_ = hip.gru_scan_bwd(dev(dhs), dev(whh), dev(h0), dev(hs_w), dev(g_w), dev(hn_w), h0 is not None)
        assert last_kernel(hip) == 'gru_scan_wide_bwd_kernel'
        close(g_[0], w_[0], torch.float32, 'gru dgi')
        close(g_[1], w_[1], torch.float32, 'gru dgh')
        if h0 is not None:
            close(g_[2], w_[2], torch.float32, 'gru dh0')
        else:
            assert g_[2] is None


@pytest.mark.parametrize('S', [5, 16, 37])
@pytest.mark.parametrize('H', [272, 512, 1024])
def test_wide_rnn_and_lstm_scans(hip, ref, H, S):
    T = 7
    for G, name in ((1, 'rnn'), (4, 'lstm')):
        gi = rnd((S, T, G * H), torch.float32, 36)
        whh = rnd((G * H, H), torch.float32, 37, scale=H ** -0.5)
        bhh = rnd((G * H,), torch.float32, 38, scale=0.1)
        for with0 in (False, True):
            h0 = rnd((S, H), torch.float32, 39, scale=0.5) if with0 else None
            c0 = rnd((S, H), torch.float32, 40, scale=0.5) if with0 else None
            dhs = rnd((S, T, H), torch.float32, 41)
            if G == 1:
                hs_w = ref.rnn_scan_fwd(gi, whh.t().contiguous(), bhh, h0)
                hs_g = hip.rnn_scan_fwd(dev(gi), dev(whh.t().contiguous()), dev(bhh), dev(h0))
                assert last_kernel(hip) == 'rnn_scan_wide_fwd_kernel'
                close(hs_g, hs_w, torch.float32, 'rnn hs')
                w_ = ref.rnn_scan_bwd(dhs, whh, hs_w, with0)
                g_ = hip.rnn_scan_bwd(dev(dhs), dev(whh), dev(hs_w), with0)
            else:
                hs_w, cs_w, g_w = ref.lstm_scan_fwd(gi, whh.t().contiguous(), bhh, h0, c0)
                hs_g, cs_g, g_g = hip.lstm_scan_fwd(dev(gi), dev(whh.t().contiguous()), dev(bhh), dev(h0), dev(c0))
                assert last_kernel(hip) == 'lstm_scan_wide_fwd_kernel'
                close(hs_g, hs_w, torch.float32, 'lstm hs')
                close(cs_g, cs_w, torch.float32, 'lstm cs')
                close(g_g, g_w, torch.float32, 'lstm gates')
                dcs = rnd((S, T, H), torch.float32, 42) if with0 else None
                w_ = ref.lstm_scan_bwd(dhs, dcs, whh, c0, hs_w, cs_w, g_w, with0)
                g_ = hip.lstm_scan_bwd(dev(dhs), dev(dcs), dev(whh), dev(c0), dev(hs_w), dev(cs_w), dev(g_w), with0)
            assert last_kernel(hip) == name + '_scan_wide_bwd_kernel'
            assert len(g_) == len(w_)
            for a, b, what in zip(g_, w_, ('dpre', 'dh0', 'dc0')):
                assert (a is None) == (b is None), what
                if b is not None:
                    close(a, b, torch.float32, '%s backward %s' % (name, what))


# ------------------------------------------------------------------------------------------------ 5. unchanged dispatch
def test_narrow_scans_keep_their_kernels(hip):
    """The scans for H <= 256 do not take part in the eve_last_kernel() attribution (recorded on the parent commit: the name
    reads '' in a fresh process after every one of the six entry points at H = 128 and H = 96, and whatever an earlier
    marked launch left otherwise); the wide family does.  So after a wide launch, narrow launches leave the name alone."""
    def scans(H):
        S, T = 3, 4
        for G in (3, 1, 4):
            gi = dev(rnd((S, T, G * H), torch.float32, 51))
            whh = dev(rnd((G * H, H), torch.float32, 52, scale=H ** -0.5))
            bhh = dev(rnd((G * H,), torch.float32, 53, scale=0.1))
            wt = whh.t().contiguous()
            if G == 3:
                hs, gates, hn = hip.gru_scan_fwd(gi, wt, bhh, None)
                yield 'gru fwd'
                hip.gru_scan_bwd(torch.ones_like(hs), whh, None, hs, gates, hn, False)
                yield 'gru bwd'
            elif G == 1:
                hs = hip.rnn_scan_fwd(gi, wt, bhh, None)
                yield 'rnn fwd'
                hip.rnn_scan_bwd(torch.ones_like(hs), whh, hs, False)
                yield 'rnn bwd'
            else:
                hs, cs, gates = hip.lstm_scan_fwd(gi, wt, bhh, None, None)
                yield 'lstm fwd'
                hip.lstm_scan_bwd(torch.ones_like(hs), None, whh, None, hs, cs, gates, False)
                yield 'lstm bwd'

    wide = [last_kernel(hip) for _ in scans(512)]
    assert wide == ['gru_scan_wide_fwd_kernel', 'gru_scan_wide_bwd_kernel', 'rnn_scan_wide_fwd_kernel', 'rnn_scan_wide_bwd_kernel',
                    'lstm_scan_wide_fwd_kernel', 'lstm_scan_wide_bwd_kernel']
    for H in (128, 96, 256):
        for what in scans(H):
            assert last_kernel(hip) == wide[-1], 'H = %d %s marked %r' % (H, what, last_kernel(hip))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 6. the limit
@pytest.mark.parametrize('H', [1040, 264])
def test_unsupported_widths_raise(hip, H):
    S, T = 2, 3
    hip.linear_fwd(torch.ones((4, 16), device='cuda'), torch.ones((16, 16), device='cuda'), None, 0)    # a marked launch that is no scan
    before = last_kernel(hip)
    assert before.startswith('linear_')
    for G, fwd in ((3, hip.gru_scan_fwd), (1, hip.rnn_scan_fwd), (4, hip.lstm_scan_fwd)):
        gi = torch.zeros((S, T, G * H), device='cuda')
        args = (gi, torch.zeros((H, G * H), device='cuda'), torch.zeros((G * H,), device='cuda'), None) + ((None,) if G == 4 else ())
        with pytest.raises(RuntimeError) as e:
            fwd(*args)
        assert WIDTH_RULE in str(e.value), str(e.value)
    z = lambda *s: torch.zeros(s, device='cuda')
    with pytest.raises(RuntimeError) as e:
        hip.gru_scan_bwd(z(S, T, H), z(3 * H, H), None, z(S, T, H), z(S, T, 3 * H), z(S, T, H), False)
    assert WIDTH_RULE in str(e.value)
    with pytest.raises(RuntimeError) as e:
        hip.rnn_scan_bwd(z(S, T, H), z(H, H), z(S, T, H), False)
    assert WIDTH_RULE in str(e.value)
    with pytest.raises(RuntimeError) as e:
        hip.lstm_scan_bwd(z(S, T, H), None, z(4 * H, H), None, z(S, T, H), z(S, T, H), z(S, T, 4 * H), False)
    assert WIDTH_RULE in str(e.value)
    assert last_kernel(hip) == before           # no scan was launched
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. module level
import os  # noqa: E402

import eve_amd  # noqa: E402
from oracle import detweights, sequence  # noqa: E402
from oracle.config import OracleConfig  # noqa: E402
from oracle.eye_net import EyeNet as OracleEyeNet  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAZE_TOL = 1e-4          # rad: the project's parity statement; test_gpu_eyenet.py holds the 128-wide variants' other
                         # outputs and states to the same figure (check_eyenet_variant(tol=GAZE_TOL))
WIDE = 512
CELLS = [dict(eye_net_rnn_type='GRU'), dict(eye_net_rnn_type='RNN'), dict(eye_net_rnn_type='LSTM'),
         dict(eye_net_rnn_type='GRU', eye_net_rnn_num_cells=2)]


def _id(over):
    return '-'.join(str(v) for v in over.values())


def to_dev(batch):
    return {k: v.cuda() for k, v in batch.items()}


def wide_net(over, dtype, seed=0):
    over = dict(over, eye_net_rnn_num_features=WIDE)
    cfg = eve_amd.reset_standalone_config()
    cfg.import_dict(dict(over, batch_size=16, weight_decay=0.005, base_learning_rate=0.001))
    net = eve_amd.EyeNet()
    net.compute_dtype = dtype
    detweights.fill_module(net, seed=seed)
    return net.cuda(), OracleConfig(batch_size=16, weight_decay=0.005, base_learning_rate=0.001, **over)


@pytest.mark.parametrize('over', CELLS, ids=_id)
def test_wide_eyenet_matches_the_oracle(hip, over):
    """EyeNet with 512-wide cells, float32, B = 2, T = 4, against the CPU oracle built from the same config: every output the
    oracle stacks (gaze, pupil sizes, the states of every step -- the last one is the final state) and the parameter gradients
    of eyenet_losses, by the criterion of test_sequence_matches_cpu_oracle_other_shape_and_grads."""
    net, ocfg = wide_net(over, torch.float32)
    ref = detweights.fill_module(OracleEyeNet(ocfg), seed=0)
    assert tuple(ref.rnn_cells[0].weight_hh.shape) == ({'GRU': 3, 'RNN': 1, 'LSTM': 4}[over['eye_net_rnn_type']] * WIDE, WIDE)
    batch = detweights.eyenet_batch(2, 4, seed=4, invalid_fraction=0.3)
    rout = sequence.eyenet_sequence(ref, batch)
    sequence.eyenet_losses(rout, batch, ocfg)['full_loss'].backward()
    dbatch = to_dev(batch)
    out = net.forward_sequence(dbatch)
    assert last_kernel(hip) != '' and '_scan_wide_fwd_kernel' in hip_scan_names(net, dbatch)
    report = {}
    for k in rout:
        report[k] = float((out[k].detach().cpu() - rout[k].detach()).abs().max())
    print('wide EyeNet %s vs oracle: %s' % (over, ', '.join('%s %.2e' % kv for kv in sorted(report.items()))))
    assert {'left_g_initial', 'right_g_initial', 'left_pupil_size', 'right_pupil_size'} <= set(report)
    if over['eye_net_rnn_type'] != 'LSTM':
        assert 'left_eye_rnn_states_0' in report and tuple(rout['left_eye_rnn_states_0'].shape) == (2, 4, WIDE)
    for k, e in report.items():
        assert e < GAZE_TOL, (k, e)
    if over['eye_net_rnn_type'] == 'LSTM':          # the oracle's stack keeps tensors only: the (h, c) pairs step by step
        prev = None
        for t in range(4):
            so = {}
            si = {k: v[:, t] for k, v in batch.items()}
            with torch.no_grad():
                ref(si, so, side='left', previous_output_dict=prev)
                ref(si, so, side='right', previous_output_dict=prev)
            prev = so
        for side in ('left', 'right'):
            for j in range(2):
                e = float((out[side + '_eye_rnn_states_0'][j][:, -1].detach().cpu() - prev[side + '_eye_rnn_states_0'][j]).abs().max())
                assert e < GAZE_TOL, (side, j, e)
    sequence.eyenet_losses(out, dbatch, ocfg)['full_loss'].backward()
    rp = dict(ref.named_parameters())
    for n, p in net.named_parameters():
        a, b = p.grad.cpu().double(), rp[n].grad.double()
        err = float((a - b).norm() / (b.norm() + 1e-12))
        assert err <= 2e-2 or float((a - b).abs().max()) < 1e-5, '%s: rel L2 %.3e' % (n, err)
    eve_amd.reset_standalone_config()


def hip_scan_names(net, dbatch):
    """The kernel names the library reports while `net` evaluates the clip (the attribution is per launch: collect it around
    every scan call of the default kernels)."""
    from eve_amd.kernels import default_kernels
    k = default_kernels()
    seen = []
    names = ('gru_scan_fwd', 'rnn_scan_fwd', 'lstm_scan_fwd')
    saved = {n: getattr(k, n) for n in names}

    def wrap(fn):
        def run(*a, **kw):
            r = fn(*a, **kw)
            seen.append(k.lib.eve_last_kernel().decode())
            return r
        return run
    try:
        for n in names:
            setattr(k, n, wrap(saved[n]))
        with torch.no_grad():
            net.forward_sequence(dbatch)
    finally:
        for n in names:
            delattr(k, n)
    return ' '.join(seen)


# ------------------------------------------------------------------------------------------------ 3. bf16 trunk + wide tail
def test_wide_eyenet_trains_in_bf16_eager_and_graph():
    """One train step through train.eyenet_trainer with a bf16 trunk and the 512-wide float32 tail, eager and as a replayed
    hipGraph: finite loss, every parameter moves, and the two agree by the bf16 criterion of
    test_eve_trainer_hipgraph_replay_equals_eager_steps (losses within 2e-2, the step's gradient within 2e-2 relative)."""
    from eve_amd import train
    batch = to_dev(detweights.eyenet_batch(2, 4, seed=11, invalid_fraction=0.1))
    runs = {}
    for mode in ('eager', 'graph'):
        net, _ = wide_net(dict(eye_net_rnn_type='GRU'), torch.bfloat16)
        net.train()
        before = {n: p.detach().clone() for n, p in net.named_parameters()}
        tr = train.eyenet_trainer(net, net.config, use_graph=(mode == 'graph'))
        terms = tr.step(batch)
        torch.cuda.synchronize()
        assert net.last_tail_path == 'layers'
        loss = float(terms['full_loss'].detach())
        assert loss == loss and abs(loss) != float('inf'), loss
        assert tr.optimizer_state()['steps_taken'] == 1
        same = [n for n, p in net.named_parameters() if torch.equal(p.detach(), before[n])]
        assert not same, 'parameters the step left unchanged: %s' % same
        assert all(torch.isfinite(p).all() for p in net.parameters())
        runs[mode] = ({k: float(terms[k].detach()) for k in ('full_loss', 'loss_ang_left_g_initial', 'loss_l1_right_pupil_size')},
                      tr.fp.grad.clone())
    a, b = runs['eager'][0], runs['graph'][0]
    for k in a:
        assert abs(a[k] - b[k]) <= 2e-2 * max(1.0, abs(a[k])), (k, a[k], b[k])
    ge, gg = runs['eager'][1], runs['graph'][1]
    assert float((ge - gg).norm() / ge.norm()) < 2e-2
    eve_amd.reset_standalone_config()


# ------------------------------------------------------------------------------------------------ 4. streaming
STREAM_KEYS = ('left_eye_patch', 'right_eye_patch', 'left_h', 'right_h', 'left_o', 'right_o', 'left_R', 'right_R', 'head_R',
               'camera_transformation', 'inv_camera_transformation', 'pixels_per_millimeter', 'millimeters_per_pixel', 'screen_frame')


def test_wide_stream_is_bit_identical_to_the_whole_clip():
    """EVEStream on a 512-wide GRU model, float32: 8 frames in chunks of 3, 1, 4 equal the whole-clip eval pass bit for bit
    (the layer-by-layer tail's contract), and get_state / set_state carry the wide state."""
    cfg = eve_amd.reset_standalone_config()
    cfg.import_json(os.path.join(REPO, 'configs', 'eye_net.json'))
    cfg.import_dict(dict(eye_net_load_pretrained=False, eye_net_rnn_num_features=WIDE))
    model = eve_amd.EVE(output_predictions=True)
    model.eye_net.compute_dtype = torch.float32
    detweights.fill_module(model.eye_net, 0)
    model = model.cuda().eval()
    b = detweights.eve_batch(2, 8, seed=4)
    d = {k: b[k].cuda() for k in STREAM_KEYS if k in b}
    full = {k: v.cuda() for k, v in b.items()}
    with torch.no_grad():
        whole = model(dict(full))
        whole.update({k: v for k, v in model.eye_net.forward_sequence(d).items() if k.endswith('_g_initial') or k.endswith('_pupil_size')})

    def chunks(stream, sizes, t0=0):
        outs = []
        for n in sizes:
            outs.append({k: v.clone() for k, v in stream.step({k: v[:, t0:t0 + n].contiguous() for k, v in d.items()}).items()})
            t0 += n
        return {k: torch.cat([o[k] for o in outs], dim=1) for k in outs[0]}

    s = eve_amd.EVEStream(model, 2)
    assert [tuple(t.shape) for t in s._eye] == [(4, WIDE)]
    got = chunks(s, (3, 1, 4))
    compared = [k for k in got if k in whole]
    assert {'left_g_initial', 'right_g_initial', 'g_initial', 'PoG_px_initial'} <= set(compared), compared
    for k in compared:
        assert torch.equal(got[k], whole[k]), (k, float((got[k].float() - whole[k].float()).abs().max()))
    # round trip: the state after 4 frames, loaded into a second stream, continues identically
    a = eve_amd.EVEStream(model, 2)
    chunks(a, (3, 1))
    st = a.get_state()
    assert tuple(st['left_eye_rnn_states_0'].shape) == (2, WIDE) and st['left_eye_rnn_states_0'].dtype == torch.float32
    c = eve_amd.EVEStream(model, 2)
    c.set_state(st)
    for k, v in c.get_state().items():
        assert torch.equal(v, st[k]), k
    rest_a, rest_c = chunks(a, (4,), 4), chunks(c, (4,), 4)
    for k in rest_a:
        assert torch.equal(rest_a[k], rest_c[k]), k
        if k in whole:
            assert torch.equal(rest_c[k], whole[k][:, 4:]), k
    eve_amd.reset_standalone_config()
