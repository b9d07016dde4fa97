"""CPU: an EyeNet whose recurrent cells are wider than 256 (eye_net_rnn_num_features = 512) on the host side -- the module
builds with the reference's parameter names and shapes, goes through a checkpoint, takes the per-layer tail, streams with
wide state buffers -- with the torch-CPU stand-in of tests/fake_kernels.py in place of the HIP library.  The kernels
themselves (csrc/recurrent_wide.hip) are checked in test_gpu_wide_scans.py."""
import os

import pytest
import torch

import eve_amd
from eve_amd import kernels
from fake_kernels import FakeKernels
from oracle import detweights, sequence
from oracle.config import OracleConfig
from oracle.eye_net import EyeNet as OracleEyeNet
from test_stream_host import StreamFakes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = 512
CELLS = [dict(eye_net_rnn_type='GRU'), dict(eye_net_rnn_type='RNN'), dict(eye_net_rnn_type='LSTM'),
         dict(eye_net_rnn_type='GRU', eye_net_rnn_num_cells=2)]
GATES = {'GRU': 3, 'RNN': 1, 'LSTM': 4}


def _id(over):
    return '-'.join(str(v) for v in over.values())


@pytest.fixture()
def fake():
    kernels.set_default_kernels(FakeKernels())
    yield
    kernels.set_default_kernels(None)
    eve_amd.reset_standalone_config()


@pytest.fixture()
def stream_fake():
    kernels.set_default_kernels(StreamFakes())           # FakeKernels plus the streaming entry points
    yield
    kernels.set_default_kernels(None)
    eve_amd.reset_standalone_config()


def wide_eyenet(over):
    over = dict(over, eye_net_rnn_num_features=WIDE)
    cfg = eve_amd.reset_standalone_config()
    cfg.import_dict(over)
    return eve_amd.EyeNet(), OracleEyeNet(OracleConfig(**over)), OracleConfig(**over)


@pytest.mark.parametrize('over', CELLS, ids=_id)
def test_wide_eyenet_has_the_reference_layout(over):
    net, ref, _ = wide_eyenet(over)
    a, b = net.state_dict(), ref.state_dict()
    assert list(a.keys()) == list(b.keys())
    assert all(tuple(a[k].shape) == tuple(b[k].shape) for k in a)
    G = GATES[over['eye_net_rnn_type']]
    for i in range(over.get('eye_net_rnn_num_cells', 1)):
        assert tuple(a['rnn_cells.%d.weight_hh' % i].shape) == (G * WIDE, WIDE)
        assert tuple(a['rnn_cells.%d.weight_ih' % i].shape) == (G * WIDE, WIDE)
        assert tuple(a['rnn_cells.%d.bias_hh' % i].shape) == (G * WIDE,)
    assert tuple(a['fc_to_gaze.0.weight'].shape)[1] == WIDE and tuple(a['fc_common.2.weight'].shape)[0] == WIDE


def test_wide_checkpoint_round_trip(tmp_path):
    """eve_amd.checkpoint writes the reference's directory layout; a wide EyeNet comes back with every key and shape, and the
    file loads strictly into a module tree with the reference's cells."""
    from eve_amd import checkpoint
    json_path = os.path.join(REPO, 'configs', 'eye_net.json')
    over = dict(eye_net_load_pretrained=False, eye_net_rnn_num_features=WIDE)
    cfg = eve_amd.reset_standalone_config()
    cfg.import_json(json_path)
    cfg.import_dict(over)
    model = eve_amd.EVE()
    detweights.fill_module(model.eye_net, 3)
    want = {k: v.clone() for k, v in model.state_dict().items()}
    assert tuple(want['eye_net.rnn_cells.0.weight_hh'].shape) == (3 * WIDE, WIDE)
    path = checkpoint.save(model, str(tmp_path), 5)
    part = torch.load(os.path.join(path, 'eye_net.pt'))
    assert tuple(part['eye_net.rnn_cells.0.weight_hh'].shape) == (3 * WIDE, WIDE)
    eve_amd.reset_standalone_config().import_json(json_path)
    eve_amd.get_config().import_dict(over)
    other = eve_amd.EVE()
    assert checkpoint.load(other, path) == 5
    got = other.state_dict()
    assert list(got.keys()) == list(want.keys())
    for k in want:
        assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k

    class ReferenceShaped(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.eye_net = OracleEyeNet(OracleConfig(json_path, **over))
    ReferenceShaped().load_state_dict(part)                  # strict
    eve_amd.reset_standalone_config()


@pytest.mark.parametrize('over', CELLS, ids=_id)
def test_wide_eyenet_takes_the_per_layer_tail_and_matches_the_oracle(fake, over):
    """Both tail selections answer for the wide configuration: the train step's (loss_terms_sequence -> last_tail_path) says
    'layers' with the one-node tail forced ON, the streaming one says not fused with the fused tail asked for; and the
    per-layer path computes what the oracle's cells compute."""
    net, ref, ocfg = wide_eyenet(over)
    detweights.fill_module(net); detweights.fill_module(ref)
    batch = detweights.eyenet_batch(2, 3, seed=5, invalid_fraction=0.2)
    net.tail_loss_node = True
    net.stream_fused_tail = True
    assert not net._stream_tail_fused_ok()
    terms = net.loss_terms_sequence(batch)
    assert net.last_tail_path == 'layers'
    rout = sequence.eyenet_sequence(ref, batch)
    rterms = sequence.eyenet_losses(rout, batch, ocfg)
    for k in ('left_g_initial', 'right_g_initial', 'left_pupil_size', 'right_pupil_size'):
        assert float((terms[k].detach() - rout[k].detach()).abs().max()) < 1e-4, k
    assert abs(float(terms['full_loss'].detach()) - float(rterms['full_loss'].detach())) <= 1e-4 * abs(float(rterms['full_loss'].detach()))
    terms['full_loss'].backward()
    rterms['full_loss'].backward()
    rp = dict(ref.named_parameters())
    for n, p in net.named_parameters():
        if n.startswith('rnn_cells'):
            a, b = p.grad.double(), rp[n].grad.double()
            assert float((a - b).norm()) <= 2e-3 * float(b.norm()) + 1e-7, n


def test_wide_stream_state_buffers(stream_fake):
    """EVEStream on a wide EyeNet: state buffers, get_state / set_state and reset at H = 512."""
    json_path = os.path.join(REPO, 'configs', 'eye_net.json')
    cfg = eve_amd.reset_standalone_config()
    cfg.import_json(json_path)
    cfg.import_dict(dict(eye_net_load_pretrained=False, eye_net_rnn_num_features=WIDE))
    model = eve_amd.EVE(output_predictions=True)
    detweights.fill_module(model.eye_net, 0)
    model.eval()
    b = detweights.eve_batch(2, 5, seed=8)
    keys = ('left_eye_patch', 'right_eye_patch', 'left_h', 'right_h', 'left_o', 'right_o', 'left_R', 'right_R', 'head_R',
            'camera_transformation', 'inv_camera_transformation', 'pixels_per_millimeter', 'millimeters_per_pixel')
    ch = lambda t0, t1: {k: b[k][:, t0:t1].contiguous() for k in keys if k in b}
    s = eve_amd.EVEStream(model, 2, use_graph=False)
    assert [tuple(t.shape) for t in s._eye] == [(4, WIDE)]
    s.step(ch(0, 3))
    st = s.get_state()
    assert tuple(st['left_eye_rnn_states_0'].shape) == (2, WIDE) and tuple(st['right_eye_rnn_states_0'].shape) == (2, WIDE)
    assert float(st['left_eye_rnn_states_0'].abs().max()) > 0
    other = eve_amd.EVEStream(model, 2, use_graph=False)
    other.set_state(st)
    for k, v in other.get_state().items():
        assert torch.equal(v, st[k]), k
    oa, ob = s.step(ch(3, 5)), other.step(ch(3, 5))
    for k in oa:
        assert torch.equal(oa[k], ob[k]), k
    # reset of stream 1: it continues as a fresh stream would, stream 0 is untouched
    again = eve_amd.EVEStream(model, 2, use_graph=False)
    again.set_state(st)
    again.reset([1])
    oc = again.step(ch(3, 5))
    fresh = eve_amd.EVEStream(model, 2, use_graph=False).step(ch(3, 5))
    for k in oc:
        assert torch.equal(oc[k][0], oa[k][0]), k
        assert torch.equal(oc[k][1], fresh[k][1]), k
    assert float(again.get_state()['left_eye_rnn_states_0'][1].abs().max()) > 0
