"""CPU: the autograd wiring of the input gradients (eye patches, head pose) through every stem route, with the torch-CPU stand-in
of tests/fake_kernels.py extended by the stem's data gradient; the GPU suite (test_gpu_input_grad.py) checks the HIP kernel."""
import pytest
import torch

import eve_amd
from eve_amd import kernels
from fake_kernels import FakeKernels, nchw
from oracle import detweights, sequence
from oracle.config import OracleConfig
from oracle.eye_net import EyeNet as OracleEyeNet


class InputGradFakes(FakeKernels):
    """FakeKernels plus include/eve_hip.h eve_stem_dgrad_pack / eve_stem_dgrad (the fake's packed filter is the rounded OIHW
    weight itself)."""

    def __init__(self):
        self.calls = []

    def stem_dgrad_pack(self, w_oihw, dtype):
        self.calls.append('stem_dgrad_pack')
        return w_oihw.detach().to(dtype)

    def stem_dgrad(self, dconv, w_packed, C, out=None):
        self.calls.append('stem_dgrad')
        N, OH, OW, _ = dconv.shape
        return torch.nn.grad.conv2d_input((N, C, 2 * OH, 2 * OW), w_packed.double(), nchw(dconv).double(), stride=2,
                                          padding=3).float()


@pytest.fixture()
def fake():
    k = InputGradFakes()
    kernels.set_default_kernels(k)
    yield k
    kernels.set_default_kernels(None)


INPUTS = ('left_eye_patch', 'right_eye_patch', 'left_h', 'right_h')


def make_net(dtype):
    cfg = eve_amd.reset_standalone_config()
    cfg.import_dict({'batch_size': 16, 'weight_decay': 0.005, 'base_learning_rate': 0.001})
    net = eve_amd.EyeNet()
    net.compute_dtype = dtype
    return detweights.fill_module(net, seed=0)


def batch_with_grad(B, T, size=128, seed=1):
    b = detweights.eyenet_batch(B, T, size=size, seed=seed)
    for k in INPUTS:
        b[k].requires_grad_(True)
    return b


def loss_of(out):
    g = torch.Generator().manual_seed(0)
    return sum((out[k] * torch.randn(out[k].shape, generator=g)).sum()
               for k in ('left_g_initial', 'right_g_initial', 'left_pupil_size', 'right_pupil_size'))


def test_clip_path_float32_input_gradients_match_the_oracle(fake):
    """Without the stem's data gradient the patches are not in the graph (autograd.grad raises); with it, the float32 clip path
    returns d/d(patches) and d/d(head pose) equal to the oracle's."""
    net = make_net(torch.float32)
    b = batch_with_grad(1, 2)
    got = torch.autograd.grad(loss_of(net.forward_sequence(b)), [b[k] for k in INPUTS])
    ref = detweights.fill_module(OracleEyeNet(OracleConfig(batch_size=16, weight_decay=0.005, base_learning_rate=0.001)), seed=0)
    rb = batch_with_grad(1, 2)
    want = torch.autograd.grad(loss_of(sequence.eyenet_sequence(ref, rb)), [rb[k] for k in INPUTS])
    for k, g, w in zip(INPUTS, got, want):
        assert float((g - w).norm() / w.norm()) < 1e-3, k
    assert fake.calls.count('stem_dgrad') == 1


@pytest.mark.parametrize('dtype,size', [(torch.bfloat16, 128), (torch.float16, 256), (torch.bfloat16, 96)])
def test_every_half_precision_stem_route_passes_the_gradient(fake, dtype, size):
    """Fused stem (128 wide), dedicated stem conv (256 wide) and the generic convolution (other widths): one stem_dgrad launch
    each, and a float32 NCHW gradient for both patches."""
    net = make_net(dtype)
    b = batch_with_grad(1, 2, size=size)
    got = torch.autograd.grad(loss_of(net.forward_sequence(b)), [b['left_eye_patch'], b['right_eye_patch']])
    for g in got:
        assert g.dtype == torch.float32 and g.shape == b['left_eye_patch'].shape and float(g.abs().sum()) > 0
    assert fake.calls.count('stem_dgrad') == 1


def test_frozen_network_passes_the_gradient_and_creates_no_parameter_grad(fake):
    net = make_net(torch.bfloat16)
    net.requires_grad_(False)
    b = batch_with_grad(1, 2)
    loss_of(net.forward_sequence(b)).backward()
    assert all(p.grad is None for p in net.parameters())
    for k in INPUTS:
        assert b[k].grad is not None and float(b[k].grad.abs().sum()) > 0, k


def test_per_step_forward_takes_the_stem_data_gradient(fake):
    net = make_net(torch.float32)
    b = batch_with_grad(2, 1)
    sub = {k: v[:, 0] for k, v in b.items()}
    out = {}
    net(sub, out, side='left')
    (out['left_g_initial'].sum() + out['left_pupil_size'].sum()).backward()
    assert fake.calls.count('stem_dgrad') == 1
    assert b['left_eye_patch'].grad is not None and b['left_h'].grad is not None


def test_no_input_gradient_no_data_gradient_launch(fake):
    net = make_net(torch.bfloat16)
    b = detweights.eyenet_batch(1, 2, seed=1)
    loss_of(net.forward_sequence(b)).backward()
    assert 'stem_dgrad' not in fake.calls and 'stem_dgrad_pack' not in fake.calls
    assert net.cnn_layers.conv1.weight.grad is not None
