"""GPU: gradients with respect to the networks' float INPUTS (eye patches, head pose, screen frames), as every nn.Module of the
reference returns them: the stem's data-gradient kernel (eve_stem_dgrad) against float64, the clip path, the per-step
contract and EVE end to end against the CPU oracle evaluated in float64, the 16-bit stem routes, frozen weights, and the
unchanged default backward."""
import os

import numpy as np
import pytest
import torch

import eve_amd
from eve_amd import kernels
from oracle import detweights, sequence
from oracle.config import OracleConfig

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


# Float32 patch gradients against the float64 oracle, relative L2.  Measured on the MI355X: 1.7e-3 (clip path, left patch) and
# 1.0e-3 (EVE, left patch), where the per-step contract (2 frames) meets 1e-4 and the float32 oracle is 5e-6 away.  The deviation
# is spread over the image, not a few flipped max-pool windows, and the torch-CPU float32 stand-in of tests/fake_kernels.py --
# whose stem data gradient is exact float64 -- shows the same size (1.1e-3 left, 7.3e-3 right): it arises upstream of the new
# kernel.  Our reading: InstanceNorm after conv1 makes the loss invariant to the brightness and contrast of each patch, so the
# true patch gradient is a small residual of large terms, and the float32 InstanceNorm backward's cancellation shows in it
# (the CPU oracle's ATen reductions accumulate float32 in double).  Not proven; the bound records the measurement.
F32_PATCH_L2 = 1e-2


def make_eyenet(dtype):
    cfg = eve_amd.reset_standalone_config()
    cfg.import_dict({'batch_size': 16, 'weight_decay': 0.005, 'base_learning_rate': 0.001})
    net = eve_amd.EyeNet()
    net.compute_dtype = dtype
    detweights.fill_module(net, seed=0)
    return net.cuda()


def eye_batch(B, T, size=128, seed=3):
    b = {k: v.cuda() for k, v in detweights.eyenet_batch(B, T, size=size, seed=seed).items()}
    for k in ('left_eye_patch', 'right_eye_patch', 'left_h', 'right_h'):
        b[k] = b[k].clone().requires_grad_(True)
    return b


def projection_loss(out, seed, keys=('left_g_initial', 'right_g_initial', 'left_pupil_size', 'right_pupil_size')):
    """Seeded random projections of the predictions: every output element carries a distinct weight."""
    g = torch.Generator().manual_seed(seed)
    total = 0.0
    for k in keys:
        v = out[k]
        w = torch.randn(v.shape, generator=g, dtype=torch.float64).to(v.device, v.dtype)
        total = total + (v * w).sum()
    return total


INPUTS = ('left_eye_patch', 'right_eye_patch', 'left_h', 'right_h')


# ---------------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize('size,N,border', [(128, 1, False), (128, 3, False), (256, 1, False), (256, 3, False), (128, 3, True)])
def test_stem_dgrad_kernel_matches_float64(dtype, size, N, border):
    """eve_stem_dgrad on exact (dtype-representable) inputs against torch.nn.grad.conv2d_input in float64 on the CPU; `border`:
    dconv non-zero only on its outer rows and columns, where the transposed convolution reads the padding taps."""
    k = kernels.default_kernels()
    g = torch.Generator().manual_seed(size + 7 * N + int(border))
    w = torch.randn((64, 3, 7, 7), generator=g).to(dtype).float()
    dconv = torch.randn((N, size // 2, size // 2, 64), generator=g).to(dtype)
    if border:
        inner = torch.zeros_like(dconv)
        inner[:, 1:-1, 1:-1] = dconv[:, 1:-1, 1:-1]
        dconv = dconv - inner
    got = k.stem_dgrad(dconv.cuda(), k.stem_dgrad_pack(w.cuda(), dtype), 3)
    torch.cuda.synchronize()
    ref = torch.nn.grad.conv2d_input((N, 3, size, size), w.double(), dconv.double().permute(0, 3, 1, 2), stride=2, padding=3)
    assert got.dtype == torch.float32 and tuple(got.shape) == (N, 3, size, size)
    err = got.double().cpu() - ref
    assert rel_l2(got, ref) <= 1e-5, rel_l2(got, ref)
    assert float(err.abs().max()) <= 1e-5 * float(ref.abs().max()), (float(err.abs().max()), float(ref.abs().max()))


# ---------------------------------------------------------------------------------------------------- 2. clip path, float32
def _oracle_eyenet_input_grads(B, T, seed, loss_seed, dtype=torch.float64):
    from oracle.eye_net import EyeNet as OracleEyeNet
    torch.set_default_dtype(dtype)
    try:
        ref = detweights.fill_module(OracleEyeNet(OracleConfig(batch_size=16, weight_decay=0.005, base_learning_rate=0.001)),
                                     seed=0).to(dtype)
        b = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in detweights.eyenet_batch(B, T, seed=seed).items()}
        for k in INPUTS:
            b[k].requires_grad_(True)
        out = sequence.eyenet_sequence(ref, b)
        grads = torch.autograd.grad(projection_loss(out, loss_seed), [b[k] for k in INPUTS])
        return dict(zip(INPUTS, grads))
    finally:
        torch.set_default_dtype(torch.float32)


def test_clip_path_input_gradients_match_the_float64_oracle():
    """EyeNet.forward_sequence, float32, B = 2, T = 3: d/d(patches) and d/d(head pose) of seeded projections of g_initial and
    pupil_size, against oracle/eye_net.py evaluated in float64 under autograd, per full tensor (bound: F32_PATCH_L2 above)."""
    net = make_eyenet(torch.float32)
    batch = eye_batch(2, 3, seed=3)
    out = net.forward_sequence(batch)
    got = dict(zip(INPUTS, torch.autograd.grad(projection_loss(out, 11), [batch[k] for k in INPUTS])))
    want = _oracle_eyenet_input_grads(2, 3, seed=3, loss_seed=11)
    ref32 = _oracle_eyenet_input_grads(2, 3, seed=3, loss_seed=11, dtype=torch.float32)
    for k in INPUTS:
        assert got[k].shape == batch[k].shape
        e, noise = rel_l2(got[k], want[k]), rel_l2(ref32[k], want[k])
        print('%s: relative L2 %.2e from the float64 oracle (the oracle in float32: %.2e)' % (k, e, noise))
        assert e <= max(F32_PATCH_L2 if k.endswith('patch') else 1e-4, 4.0 * noise), (k, e, noise)


def test_per_step_contract_returns_the_patch_gradient():
    """The reference's per-step EyeNet.forward (one eye, one frame) in float32: the patch and head-pose gradients equal the
    float64 oracle's per-step evaluation within 1e-4 relative L2."""
    from oracle.eye_net import EyeNet as OracleEyeNet
    net = make_eyenet(torch.float32)
    batch = eye_batch(2, 1, seed=4)
    sub = {k: v[:, 0] for k, v in batch.items()}
    out = {}
    net(sub, out, side='left')
    got = torch.autograd.grad(projection_loss(out, 5, ('left_g_initial', 'left_pupil_size')), [sub['left_eye_patch'], sub['left_h']])
    torch.set_default_dtype(torch.float64)
    try:
        ref = detweights.fill_module(OracleEyeNet(OracleConfig(batch_size=16, weight_decay=0.005, base_learning_rate=0.001)),
                                     seed=0).double()
        b = {k: (v[:, 0].double() if v.is_floating_point() else v[:, 0]) for k, v in detweights.eyenet_batch(2, 1, seed=4).items()}
        for k in ('left_eye_patch', 'left_h'):
            b[k].requires_grad_(True)
        rout = {}
        ref(b, rout, side='left')
        want = torch.autograd.grad(projection_loss(rout, 5, ('left_g_initial', 'left_pupil_size')), [b['left_eye_patch'], b['left_h']])
    finally:
        torch.set_default_dtype(torch.float32)
    for name, g_, w_ in zip(('patch', 'h'), got, want):
        assert rel_l2(g_, w_) <= 1e-4, (name, rel_l2(g_, w_))


# ---------------------------------------------------------------------------------------------------- 3. EVE end to end
def test_eve_full_loss_patch_gradients_match_the_float64_oracle():
    """eve_amd.EVE on configs/eye_net.json (EyeNet trainable), float32, B = 2, T = 3: d(full_loss)/d(left / right patch) against
    the oracle's eve_forward + full_loss evaluated in float64 (bound: F32_PATCH_L2 above)."""
    from oracle import eve as oracle_eve
    from oracle.eye_net import EyeNet as OracleEyeNet
    json_path = os.path.join(REPO, 'configs', 'eye_net.json')
    cfg = eve_amd.reset_standalone_config()
    cfg.import_json(json_path)
    cfg.import_dict(dict(eye_net_load_pretrained=False))
    model = eve_amd.EVE(output_predictions=True)
    model.eye_net.compute_dtype = torch.float32
    detweights.fill_module(model.eye_net, 0)
    model = model.cuda().train()
    batch = detweights.eve_batch(2, 3, seed=13, invalid_fraction=0.2, with_screen=False)
    dev = {k: v.cuda() for k, v in batch.items()}
    for k in ('left_eye_patch', 'right_eye_patch'):
        dev[k] = dev[k].clone().requires_grad_(True)
    np.random.seed(2)
    got = model({'s': dev}, current_epoch=0.0)
    g = torch.autograd.grad(got['full_loss'], [dev['left_eye_patch'], dev['right_eye_patch']])
    ocfg = OracleConfig(json_path, eye_net_load_pretrained=False)
    w, loss = {}, {}
    for dt in (torch.float32, torch.float64):
        torch.set_default_dtype(dt)
        try:
            oeye = detweights.fill_module(OracleEyeNet(ocfg), 0).to(dt)
            bo = {k: (v.to(dt) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in batch.items()}
            for k in ('left_eye_patch', 'right_eye_patch'):
                bo[k].requires_grad_(True)
            np.random.seed(2)
            want, _, _ = oracle_eve.eve_forward(oeye, None, dict(bo), ocfg, True)
            w[dt] = torch.autograd.grad(want['full_loss'], [bo['left_eye_patch'], bo['right_eye_patch']])
            loss[dt] = float(want['full_loss'].detach())
        finally:
            torch.set_default_dtype(torch.float32)
    assert abs(float(got['full_loss'].detach()) - loss[torch.float64]) <= 1e-4 * abs(loss[torch.float64])
    for side, a, b, b32 in zip(('left', 'right'), g, w[torch.float64], w[torch.float32]):
        e, noise = rel_l2(a, b), rel_l2(b32, b)
        print('%s patch: relative L2 %.2e from the float64 oracle (the oracle in float32: %.2e)' % (side, e, noise))
        assert e <= max(F32_PATCH_L2, 4.0 * noise), (side, e, noise)


# ---------------------------------------------------------------------------------------------------- 4. 16-bit stem routes
class _Record(object):
    """The HipKernels instance with every method call recorded by name (and stem_dgrad's operands kept)."""

    def __init__(self, k):
        self._k, self.calls, self.dgrad = k, [], []

    def __getattr__(self, name):
        v = getattr(self._k, name)
        if not callable(v):
            return v

        def call(*a, **kw):
            self.calls.append(name)
            r = v(*a, **kw)
            if name == 'stem_dgrad':
                self.dgrad.append((a[0].detach().clone(), a[1].detach().clone(), r.detach().clone()))
            return r
        return call


@pytest.fixture()
def recorder():
    rec = _Record(kernels.default_kernels())
    kernels.set_default_kernels(rec)
    yield rec
    kernels.set_default_kernels(None)


# Patch gradient of the 16-bit routes against the float32 path, relative L2, measured on the MI355X (left patch): bf16 fused route
# 128^2 4.5e-1, f16 dedicated stem conv 256^2 1.7e-1.  Far outside the 2e-2 envelope of the 16-bit WEIGHT gradients: a pixel's
# gradient follows one chain of max-pool / ReLU decisions, and 16-bit activations flip many of them (the weight gradients sum
# over all pixels and average it out).  The kernel's own share is separated below (1e-5 against float64 on the same dconv).
HALF_BOUNDS = {(torch.bfloat16, 128): 0.6, (torch.float16, 256): 0.25}


@pytest.mark.parametrize('dtype,size,route', [(torch.bfloat16, 128, 'stem_bwd_dx'), (torch.float16, 256, 'stem7x7s2_fwd')])
def test_half_precision_stem_routes_return_the_patch_gradient(recorder, dtype, size, route):
    """bf16 through the fused stem (128 wide) and f16 through the dedicated stem conv (256 wide), B = 1, T = 2: the patch gradient
    against the float32 HIP path on the same weights (bound: HALF_BOUNDS, the measured deviation with margin),
    and the kernel's share separated from the rounding upstream: stem_dgrad's output against its own float64 evaluation on the
    16-bit d(conv1 out) it was given."""
    res = {}
    for dt in (torch.float32, dtype):
        net = make_eyenet(dt)
        batch = eye_batch(1, 2, size=size, seed=6)
        recorder.calls.clear()
        recorder.dgrad.clear()
        out = net.forward_sequence(batch)
        res[dt] = torch.autograd.grad(projection_loss(out, 3), [batch['left_eye_patch'], batch['right_eye_patch']])
        torch.cuda.synchronize()
        assert recorder.calls.count('stem_dgrad') == 1
    assert route in recorder.calls
    dconv, wp, dx = recorder.dgrad[0]
    w = net.cnn_layers.conv1.weight.detach().to(dtype).double().cpu()
    N, OH, OW, _ = dconv.shape
    ref = torch.nn.grad.conv2d_input((N, 3, 2 * OH, 2 * OW), w, dconv.double().cpu().permute(0, 3, 1, 2), stride=2, padding=3)
    assert dconv.dtype == dtype and rel_l2(dx, ref) <= 1e-5, rel_l2(dx, ref)
    for side, a, b in zip(('left', 'right'), res[dtype], res[torch.float32]):
        assert a.dtype == torch.float32
        e = rel_l2(a, b)
        print('%s %s %d^2 %s patch: relative L2 %.2e from the float32 path' % (route, dtype, size, side, e))
        assert e <= HALF_BOUNDS[(dtype, size)], (side, e)


# ---------------------------------------------------------------------------------------------------- 5. frozen weights
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_frozen_weights_give_the_same_patch_gradient_and_no_parameter_grad(dtype):
    """The gaze-loss use: eye_net.requires_grad_(False) and patches that require grad.  The patch gradient equals the trainable
    network's bit for bit; no parameter receives a .grad."""
    res = {}
    for frozen in (False, True):
        net = make_eyenet(dtype)
        net.requires_grad_(not frozen)
        batch = eye_batch(1, 2, seed=8)
        out = net.forward_sequence(batch)
        res[frozen] = torch.autograd.grad(projection_loss(out, 4), [batch['left_eye_patch'], batch['right_eye_patch']])
        if frozen:
            assert all(p.grad is None for p in net.parameters())
    for a, b in zip(res[False], res[True]):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------- 6. unchanged default
def test_default_backward_runs_the_fused_stem_weight_gradient_only(recorder):
    """Patches that do not require grad (the training step): the fused stem backward + weight gradient in one launch, as before;
    no d(conv1 out) tensor and no data-gradient launch.  With patch gradients wanted: stem_bwd_dx feeds stem_wgrad and
    stem_dgrad."""
    net = make_eyenet(torch.bfloat16)
    batch = {k: v.cuda() for k, v in detweights.eyenet_batch(1, 2, seed=9).items()}
    projection_loss(net.forward_sequence(batch), 1).backward()
    torch.cuda.synchronize()
    assert 'stem_bwd_wgrad' in recorder.calls
    assert 'stem_dgrad' not in recorder.calls and 'stem_bwd_dx' not in recorder.calls and 'stem_dgrad_pack' not in recorder.calls
    recorder.calls.clear()
    net.zero_grad(set_to_none=True)
    batch['left_eye_patch'].requires_grad_(True)
    projection_loss(net.forward_sequence(batch), 1).backward()
    torch.cuda.synchronize()
    assert 'stem_bwd_wgrad' not in recorder.calls
    assert recorder.calls.count('stem_bwd_dx') == 1 and recorder.calls.count('stem_wgrad') == 1
    assert recorder.calls.count('stem_dgrad') == 1
    assert batch['left_eye_patch'].grad is not None and batch['right_eye_patch'].grad is None


# ---------------------------------------------------------------------------------------------------- 7. RefineNet screen frame
def test_refinenet_screen_frame_gradient_matches_the_float64_oracle():
    """d/d(screen_frame) through RefineNet.forward_sequence (ToNHWCFn and the first convolution's data gradient), float32,
    B = 1, T = 2, against oracle/refine_net.py in float64.  Bound: max(1e-4, 4 x the oracle's own float32 deviation from its
    float64 evaluation) -- the gradient passes softmax(100 h) and the encoder's max-pool decisions, so any float32 evaluation
    is one draw (tests/test_gpu_eve.py, check_grads_against_float64_reference)."""
    from oracle.refine_net import RefineNet as OracleRefineNet
    cfg = eve_amd.reset_standalone_config()
    cfg.import_dict({'load_screen_content': True, 'refine_net_enabled': True, 'refine_net_rnn_type': 'CGRU'})
    net = eve_amd.RefineNet()
    net.compute_dtype = torch.float32
    detweights.fill_module(net, seed=1)
    net = net.cuda()
    rb = detweights.refinenet_batch(1, 2, seed=4)
    hm = rb['heatmap_initial'].cuda()
    sf = rb['screen_frame'].cuda().requires_grad_(True)
    hf, _ = net.forward_sequence(hm, sf)
    gen = torch.Generator().manual_seed(7)
    proj = torch.randn(hf.shape, generator=gen, dtype=torch.float64)
    (got,) = torch.autograd.grad((hf * proj.to(hf.device, hf.dtype)).sum(), [sf])
    ocfg = OracleConfig(load_screen_content=True, refine_net_enabled=True, refine_net_rnn_type='CGRU')
    ref = {}
    for dt in (torch.float32, torch.float64):
        torch.set_default_dtype(dt)
        try:
            net_o = detweights.fill_module(OracleRefineNet(ocfg), 1).to(dt)
            sf_o = rb['screen_frame'].to(dt).requires_grad_(True)
            hf_o, _ = sequence.refinenet_sequence(net_o, rb['heatmap_initial'].to(dt), sf_o)
            (ref[dt],) = torch.autograd.grad((hf_o * proj.to(dt)).sum(), [sf_o])
        finally:
            torch.set_default_dtype(torch.float32)
    want = ref[torch.float64]
    e, noise = rel_l2(got, want), rel_l2(ref[torch.float32], want)
    print('screen_frame gradient: relative L2 %.2e from the float64 oracle (the oracle in float32: %.2e)' % (e, noise))
    assert float(got.abs().sum()) > 0
    assert e <= max(1e-4, 4.0 * noise), (e, noise)
