"""GPU: the live CLSTM bottleneck behind the eve_amd config key refine_net_clstm_feeds_features -- the differentiable clip scan
(eve_clstm_scan_fwd_train_c / eve_clstm_scan_bwd_c, csrc/cell_scan_f32.hip), the per-frame gate adjoint (eve_clstm_gates_bwd) and
RefineNet / EVEStream / refinenet_trainer on top of them.  With the key off the reference's dead cell (refine_net.py:168-174) is
what runs; that contract is restated here next to the live one.  The CPU side: test_clstm_live_host.py."""
import types

import numpy as np
import pytest
import torch

import eve_amd
import refine_variants as rv
from eve_amd import conv_rnn, losses, ops
from eve_amd.kernels import default_kernels
from oracle import detweights, sequence
from oracle.config import OracleConfig
from test_gpu_kernels import close as close_16bit
from test_gpu_stream import gpu_clip, make_model, maxdiff, run_chunks

pytestmark = pytest.mark.gpu
KEY = 'refine_net_clstm_feeds_features'


def kname(base, C):
    return base if C == 64 else '%s<%d>' % (base, C)


# ------------------------------------------------------------------------------------------------ 1. the clip scan
def restate_clstm(xs, h0, c0, w, bias, dhs_tm, dcs_tm):
    """CLSTMCell (common.py:355-385, gate order in / forget / out / cell) unrolled over T with autograd, in the dtype of its
    operands; layouts are the kernels' (NHWC activations, OHWI bank).  -> every tensor the kernels emit."""
    xs, w, bias = (t.clone().requires_grad_() for t in (xs, w, bias))
    h0l, c0l = (None if t is None else t.clone().requires_grad_() for t in (h0, c0))
    h = torch.zeros_like(xs[:, 0]) if h0l is None else h0l
    c = torch.zeros_like(xs[:, 0]) if c0l is None else c0l
    hs, cs, pres, gates = [], [], [], []
    for t in range(xs.shape[1]):
        pre = rv._conv(torch.cat([xs[:, t], h], -1), w, bias)
        pre.retain_grad()
        i, f, o, g = pre.chunk(4, dim=-1)
        i, f, o, g = torch.sigmoid(i), torch.sigmoid(f), torch.sigmoid(o), torch.tanh(g)
        c = f * c + i * g
        h = o * torch.tanh(c)
        hs.append(h); cs.append(c); pres.append(pre); gates.append(torch.cat([i, f, o, g], -1))
    hs_tm, cs_tm = torch.stack(hs, 0), torch.stack(cs, 0)
    loss = (hs_tm * dhs_tm).sum()
    if dcs_tm is not None:
        loss = loss + (cs_tm * dcs_tm).sum()
    loss.backward()
    det = lambda t: None if t is None else t.detach()
    return dict(hs=det(hs_tm.transpose(0, 1)), cs=det(cs_tm.transpose(0, 1)), gates_tm=det(torch.stack(gates, 0)), cs_tm=det(cs_tm),
                hs_tm=det(hs_tm), dpre=torch.stack([p.grad for p in pres], 0), dxs_tm=xs.grad.transpose(0, 1),
                dh0=None if h0l is None else h0l.grad, dc0=None if c0l is None else c0l.grad,
                dw=w.grad, db=bias.grad)


@pytest.mark.parametrize('with_init', [False, True], ids=['zero-state', 'h0-c0'])
@pytest.mark.parametrize('T', [1, 4])
@pytest.mark.parametrize('C', [32, 64, 128])
def test_clstm_training_scan_matches_autograd_of_the_unrolled_cell(C, T, with_init):
    """B = 3.  Bounds of test_gpu_refinenet.test_float32_clip_scans_match_the_per_frame_contract for the CRNN scan: 2e-5 on what
    the forward writes, 3e-5 on what the backward writes (T <= 8), relative to max(1, |reference|max).  The restatement is also
    evaluated in float64 and a tensor is held to max(that bound, 4 x the float32 restatement's own deviation from float64); both
    numbers are printed per tensor.  The backward runs on the float32 restatement's forward tensors, so it is compared on equal
    inputs; the weight and bias gradients come from conv_rnn.CLSTMScanFn (one batched launch each over the T*B frames).  With initial
    states the case also feeds a gradient into the stored cell states (dcs), without them that operand is NULL.
    Measured on an MI355X, worst of the 12 cases relative to max(1, |reference|max), kernel error | the float32 restatement's own
    deviation from float64: forward tensors 1.3e-6 | 3.2e-6; dpre 6.1e-7 | 1.2e-6; dxs 3.4e-6 | 2.8e-6; dh0 2.6e-6 | 2.4e-6; dc0
    5.2e-7 | 6.3e-7; dw 7.4e-7 | 7.6e-7; db 5.2e-7 | 5.8e-7 -- the 2e-5 / 3e-5 bounds hold at every width and the float64
    allowance never engaged.
    Every launch runs twice and must reproduce itself bit for bit."""
    hip = default_kernels()
    B = 3
    g = torch.Generator().manual_seed(1000 * C + 10 * T + int(with_init))
    rn = lambda *shape, scale=1.0: torch.randn(shape, generator=g) * scale
    cu = lambda t: None if t is None else t.cuda()
    d = lambda t: None if t is None else t.double()
    s = 0.04 * (64.0 / C) ** 0.5                               # filter scale: the pre-activation variance of the C = 64 test
    xs = rn(B, T, 5, 8, C, scale=0.8)
    h0, c0 = (rn(B, 5, 8, C, scale=0.5), rn(B, 5, 8, C, scale=0.5)) if with_init else (None, None)
    w, bias = rn(4 * C, 3, 3, 2 * C, scale=s), rn(4 * C, scale=0.2)
    dhs, dcs = rn(T, B, 5, 8, C), (rn(T, B, 5, 8, C) if with_init else None)
    want = restate_clstm(xs, h0, c0, w, bias, dhs, dcs)
    want64 = restate_clstm(d(xs), d(h0), d(c0), d(w), d(bias), d(dhs), d(dcs))
    report = []

    def close(name, a, tol):
        b, b64 = want[name], want64[name]
        if b is None:
            assert a is None, name
            return
        a = a.detach().float().cpu()
        assert tuple(a.shape) == tuple(b.shape), (name, tuple(a.shape), tuple(b.shape))
        err, ref_max = float((a - b).abs().max()), float(b.abs().max())
        ref_dev = float((b.double() - b64).abs().max())
        bound = max(tol * max(1.0, ref_max), 4.0 * ref_dev)
        report.append('%s %.1e (restatement f32-vs-f64 %.1e, |ref|max %.2g)' % (name, err, ref_dev, ref_max))
        print(report[-1])
        assert err <= bound, (name, err, bound, ref_dev)

    # training forward, twice; hs / cs bit-equal to the inference entry point
    fwd = [hip.clstm_scan_fwd_train(cu(xs), cu(h0), cu(c0), cu(w), cu(bias)) for _ in range(2)]
    assert hip.lib.eve_last_kernel().decode() == kname('clstm_scan_f32_fwd_train_kernel', C)
    for a, b in zip(*fwd):
        assert torch.equal(a, b)
    hs_i, cs_i = hip.clstm_scan_fwd(cu(xs), cu(h0), cu(c0), cu(w), cu(bias))
    assert hip.lib.eve_last_kernel().decode() == kname('clstm_scan_f32_fwd_kernel', C)
    assert torch.equal(fwd[0][0], hs_i) and torch.equal(fwd[0][1], cs_i)
    for name, a in zip(('hs', 'cs', 'gates_tm', 'cs_tm', 'hs_tm'), fwd[0]):
        close(name, a, 2e-5)
    # backward on the restatement's forward tensors, twice
    wt = w.permute(3, 1, 2, 0).contiguous()
    bwd = [hip.clstm_scan_bwd(cu(dhs), cu(dcs), cu(want['gates_tm'].contiguous()), cu(want['cs_tm'].contiguous()), cu(c0), cu(wt),
                              want_d0=with_init) for _ in range(2)]
    assert hip.lib.eve_last_kernel().decode() == kname('clstm_scan_f32_bwd_kernel', C)
    for a, b in zip(*bwd):
        assert (a is None and b is None) or torch.equal(a, b)
    for name, a in zip(('dpre', 'dxs_tm', 'dh0', 'dc0'), bwd[0]):
        close(name, a, 3e-5)
    # the autograd shell: the same through CLSTMScanFn, plus the batched weight / bias gradients
    wp = torch.nn.Parameter(w.permute(0, 3, 1, 2).contiguous().cuda())           # the module's OIHW parameter
    bp = torch.nn.Parameter(bias.cuda())
    pack = ops.PackedWeight(wp, torch.float32, cin_pad=2 * C, cout_pad=4 * C)
    leaf = lambda t: None if t is None else t.cuda().requires_grad_()
    xl, hl, cl = leaf(xs), leaf(h0), leaf(c0)
    hs_f, cs_f = conv_rnn.CLSTMScanFn.apply(xl, wp, bp, hl, cl, pack)
    assert torch.equal(hs_f, hs_i) and torch.equal(cs_f, cs_i)
    loss = (hs_f * cu(dhs).transpose(0, 1)).sum()
    if dcs is not None:
        loss = loss + (cs_f * cu(dcs).transpose(0, 1)).sum()
    loss.backward()
    close('dxs_tm', xl.grad.transpose(0, 1), 3e-5)
    close('dh0', None if hl is None else hl.grad, 3e-5)
    close('dc0', None if cl is None else cl.grad, 3e-5)
    close('dw', wp.grad.permute(0, 2, 3, 1), 3e-5)
    close('db', bp.grad, 3e-5)


def test_an_unsupported_width_is_refused_without_a_launch():
    hip = default_kernels()
    C = 48
    z = lambda *s: torch.zeros(s, device='cuda')
    before = hip.lib.eve_last_kernel().decode()
    for call in (lambda: hip.clstm_scan_fwd_train(z(1, 1, 5, 8, C), None, None, z(4 * C, 3, 3, 2 * C), z(4 * C)),
                 lambda: hip.clstm_scan_bwd(z(1, 1, 5, 8, C), None, z(1, 1, 5, 8, 4 * C), z(1, 1, 5, 8, C), None, z(2 * C, 3, 3, 4 * C))):
        with pytest.raises(RuntimeError, match='unsupported channel count'):
            call()
    assert hip.lib.eve_last_kernel().decode() == before
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. the per-frame gate adjoint
@pytest.mark.parametrize('with_dc', [False, True], ids=['dc-null', 'dc'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize('C', [32, 64])
def test_clstm_gates_bwd_is_the_adjoint_of_the_gate_math(C, dtype, with_dc):
    """eve_clstm_gates_bwd against autograd of common.py:376-385 on the same (format-valued) operands, P = 3 * 40 pixels:
    float32 to the scan's backward bound (3e-5 relative to max(1, |reference|max)), bf16 / fp16 to test_gpu_kernels.close."""
    hip = default_kernels()
    g = torch.Generator().manual_seed(7 * C + int(with_dc))
    rn = lambda *shape, scale=1.0: (torch.randn(shape, generator=g) * scale).to(dtype)
    gates, c_prev = rn(3, 5, 8, 4 * C, scale=1.5), rn(3, 5, 8, C, scale=0.7)
    dh, dc = rn(3, 5, 8, C), (rn(3, 5, 8, C) if with_dc else None)
    gl, cl = gates.float().clone().requires_grad_(), c_prev.float().clone().requires_grad_()
    i, f, o, gg = gl.chunk(4, dim=-1)
    cn = torch.sigmoid(f) * cl + torch.sigmoid(i) * torch.tanh(gg)
    hn = torch.sigmoid(o) * torch.tanh(cn)
    loss = (hn * dh.float()).sum()
    if with_dc:
        loss = loss + (cn * dc.float()).sum()
    loss.backward()
    got = [hip.clstm_gates_bwd(dh.cuda(), None if dc is None else dc.cuda(), gates.cuda(), c_prev.cuda()) for _ in range(2)]
    for a, b in zip(*got):
        assert torch.equal(a, b)
    for name, a, b in zip(('dgates', 'dc_prev'), got[0], (gl.grad, cl.grad)):
        assert a.dtype == dtype
        if dtype == torch.float32:
            err, ref_max = float((a.cpu() - b).abs().max()), float(b.abs().max())
            assert err <= 3e-5 * max(1.0, ref_max), (name, err, ref_max)
        else:
            close_16bit(a, b, dtype, name)
    # and through the autograd shell
    gp, cp = gates.cuda().requires_grad_(), c_prev.cuda().requires_grad_()
    h2, c2 = conv_rnn.CLSTMGatesFn.apply(gp, cp)
    l2 = (h2.float() * dh.cuda().float()).sum()
    if with_dc:
        l2 = l2 + (c2.float() * dc.cuda().float()).sum()
    l2.backward()
    assert torch.equal(gp.grad, got[0][0]) and torch.equal(cp.grad, got[0][1])


# ------------------------------------------------------------------------------------------------ 3. the module, float32
def make_net(cells=1, screen=True, dtype=torch.float32, live=True, width=64):
    cfg = eve_amd.reset_standalone_config()
    over = {'load_screen_content': screen, 'refine_net_enabled': True, 'refine_net_rnn_type': 'CLSTM',
            'refine_net_rnn_num_cells': cells, 'refine_net_num_features': width}
    cfg.import_dict(dict(over, **{KEY: live}))
    net = eve_amd.RefineNet()
    net.compute_dtype = dtype
    detweights.fill_module(net, seed=1)                  # deterministic NON-ZERO weights: the shipped init zeroes final's last conv
    return net.cuda(), cfg, over


def live_oracle(over):
    """oracle.refine_net.RefineNet with the bottleneck's one line changed: a tuple state's h is handed on."""
    from oracle.refine_net import Bottleneck, RefineNet
    ocfg = OracleConfig(**over)
    ref = detweights.fill_module(RefineNet(ocfg), seed=1)

    def forward(self, x, output_dict, previous_output_dict):
        for i, cell in enumerate(self.rnn_cells):
            key = 'refinenet_rnn_states_%d' % i
            prev = None if previous_output_dict is None else previous_output_dict[key]
            states = cell(x, prev)
            output_dict[key] = states
            x = states[0] if isinstance(states, tuple) else states          # refine_net.py:168-174 drops the tuple instead
        return x

    patched = [m for m in ref.modules() if isinstance(m, Bottleneck)]
    assert len(patched) == 1
    patched[0].forward = types.MethodType(forward, patched[0])
    return ref, ocfg


@pytest.mark.parametrize('cells,screen', [(1, True), (2, True), (1, False)], ids=['one-cell', 'two-cells', 'no-screen'])
def test_live_clstm_refinenet_matches_the_restated_reference(cells, screen):
    """B = 2, T = 3, float32, key on: heat-maps <= 1e-4 and every parameter's gradient norm within 1e-2 (+ 3e-5 absolute for the
    biases whose gradient is exactly zero), as the RefineNet fixture tests hold; the cells' gate banks receive a gradient.
    Without screen content the network's only input is a smooth Gaussian heat-map whose tails are flat: whole max-pool windows and
    ReLU inputs are then EQUAL to the last bit, the gradient there is a set (any tied element may take it), and two float32
    evaluations pick different members -- on the plain heat-map this module is 3.0e-2 off on initial.0.weight on the GPU, 2.2e-2
    under the ATen stand-in kernels on the CPU (no HIP involved), the CGRU model of the parent commit 9.4e-2, with every other
    parameter within 4e-3.  The restated reference is a reference only where the gradient is unique, so the no-screen case adds
    a fixed uniform texture of amplitude 1e-3 to the heat-maps (the screen frames do the same job in the other cases); with it
    the stand-in path is within 7e-4 on every parameter.  Bounds and everything compared are the same in all three cases."""
    rb = detweights.refinenet_batch(2, 3, seed=0, invalid_fraction=0.25)
    if not screen:                                  # break the exact ties of a heat-map-only input (docstring)
        tex = torch.rand(rb['heatmap_initial'].shape, generator=torch.Generator().manual_seed(0))
        rb['heatmap_initial'] = rb['heatmap_initial'] + 1e-3 * tex
    net, cfg, over = make_net(cells, screen)
    ref, ocfg = live_oracle(over)
    hf_o, _ = sequence.refinenet_sequence(ref, rb['heatmap_initial'], rb['screen_frame'] if screen else None)
    sequence.refinenet_losses(hf_o, rb['heatmap_final_gt'], rb['validity'], ocfg)['full_loss'].backward()
    drb = {k: v.cuda() for k, v in rb.items()}
    hf, states = net.forward_sequence(drb['heatmap_initial'], drb['screen_frame'] if screen else None)
    e = maxdiff(hf.detach().cpu(), hf_o.detach())
    print('heatmap_final: max |diff| %.2e' % e)
    assert e <= 1e-4 and float(hf_o.detach().std()) > 1e-3
    assert len(states) == cells and all(isinstance(st, tuple) and tuple(st[0].shape) == (2, 3, 64, 5, 8) for st in states)
    losses.refinenet_loss_terms(hf, drb['heatmap_final_gt'], drb['validity'], cfg)['full_loss'].backward()
    rparams = dict(ref.named_parameters())
    assert set(rparams) == set(dict(net.named_parameters()))
    for n, p in net.named_parameters():
        assert p.grad is not None, n
        got, want = float(p.grad.double().norm()), float(rparams[n].grad.double().norm())
        assert abs(got - want) <= 1e-2 * want + 3e-5, '%s: |g| %.6g vs %.6g' % (n, got, want)
    for i in range(cells):
        gw = dict(net.named_parameters())['network.between_module.between_module.between_module.between_module.between_module'
                                          '.rnn_cells.%d.gates.weight' % i].grad
        assert float(gw.abs().max()) > 0


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_live_clstm_scan_trains_like_the_per_frame_path(dtype):
    """Key on, C = 64, B = 2 x T = 4: whole forward + backward through the clip scan vs eve_dispatch_config.cgru_scan = 0 (the
    per-frame convolution + eve_clstm_gates_{fwd,bwd}); bounds of test_refinenet_clip_scans_train_like_the_per_frame_path."""
    rb = detweights.refinenet_batch(2, 4, seed=3)
    outs = {}
    for mode in (1, 0):
        with default_kernels().dispatch_override(cgru_scan=mode):
            net, _, _ = make_net(dtype=dtype)
            hf, states = net.forward_sequence(rb['heatmap_initial'].cuda(), rb['screen_frame'].cuda())
            (hf.float() * rb['heatmap_final_gt'].cuda()).sum().backward()
        outs[mode] = (hf.detach().float().cpu(), [t.detach().float().cpu() for t in states[0]],
                      {n: p.grad.detach().float().cpu() for n, p in net.named_parameters() if p.grad is not None})
    a, b = outs[1], outs[0]
    f32 = dtype == torch.float32
    assert maxdiff(a[0], b[0]) < (2e-5 if f32 else 0.05)
    for sa, sb in zip(a[1], b[1]):
        assert tuple(sa.shape) == tuple(sb.shape)
        assert maxdiff(sa, sb) < (2e-5 if f32 else 0.06)
    assert set(a[2]) == set(b[2]) and any('.gates.weight' in n for n in a[2])
    for n in b[2]:
        ga, gb = a[2][n], b[2][n]
        if ga.dim() < 2:
            continue          # biases feeding an InstanceNorm have an exactly-zero gradient: what is computed is rounding noise
        assert float((ga - gb).norm()) <= (2e-3 if f32 else 0.15) * float(gb.norm()) + 1e-4, n


def test_key_off_keeps_the_reference_dead_cell():
    """The default: the cell's parameters get no gradient and heatmap_final does not depend on them (their replacement by noise
    changes nothing, bit for bit) -- and with the key on, on the same weights, it does."""
    rb = detweights.refinenet_batch(2, 3, seed=0)
    hm, sc = rb['heatmap_initial'].cuda(), rb['screen_frame'].cuda()
    res = {}
    for live in (False, True):
        net, _, _ = make_net(live=live)
        hf, _ = net.forward_sequence(hm, sc)
        (hf * rb['heatmap_final_gt'].cuda()).sum().backward()
        cellp = {n: p for n, p in net.named_parameters() if '.rnn_cells.' in n}
        assert len(cellp) == 2
        for n, p in cellp.items():
            assert (p.grad is not None) == live, n
        with torch.no_grad():
            for n, p in cellp.items():
                p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(5)).cuda() * 0.05)
            net.invalidate_packs()
            hf2, _ = net.forward_sequence(hm, sc)
        res[live] = (hf.detach(), hf2)
    assert torch.equal(*res[False])
    assert maxdiff(*res[True]) > 1e-4
    assert maxdiff(res[False][0], res[True][0]) > 1e-4


# ------------------------------------------------------------------------------------------------ 4. streaming and training
def test_stream_with_a_live_clstm_matches_the_whole_clip():
    """EVEStream at B = 2, a clip of 4 frames as 1 + 3, key on, equals one eval pass (bounds of
    test_gpu_stream.test_stream_float32_matches_the_whole_clip); the carried state is the float32 (h, c) pair."""
    model, _ = make_model('refine_net.json')
    model.refine_net.config.override(KEY, True)
    b, d, full = gpu_clip(2, 4)
    with torch.no_grad():
        whole = model(dict(full))
    stream = eve_amd.EVEStream(model, 2)
    got = run_chunks(stream, d, [1, 3])
    checked = 0
    for k, v in got.items():
        if k in whole:
            e = maxdiff(v, whole[k])
            amp = 5.0 if k.endswith('_final') else 1.0
            assert e <= amp * (1e-2 if 'px' in k else (1e-3 if 'cm' in k else 1e-5)), (k, e)
            checked += 1
    assert checked >= 4 and any(k.endswith('_final') for k in got if k in whole)
    st = stream.get_state()['refinenet_rnn_states_0']
    assert isinstance(st, tuple) and all(tuple(t.shape) == (2, 64, 5, 8) and t.dtype == torch.float32 for t in st)
    # the stream really runs the live cell: the dead one is outside the stream's bound on the same weights
    model.refine_net.config.override(KEY, False)
    with torch.no_grad():
        dead = model(dict(full))
    assert maxdiff(dead['PoG_px_final'], whole['PoG_px_final']) > 5e-2 and torch.equal(dead['PoG_px_initial'], whole['PoG_px_initial'])


def test_refinenet_trainer_step_updates_the_live_cell():
    """One train.refinenet_trainer step, float32, key on: the cell's parameters live in the flat buffer, receive their gradients
    in place and change; the update equals clip_grad_norm_ + torch.optim.Adam on the same gradients to the tolerance of
    test_gpu_bf16_parity.test_trainer_update_equals_clip_plus_torch_adam_on_the_same_gradients."""
    from eve_amd import train
    net, cfg, _ = make_net()
    trainer = train.refinenet_trainer(net, cfg)
    cell = [n for n, _ in net.named_parameters() if '.rnn_cells.' in n]
    assert len(cell) == 2
    before = {n: p.detach().cpu().clone() for n, p in net.named_parameters()}
    shadow = {n: torch.nn.Parameter(t.clone()) for n, t in before.items()}
    opt = torch.optim.Adam(shadow.values(), lr=cfg.learning_rate, weight_decay=cfg.weight_decay)
    batch = {k: v.cuda() for k, v in detweights.refinenet_batch(2, 3, seed=41, invalid_fraction=0.2).items()}
    trainer._forward_backward(batch)
    for n, p in net.named_parameters():
        assert p.grad is not None, n
        shadow[n].grad = p.grad.detach().cpu().clone()
    for n in cell:
        p = dict(net.named_parameters())[n]
        assert getattr(p, '_eve_flat_grad', False) and float(p.grad.abs().max()) > 0, n
    total = float(torch.nn.utils.clip_grad_norm_(list(shadow.values()), cfg.gradient_clip_amount))
    opt.step()
    trainer._update(1.0)
    np.testing.assert_allclose(float(trainer.sumsq.sqrt()), total, rtol=1e-5)
    for n, p in net.named_parameters():
        diff = (p.detach().cpu() - shadow[n].detach()).abs().reshape(-1)
        assert float(diff.max()) <= 2.0 * cfg.learning_rate, n
        assert float((diff > 1e-4 * cfg.learning_rate).float().mean()) <= 1e-3, n
        assert float(diff.mean()) <= 1e-4 * cfg.learning_rate, n
    for n in cell:
        assert float((dict(net.named_parameters())[n].detach().cpu() - before[n]).abs().max()) > 0, n
