"""CPU: the module logic behind refine_net_clstm_feeds_features (eve_amd only; the reference drops a tuple state's output,
refine_net.py:168-174) under a torch-CPU stand-in for the three new kernels: key on / off routing, the stacked order, the
getattr default under the reference's own config singleton, and the state layout.  The GPU side: test_gpu_clstm_live.py."""
import sys
import types

import pytest
import torch

import eve_amd
from eve_amd import kernels, train
from fake_kernels import FakeKernels, nchw
from oracle import detweights, sequence
from oracle.config import OracleConfig
from oracle.refine_net import Bottleneck as OracleBottleneck
from oracle.refine_net import RefineNet as OracleRefineNet

KEY = 'refine_net_clstm_feeds_features'


def _dgrad(dy, w_ihwo):
    shape = (dy.shape[0], w_ihwo.shape[0], dy.shape[1], dy.shape[2])
    return torch.nn.grad.conv2d_input(shape, w_ihwo.permute(3, 0, 1, 2).float(), nchw(dy), 1, 1).permute(0, 2, 3, 1)


class LiveFakes(FakeKernels):
    """FakeKernels plus the contracts of eve_clstm_scan_fwd_train_c / eve_clstm_scan_bwd_c / eve_clstm_gates_bwd
    (include/eve_hip.h), restated with ATen ops; `calls` counts what the module issued."""

    def __init__(self):
        self.calls = {'clstm_scan_fwd': 0, 'clstm_scan_fwd_train': 0, 'clstm_scan_bwd': 0, 'clstm_gates_fwd': 0, 'clstm_gates_bwd': 0}

    def clstm_scan_fwd(self, *a):
        self.calls['clstm_scan_fwd'] += 1
        return super().clstm_scan_fwd(*a)

    def clstm_gates_fwd(self, *a):
        self.calls['clstm_gates_fwd'] += 1
        return super().clstm_gates_fwd(*a)

    def clstm_scan_fwd_train(self, xs, h0, c0, w_ohwi, bias):
        self.calls['clstm_scan_fwd_train'] += 1
        h = torch.zeros_like(xs[:, 0]) if h0 is None else h0
        c = torch.zeros_like(xs[:, 0]) if c0 is None else c0
        hs, cs, gates = [], [], []
        for t in range(xs.shape[1]):
            i, f, o, g = self.conv2d_fwd(torch.cat([xs[:, t], h], -1), w_ohwi, bias, 1, 1).chunk(4, dim=-1)
            i, f, o, g = torch.sigmoid(i), torch.sigmoid(f), torch.sigmoid(o), torch.tanh(g)
            c = f * c + i * g
            h = o * torch.tanh(c)
            hs.append(h); cs.append(c); gates.append(torch.cat([i, f, o, g], -1))
        return torch.stack(hs, 1), torch.stack(cs, 1), torch.stack(gates, 0), torch.stack(cs, 0), torch.stack(hs, 0)

    def clstm_scan_bwd(self, dhs_tm, dcs_tm, gates_tm, cs_tm, c0, w_ihwo, want_d0=False):
        self.calls['clstm_scan_bwd'] += 1
        T, B, H, W, C = dhs_tm.shape
        carry_h, carry_c = torch.zeros((B, H, W, C)), torch.zeros((B, H, W, C))
        dpre, dxs = [None] * T, [None] * T
        for t in range(T - 1, -1, -1):
            i, f, o, g = gates_tm[t].chunk(4, dim=-1)
            cp = cs_tm[t - 1] if t > 0 else (c0 if c0 is not None else torch.zeros_like(cs_tm[0]))
            dh = dhs_tm[t] + carry_h
            tc = torch.tanh(cs_tm[t])
            dc = carry_c + dh * o * (1 - tc * tc) + (0 if dcs_tm is None else dcs_tm[t])
            dpre[t] = torch.cat([dc * g * i * (1 - i), dc * cp * f * (1 - f), dh * tc * o * (1 - o), dc * i * (1 - g * g)], -1)
            carry_c = dc * f
            dcat = _dgrad(dpre[t], w_ihwo)
            dxs[t], carry_h = dcat[..., :C].contiguous(), dcat[..., C:]
        return (torch.stack(dpre, 0), torch.stack(dxs, 0), carry_h.contiguous() if want_d0 else None,
                carry_c.contiguous() if want_d0 else None)

    def clstm_gates_bwd(self, dh, dc_in, gates, c_prev):
        self.calls['clstm_gates_bwd'] += 1
        i, f, o, g = gates.float().chunk(4, dim=-1)
        i, f, o, g = torch.sigmoid(i), torch.sigmoid(f), torch.sigmoid(o), torch.tanh(g)
        tc = torch.tanh(f * c_prev.float() + i * g)
        dc = dh.float() * o * (1 - tc * tc) + (0 if dc_in is None else dc_in.float())
        dg = torch.cat([dc * g * i * (1 - i), dc * c_prev.float() * f * (1 - f), dh.float() * tc * o * (1 - o), dc * i * (1 - g * g)], -1)
        return dg.to(gates.dtype), (dc * f).to(c_prev.dtype)


@pytest.fixture()
def fake():
    k = LiveFakes()
    kernels.set_default_kernels(k)
    yield k
    kernels.set_default_kernels(None)
    eve_amd.reset_standalone_config()


def make_pair(cells=1, live=True):
    """(eve_amd.RefineNet, its config, the oracle with the bottleneck's one line changed when `live`, the oracle's config)"""
    over = {'load_screen_content': True, 'refine_net_enabled': True, 'refine_net_rnn_type': 'CLSTM', 'refine_net_rnn_num_cells': cells}
    cfg = eve_amd.reset_standalone_config()
    assert getattr(cfg, KEY) is False                      # the default
    cfg.import_dict(dict(over, **{KEY: live}))
    net = eve_amd.RefineNet()
    net.compute_dtype = torch.float32
    ocfg = OracleConfig(**over)
    ref = OracleRefineNet(ocfg)
    assert list(net.state_dict().keys()) == list(ref.state_dict().keys())          # the key adds no parameter and renames none
    detweights.fill_module(net, 1); detweights.fill_module(ref, 1)
    if live:
        def forward(self, x, output_dict, previous_output_dict):
            for i, cell in enumerate(self.rnn_cells):
                key = 'refinenet_rnn_states_%d' % i
                states = cell(x, None if previous_output_dict is None else previous_output_dict[key])
                output_dict[key] = states
                x = states[0] if isinstance(states, tuple) else states          # refine_net.py:168-174 drops the tuple instead
            return x
        bott = [m for m in ref.modules() if isinstance(m, OracleBottleneck)]
        assert len(bott) == 1
        bott[0].forward = types.MethodType(forward, bott[0])
    return net, cfg, ref, ocfg


def oracle_states(ref, rb, cells):
    """The oracle's per-step states over the clip: per cell (h, c) [B, T, C, 5, 8]."""
    prev, hist = None, [[] for _ in range(cells)]
    for t in range(rb['heatmap_initial'].shape[1]):
        so = {'heatmap_initial': rb['heatmap_initial'][:, t]}
        ref({'screen_frame': rb['screen_frame'][:, t]}, so, previous_output_dict=prev)
        for i in range(cells):
            hist[i].append(so['refinenet_rnn_states_%d' % i])
        prev = so
    return [tuple(torch.stack([s[j] for s in h], dim=1) for j in range(2)) for h in hist]


@pytest.mark.parametrize('cells', [1, 2])
def test_key_on_routes_the_clip_through_the_differentiable_scan(fake, cells):
    """Heat-maps, every cell's (h, c) history and every parameter gradient equal the restated reference; with two cells this is
    only so if cell 1 reads cell 0's h (not the bottleneck input, which is what the dead stack hands every cell)."""
    net, cfg, ref, ocfg = make_pair(cells, live=True)
    rb = detweights.refinenet_batch(2, 3, seed=5)
    hf, states = net.forward_sequence(rb['heatmap_initial'], rb['screen_frame'])
    # the restated reference in FLOAT64: two float32 evaluations of this network differ from each other by the sum of their own
    # deviations from the exact gradient (the float32 oracle alone is 2.5e-2 away on initial.1.bias: ReLU / max-pool decisions on
    # last-bit ties), so the module is held to the host suite's 3e-2 against the exact one
    ref = ref.double()
    rb64 = {k: (v.double() if v.is_floating_point() else v) for k, v in rb.items()}
    want, _ = sequence.refinenet_sequence(ref, rb64['heatmap_initial'], rb64['screen_frame'])
    assert float((hf.detach() - want.detach()).abs().max()) < 1e-4
    assert fake.calls['clstm_scan_fwd_train'] == cells and fake.calls['clstm_scan_fwd'] == 0
    with torch.no_grad():
        for st, ost in zip(states, oracle_states(ref, rb64, cells)):
            assert isinstance(st, tuple) and len(st) == 2
            for a, b in zip(st, ost):
                assert tuple(a.shape) == tuple(b.shape) == (2, 3, 64, 5, 8)
                assert float((a - b).abs().max()) < 1e-4
    sequence.refinenet_losses(hf, rb['heatmap_final_gt'], rb['validity'], ocfg)['full_loss'].backward()
    sequence.refinenet_losses(want, rb64['heatmap_final_gt'], rb64['validity'], ocfg)['full_loss'].backward()
    assert fake.calls['clstm_scan_bwd'] == cells
    rp = dict(ref.named_parameters())
    for n, p in net.named_parameters():
        assert p.grad is not None and rp[n].grad is not None, n
        a, b = p.grad.double(), rp[n].grad.double()
        assert float((a - b).norm()) <= 3e-2 * float(b.norm()) + 1e-5, n
    assert sum('.rnn_cells.' in n for n in rp) == 2 * cells


def test_key_off_is_the_reference_dead_cell(fake):
    net, cfg, ref, ocfg = make_pair(2, live=False)
    rb = detweights.refinenet_batch(2, 2, seed=5)
    hf, states = net.forward_sequence(rb['heatmap_initial'], rb['screen_frame'])
    want, _ = sequence.refinenet_sequence(ref, rb['heatmap_initial'], rb['screen_frame'])
    assert float((hf.detach() - want.detach()).abs().max()) < 1e-4
    assert fake.calls['clstm_scan_fwd'] == 2 and fake.calls['clstm_scan_fwd_train'] == 0
    hf.sum().backward()
    assert fake.calls['clstm_scan_bwd'] == 0 and fake.calls['clstm_gates_bwd'] == 0
    for n, p in net.named_parameters():
        assert (p.grad is None) == ('.rnn_cells.' in n), n
    # every cell of the dead stack saw the bottleneck input, as in the reference
    with torch.no_grad():
        for st, ost in zip(states, oracle_states(ref, rb, 2)):
            for a, b in zip(st, ost):
                assert float((a - b).abs().max()) < 1e-4


def test_inference_with_the_key_on_keeps_nothing_for_a_backward(fake):
    net, cfg, ref, ocfg = make_pair(1, live=True)
    rb = detweights.refinenet_batch(2, 2, seed=5)
    with torch.no_grad():
        hf, _ = net.forward_sequence(rb['heatmap_initial'], rb['screen_frame'])
        want, _ = sequence.refinenet_sequence(ref, rb['heatmap_initial'], rb['screen_frame'])
    assert fake.calls['clstm_scan_fwd'] == 1 and fake.calls['clstm_scan_fwd_train'] == 0
    assert float((hf.detach() - want.detach()).abs().max()) < 1e-4


def test_per_step_contract_and_continuation_with_the_key_on(fake):
    """forward() with previous_output_dict (per-frame convolution + eve_clstm_gates_{fwd,bwd}) equals forward_sequence, stores
    the state as (h, c) in the reference layout and differentiates through the cell; a clip continued from a previous call's last
    state equals the whole clip."""
    net, cfg, ref, ocfg = make_pair(1, live=True)
    rb = detweights.refinenet_batch(2, 3, seed=5)
    hf, states = net.forward_sequence(rb['heatmap_initial'], rb['screen_frame'])
    outs, prev = [], None
    for t in range(3):
        so = {'heatmap_initial': rb['heatmap_initial'][:, t]}
        net({'screen_frame': rb['screen_frame'][:, t]}, so, previous_output_dict=prev)
        st = so['refinenet_rnn_states_0']
        assert isinstance(st, tuple) and all(tuple(s.shape) == (2, 64, 5, 8) for s in st)
        outs.append(so['heatmap_final'])
        prev = so
    stepped = torch.stack(outs, dim=1)
    assert float((stepped - hf).detach().abs().max()) < 1e-5
    assert fake.calls['clstm_gates_fwd'] == 3
    net.zero_grad()
    stepped.sum().backward()
    assert fake.calls['clstm_gates_bwd'] == 3
    g_step = {n: p.grad.clone() for n, p in net.named_parameters()}
    net.zero_grad()
    hf.sum().backward()
    for n, p in net.named_parameters():
        if p.dim() < 2:
            continue          # biases feeding an InstanceNorm have an exactly-zero gradient: what is computed is rounding noise
        assert float((p.grad - g_step[n]).norm()) <= 2e-3 * float(p.grad.norm()) + 1e-4, n      # the GPU suite's scan-vs-per-frame bound
    assert float(g_step[[n for n in g_step if n.endswith('rnn_cells.0.gates.weight')][0]].abs().max()) > 0
    with torch.no_grad():
        first, st1 = net.forward_sequence(rb['heatmap_initial'][:, :1], rb['screen_frame'][:, :1])
        rest, st2 = net.forward_sequence(rb['heatmap_initial'][:, 1:], rb['screen_frame'][:, 1:],
                                         initial_states=[tuple(s[:, -1] for s in st1[0])])
    assert float((torch.cat([first, rest], 1) - hf.detach()).abs().max()) < 1e-5
    for a, b in zip(st2[0], states[0]):
        assert float((a[:, -1] - b[:, -1]).abs().max()) < 1e-5


def test_reference_config_singleton_without_the_key_means_off(fake, monkeypatch):
    """Inside the reference code base get_config() returns core.DefaultConfig(), which has no such key: every reader uses
    getattr(config, key, False), so the module builds, runs and keeps the dead cell."""
    ocfg = OracleConfig(load_screen_content=True, refine_net_enabled=True, refine_net_rnn_type='CLSTM')
    assert not hasattr(ocfg, KEY)
    core = types.ModuleType('core')
    core.DefaultConfig = lambda: ocfg
    monkeypatch.setitem(sys.modules, 'core', core)
    assert eve_amd.get_config() is ocfg
    net = eve_amd.RefineNet()
    net.compute_dtype = torch.float32
    detweights.fill_module(net, 1)
    assert net._clstm_live() is False
    rb = detweights.refinenet_batch(1, 2, seed=5)
    hf, _ = net.forward_sequence(rb['heatmap_initial'], rb['screen_frame'])
    hf.sum().backward()
    assert fake.calls['clstm_scan_fwd'] == 1 and fake.calls['clstm_scan_fwd_train'] == 0
    assert all(p.grad is None for n, p in net.named_parameters() if '.rnn_cells.' in n)


def test_trainer_holds_the_live_cell_in_its_flat_buffer(fake):
    """train.refinenet_trainer needs no logic of its own: the cell's parameters are entries of the flat buffer, their gradients
    are written into its gradient slices in place, and a step changes them."""
    net, cfg, _, _ = make_pair(1, live=True)
    tr = train.refinenet_trainer(net, cfg)
    cell = {n: p for n, p in net.named_parameters() if '.rnn_cells.' in n}
    assert len(cell) == 2
    in_flat = {id(p) for p, _, _ in tr.fp.entries}
    rb = detweights.refinenet_batch(2, 2, seed=5, invalid_fraction=0.2)
    before = {n: p.detach().clone() for n, p in cell.items()}
    tr.step(rb)
    for n, p in cell.items():
        assert id(p) in in_flat and getattr(p, '_eve_flat_grad', False), n
        assert float(p.grad.abs().max()) > 0 and float((p.detach() - before[n]).abs().max()) > 0, n
    for p, off, n in tr.fp.entries:
        assert p.grad.data_ptr() == tr.fp.grad.data_ptr() + 4 * off
