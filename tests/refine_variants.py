"""Shared by test_refine_scan_variants_host.py and test_gpu_refine_scan_variants.py: the five bottleneck configurations of
tests/golden/refinenet_variants.npz (tests/golden/make_golden_refine_variants.py) and how a model of each is built and read."""
import os

import numpy as np
import torch

from oracle import detweights
from oracle.config import OracleConfig

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
# tag: (refine_net_rnn_type, refine_net_num_features, refine_net_rnn_num_cells) -- the cases the fixture was generated for
CASES = {
    'CGRU_c32_n1': ('CGRU', 32, 1),
    'CGRU_c128_n1': ('CGRU', 128, 1),
    'CGRU_c64_n2': ('CGRU', 64, 2),
    'CRNN_c64_n2': ('CRNN', 64, 2),
    'CLSTM_c32_n2': ('CLSTM', 32, 2),
}


def overrides(tag):
    kind, width, cells = CASES[tag]
    return {'load_screen_content': True, 'refine_net_enabled': True, 'refine_net_rnn_type': kind,
            'refine_net_num_features': width, 'refine_net_rnn_num_cells': cells}


def fixture():
    return np.load(os.path.join(GOLDEN, 'refinenet_variants.npz'))


def fixture_batch(fx):
    return detweights.refinenet_batch(int(fx['B']), int(fx['T']), seed=int(fx['seed']), invalid_fraction=float(fx['invalid_fraction']))


def make_net(tag, dtype=torch.float32, weight_seed=1):
    """(eve_amd.RefineNet with the deterministic weights, its config) for a case; on the CPU -- callers move it."""
    import eve_amd
    cfg = eve_amd.reset_standalone_config()
    cfg.import_dict(overrides(tag))
    net = eve_amd.RefineNet()
    net.compute_dtype = dtype
    detweights.fill_module(net, seed=weight_seed)
    return net, cfg


def make_oracle(tag, weight_seed=1):
    from oracle.refine_net import RefineNet
    cfg = OracleConfig(**overrides(tag))
    return detweights.fill_module(RefineNet(cfg), seed=weight_seed), cfg


def per_step(net, heatmap_initial, screen_frame, n_cells):
    """The reference's per-step dict contract over a clip -> (heatmap_final [B,T,1,H,W], per cell the stacked states
    [B,T,C,5,8], a pair for a CLSTM cell)."""
    outs, prev, hist = [], None, [[] for _ in range(n_cells)]
    for t in range(heatmap_initial.shape[1]):
        so = {'heatmap_initial': heatmap_initial[:, t]}
        net({'screen_frame': screen_frame[:, t]}, so, previous_output_dict=prev)
        outs.append(so['heatmap_final'])
        for i in range(n_cells):
            hist[i].append(so['refinenet_rnn_states_%d' % i])
        prev = so
    states = [tuple(torch.stack([s[j] for s in h], dim=1) for j in range(2)) if isinstance(h[0], tuple) else torch.stack(h, dim=1)
              for h in hist]
    return torch.stack(outs, dim=1), states


def fixture_states(fx, tag):
    """Per cell the fixture's states [B,T,C,5,8] (a pair (h, c) for CLSTM)."""
    kind, _, cells = CASES[tag]
    return [(fx['%s/state_%d' % (tag, i)], fx['%s/cell_%d' % (tag, i)]) if kind == 'CLSTM' else fx['%s/state_%d' % (tag, i)]
            for i in range(cells)]


def flat(states):
    """[(name, tensor)] over cells and tuple halves."""
    out = []
    for i, st in enumerate(states):
        for j, t in enumerate(st if isinstance(st, tuple) else (st,)):
            out.append(('cell%d.%d' % (i, j), t))
    return out


# ---- the per-frame contract of the clip scans (common.py:331-415 applied per frame), evaluated in the dtype of its operands ----
# tests/fake_kernels.py states the same contract but converts to float32 inside; these run in float32 AND float64, which is what
# the float32 bounds at K = 2 304 are derived from.  Layouts are the kernels': NHWC activations, OHWI / IHWO filter banks.
def _conv(x, w_ohwi, bias):
    return torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w_ohwi.permute(0, 3, 1, 2), bias, 1, 1).permute(0, 2, 3, 1)


def _dgrad(dy, w_ihwo):
    w = w_ihwo.permute(3, 0, 1, 2)                                      # [Cout, Cin, KH, KW]
    shape = (dy.shape[0], w.shape[1], dy.shape[1], dy.shape[2])
    return torch.nn.grad.conv2d_input(shape, w, dy.permute(0, 3, 1, 2), 1, 1).permute(0, 2, 3, 1)


def contract_cgru_fwd(xs, h0, w1, b1, w2, b2, rnd=lambda t: t):
    """-> hs [B,T,..], and time-major hs_tm, ru, rh, og.  rnd: the storage rounding of the 16-bit scans (the two sigmoid
    gates, r * h, the tanh gate and the new state are rounded to the format; the convolutions accumulate in float32 and are NOT
    rounded, unlike the per-frame kernels' outputs) -- pass e.g. lambda t: t.bfloat16().float() with bf16-valued operands."""
    h = torch.zeros_like(xs[:, 0]) if h0 is None else h0
    C = h.shape[-1]
    hs, rus, rhs, ogs = [], [], [], []
    for t in range(xs.shape[1]):
        ru = rnd(torch.sigmoid(_conv(torch.cat([xs[:, t], h], -1), w1, b1)))
        rh = rnd(ru[..., :C] * h)
        o = rnd(torch.tanh(_conv(torch.cat([rh, xs[:, t]], -1), w2, b2)))
        u = ru[..., C:]
        h = rnd((1 - u) * o + u * h)
        hs.append(h); rus.append(ru); rhs.append(rh); ogs.append(o)
    return torch.stack(hs, 1), torch.stack(hs, 0), torch.stack(rus, 0), torch.stack(rhs, 0), torch.stack(ogs, 0)


def contract_cgru_bwd(dhs_tm, ru, og, hs_tm, h0, w1t, w2t, want_dh0):
    """-> time-major dg1_all, dg2_all, dxs_tm, and dh0 or None"""
    T, B, H, W, C = dhs_tm.shape
    carry = torch.zeros_like(dhs_tm[0])
    dg1_all, dg2_all, dxs = [None] * T, [None] * T, [None] * T
    for t in range(T - 1, -1, -1):
        hp = hs_tm[t - 1] if t > 0 else (h0 if h0 is not None else torch.zeros_like(hs_tm[0]))
        r, u, o = ru[t][..., :C], ru[t][..., C:], og[t]
        dhn = dhs_tm[t] + carry
        dg2 = dhn * (1 - u) * (1 - o * o)
        dcat2 = _dgrad(dg2, w2t)
        drh, dx2 = dcat2[..., :C], dcat2[..., C:]
        dg1 = torch.cat([drh * hp * r * (1 - r), dhn * (hp - o) * u * (1 - u)], dim=-1)
        dcat1 = _dgrad(dg1, w1t)
        carry = dhn * u + drh * r + dcat1[..., C:]
        dg1_all[t], dg2_all[t], dxs[t] = dg1, dg2, dcat1[..., :C] + dx2
    return torch.stack(dg1_all, 0), torch.stack(dg2_all, 0), torch.stack(dxs, 0), (carry if want_dh0 else None)


def contract_crnn_fwd(xs, h0, w, bias):
    h = torch.zeros_like(xs[:, 0]) if h0 is None else h0
    hs = []
    for t in range(xs.shape[1]):
        h = torch.tanh(_conv(torch.cat([xs[:, t], h], -1), w, bias))
        hs.append(h)
    return torch.stack(hs, 1), torch.stack(hs, 0)


def contract_crnn_bwd(dhs_tm, hs_tm, wt, want_dh0):
    T, C = dhs_tm.shape[0], dhs_tm.shape[-1]
    carry = torch.zeros_like(dhs_tm[0])
    dpre, dxs = [None] * T, [None] * T
    for t in range(T - 1, -1, -1):
        a = (dhs_tm[t] + carry) * (1 - hs_tm[t] * hs_tm[t])
        dcat = _dgrad(a, wt)
        dpre[t], dxs[t], carry = a, dcat[..., :C], dcat[..., C:]
    return torch.stack(dpre, 0), torch.stack(dxs, 0), (carry if want_dh0 else None)


def contract_clstm_fwd(xs, h0, c0, w, bias):
    h = torch.zeros_like(xs[:, 0]) if h0 is None else h0
    c = torch.zeros_like(xs[:, 0]) if c0 is None else c0
    hs, cs = [], []
    for t in range(xs.shape[1]):
        i, f, o, g = _conv(torch.cat([xs[:, t], h], -1), w, bias).chunk(4, dim=-1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        hs.append(h); cs.append(c)
    return torch.stack(hs, 1), torch.stack(cs, 1)
