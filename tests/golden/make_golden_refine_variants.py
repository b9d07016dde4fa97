#!/usr/bin/env python
"""Golden vectors for the OTHER bottleneck configurations of the reference RefineNet (src/models/refine_net.py:132-176, 188:
`refine_net_num_features` and `refine_net_rnn_num_cells`), produced by running the reference's own RefineNet.forward per
step: stacked cells and the 32- / 128-wide bottleneck, which tests/golden/refinenet.npz (64 wide, one cell) does not cover.

Run here only (needs /root/reference):   python tests/golden/make_golden_refine_variants.py
Writes tests/golden/refinenet_variants.npz (numbers only; inputs and weights come from oracle/detweights.py seeds).
Per case `<tag>/`: heatmap_final [B,T,1,18,32] (every 4th pixel), state_<i> [B,T,C,5,8] for every cell i at every frame (and
cell_<i>, the second half of a CLSTM tuple), loss_ce, and grad_names / grad_norms for the scalar loss of refinenet.npz
(1.0 * cross-entropy + 0.0 * MSE of heatmap_final; -1 = no gradient reached the parameter).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from oracle import detweights  # noqa: E402

# tag: (refine_net_rnn_type, refine_net_num_features, refine_net_rnn_num_cells)
CASES = {
    'CGRU_c32_n1': ('CGRU', 32, 1),
    'CGRU_c128_n1': ('CGRU', 128, 1),
    'CGRU_c64_n2': ('CGRU', 64, 2),
    'CRNN_c64_n2': ('CRNN', 64, 2),
    'CLSTM_c32_n2': ('CLSTM', 32, 2),
}
B, T, SEED, WEIGHT_SEED, INVALID = 2, 3, 4, 1, 0.25


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    config = mg.import_reference()
    from models.refine_net import RefineNet
    from losses.cross_entropy import CrossEntropyLoss
    from losses.mse import MSELoss
    config.override('load_screen_content', True)
    config.override('refine_net_enabled', True)
    rb = detweights.refinenet_batch(B, T, seed=SEED, invalid_fraction=INVALID)
    fix = {'B': B, 'T': T, 'seed': SEED, 'weight_seed': WEIGHT_SEED, 'invalid_fraction': INVALID}
    for tag, (kind, width, n_cells) in CASES.items():
        config.override('refine_net_rnn_type', kind)
        config.override('refine_net_num_features', width)
        config.override('refine_net_rnn_num_cells', n_cells)
        net = detweights.fill_module(RefineNet(), seed=WEIGHT_SEED)
        outs, prev, states = [], None, [[] for _ in range(n_cells)]
        for t in range(T):
            sub_in = {'screen_frame': rb['screen_frame'][:, t]}
            sub_out = {'heatmap_initial': rb['heatmap_initial'][:, t]}
            net(sub_in, sub_out, previous_output_dict=prev)
            outs.append(sub_out['heatmap_final'])
            for i in range(n_cells):
                states[i].append(sub_out['refinenet_rnn_states_%d' % i])
            prev = sub_out
        hf = torch.stack(outs, dim=1)
        ref = {'heatmap_final': rb['heatmap_final_gt'], 'heatmap_final_validity': rb['validity']}
        ce = CrossEntropyLoss()(hf, 'heatmap_final', ref)
        mse = MSELoss()(hf, 'heatmap_final', ref)
        (1.0 * ce + 0.0 * mse).backward()
        fix[tag + '/heatmap_final'] = mg.np_(hf[..., ::4, ::4])
        for i, per_t in enumerate(states):
            if isinstance(per_t[0], tuple):
                fix['%s/state_%d' % (tag, i)] = mg.np_(torch.stack([s[0] for s in per_t], dim=1))
                fix['%s/cell_%d' % (tag, i)] = mg.np_(torch.stack([s[1] for s in per_t], dim=1))
            else:
                fix['%s/state_%d' % (tag, i)] = mg.np_(torch.stack(per_t, dim=1))
        fix[tag + '/loss_ce'] = mg.np_(ce)
        names, norms, _ = mg.grad_summary(net)
        fix[tag + '/grad_names'], fix[tag + '/grad_norms'] = names, norms
        print(tag, 'ce', float(ce.detach()), 'dead grads', int((np.asarray(norms) < 0).sum()), 'of', len(norms),
              'state std', float(fix[tag + '/state_0'].std()))
    out = os.path.join(mg.OUT, 'refinenet_variants.npz')
    np.savez_compressed(out, **fix)
    print('refinenet_variants.npz', len(fix), 'arrays', os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
