#!/usr/bin/env python
"""Per-launch timing of the EyeNet recurrent scans, forward and backward, float32:
    bench_scan.py [--cell GRU|RNN|LSTM] [--reps 30] [--json FILE]
H = 256 runs the one-workgroup-per-sequence kernels of csrc/recurrent.hip (the yardstick), H = 512 / 1024 the wide family of
csrc/recurrent_wide.hip (tiles of 16 sequences on v_mfma_f32_16x16x4_f32).  Shapes: S = 64, T = 30 (the tail of a B = 32 train
step: both eyes) and S = 2, T = 1 (one live camera).  HIP events around `reps` back-to-back launches after a warm-up launch,
the median of 5 such windows.  The float32 rate counts the recurrent product only, 2 * S * T * H * G*H per direction; for the
wide family the MFMAs also run the rows of a partial tile, so the share of the matrix pipe that is BUSY is higher by
16 * ceil(S / 16) / S."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eve_amd.kernels import HipKernels  # noqa: E402

GATES = {'GRU': 3, 'RNN': 1, 'LSTM': 4}
SHAPES = [(64, 30), (2, 1)]
WIDTHS = [256, 512, 1024]


def timeit(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps * 1e3)
    out.sort()
    return out[2], out[0], out[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cell', default='GRU', choices=sorted(GATES))
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    assert a.reps >= 20
    G = GATES[a.cell]
    k = HipKernels()
    g = torch.Generator(device='cpu').manual_seed(0)
    rows = []
    print('%s scan, float32, us per launch: median (min .. max) of 5 windows of %d launches' % (a.cell, a.reps))
    for S, T in SHAPES:
        for H in WIDTHS:
            gi = torch.randn((S, T, G * H), generator=g).cuda()
            whh = (torch.randn((G * H, H), generator=g) * H ** -0.5).cuda()
            wt = whh.t().contiguous()
            bhh = (torch.randn((G * H,), generator=g) * 0.1).cuda()
            dhs = torch.randn((S, T, H), generator=g).cuda()
            if a.cell == 'GRU':
                hs, gates, hn = k.gru_scan_fwd(gi, wt, bhh, None)
                fwd = lambda: k.gru_scan_fwd(gi, wt, bhh, None)
                bwd = lambda: k.gru_scan_bwd(dhs, whh, None, hs, gates, hn, True)
            elif a.cell == 'RNN':
                hs = k.rnn_scan_fwd(gi, wt, bhh, None)
                fwd = lambda: k.rnn_scan_fwd(gi, wt, bhh, None)
                bwd = lambda: k.rnn_scan_bwd(dhs, whh, hs, True)
            else:
                hs, cs, gates = k.lstm_scan_fwd(gi, wt, bhh, None, None)
                fwd = lambda: k.lstm_scan_fwd(gi, wt, bhh, None, None)
                bwd = lambda: k.lstm_scan_bwd(dhs, None, whh, None, hs, cs, gates, True)
            flop = 2.0 * S * T * H * G * H
            row = dict(cell=a.cell, S=S, T=T, H=H, flop=flop)
            for name, fn in (('fwd', fwd), ('bwd', bwd)):
                fn()
                kern = k.lib.eve_last_kernel().decode() if H > 256 else 'recurrent.hip, one workgroup per sequence'
                med, lo, hi = timeit(fn, a.reps)
                row[name + '_us'], row[name + '_us_min'], row[name + '_us_max'] = med, lo, hi
                row[name + '_tflops'] = flop / med / 1e6
                row[name + '_kernel'] = kern
                print('S=%3d T=%2d H=%4d %s  %9.1f (%9.1f .. %9.1f) us   %7.3f TFLOP/s f32   %s' % (
                    S, T, H, name, med, lo, hi, flop / med / 1e6, kern))
            rows.append(row)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
