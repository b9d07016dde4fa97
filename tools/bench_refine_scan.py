#!/usr/bin/env python
"""RefineNet forward + backward at B x T for the bottleneck configurations beyond the shipped one (stacked cells,
refine_net_num_features 32 / 128), with the clip-long scans on (default) and with eve_dispatch_config.cgru_scan = 0 (the
per-frame launches: what these configurations ran on before the scans covered them).  The two modes alternate on one device,
rep by rep; the table reports the median and the spread of each.  Prints a markdown table (profiles/refine_scan_widths.md).
--live-clstm measures the CLSTM cell with refine_net_clstm_feeds_features on (the differentiable scan against the per-frame
convolution + gate kernels); --scan-mode 3 scans the combinations RefineNet._use_scan leaves per frame by default."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import eve_amd  # noqa: E402
from eve_amd import synthetic as detweights  # noqa: E402  (synthetic clips and weights)
from eve_amd.kernels import default_kernels  # noqa: E402

CASES = [('CGRU', 32, 1), ('CGRU', 128, 1), ('CGRU', 64, 2), ('CRNN', 32, 1), ('CRNN', 128, 1), ('CRNN', 64, 2),
         ('CLSTM', 32, 2), ('CLSTM', 128, 1), ('CGRU', 64, 1)]
LIVE_CLSTM_CASES = [('CLSTM', 32, 1), ('CLSTM', 64, 1), ('CLSTM', 128, 1), ('CLSTM', 64, 2)]

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=32)
ap.add_argument('--seq', type=int, default=30)
ap.add_argument('--reps', type=int, default=7)
ap.add_argument('--warmup', type=int, default=2)
ap.add_argument('--dtypes', default='bf16,f32')
ap.add_argument('--live-clstm', action='store_true', help='CLSTM with refine_net_clstm_feeds_features = True')
ap.add_argument('--scan-mode', type=int, default=1, choices=(1, 3), help='eve_dispatch_config.cgru_scan of the "scans" column')
args = ap.parse_args()
DT = {'bf16': torch.bfloat16, 'f32': torch.float32, 'fp16': torch.float16}


def make(kind, width, cells, dtype):
    cfg = eve_amd.reset_standalone_config()
    cfg.import_dict({'load_screen_content': True, 'refine_net_enabled': True, 'refine_net_rnn_type': kind,
                     'refine_net_num_features': width, 'refine_net_rnn_num_cells': cells,
                     'refine_net_clstm_feeds_features': args.live_clstm})
    net = eve_amd.RefineNet()
    net.compute_dtype = dtype
    detweights.fill_module(net, seed=0)
    return net.cuda()


def one(net, batch, mode):
    with default_kernels().dispatch_override(cgru_scan=mode):
        for p in net.parameters():
            p.grad = None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        hf, _ = net.forward_sequence(batch['heatmap_initial'], batch['screen_frame'])
        (hf.float() * batch['heatmap_final_gt']).sum().backward()
        e1.record()
        torch.cuda.synchronize()
    return e0.elapsed_time(e1)


batch = {k: v.cuda() for k, v in detweights.refinenet_batch(args.batch, args.seq, seed=1).items()}
print('RefineNet forward + backward, B = %d x T = %d, ms (median [min .. max] of %d alternating reps)\n' % (args.batch, args.seq, args.reps))
print('| cell | width | cells | format | scans | per-frame (cgru_scan = 0) | per-frame / scans | scanned by default |')
print('|---|---|---|---|---|---|---|---|')
for name in args.dtypes.split(','):
    for kind, width, cells in (LIVE_CLSTM_CASES if args.live_clstm else CASES):
        net = make(kind, width, cells, DT[name])
        scanned = net._use_scan(net._rnn_cells(), (5, 8, width), DT[name])
        for _ in range(args.warmup):
            one(net, batch, args.scan_mode), one(net, batch, 0)
        ts = {1: [], 0: []}
        for _ in range(args.reps):
            for mode in (args.scan_mode, 0):
                ts[min(mode, 1)].append(one(net, batch, mode))
        f = lambda v: '%.2f [%.2f .. %.2f]' % (statistics.median(v), min(v), max(v))
        print('| %s | %d | %d | %s | %s | %s | %.2f | %s |' % (kind, width, cells, name, f(ts[1]), f(ts[0]),
                                                              statistics.median(ts[0]) / statistics.median(ts[1]),
                                                              'yes' if scanned else ('no (scanned here: cgru_scan = 3)' if args.scan_mode == 3 else
                                                                                       'no (both columns are the per-frame path)')), flush=True)
        del net
