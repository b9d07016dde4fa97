#!/usr/bin/env python
"""Device time of the gaze history's two launches (eve_gaze_history_plan, eve_gaze_history_update) and of the EVEStream step with and
without history=.  One JSON line per measurement:

    python tools/bench_gaze_history.py [--sizes 128x72 480x270 960x540] [--shape 32x2] [--reps 50] [--step [--dtype bf16] [--steps 100] [--repeat 5]]

Kernels: per map size, B x T frames of random points of gaze; a captured chain of 32 launches of each kernel, replayed `reps` times
under device events: `plan_us` and `update_us` per launch, plain, with per_frame (`update_frames_us`) and, at the first size, with the
heat source (`update_heat_us`).  `bytes` is what the update launch must move -- one read and one write of the maps, 2 * B * MH * MW * 4,
plus B * T * MH * MW * 4 per extra (the per-frame maps written, the heat maps read) -- and `hbm_fraction` that over the time over 8 TB/s.
`launch_floor_us` is the time per launch of a chain of smallest launches in the same process.
--step: the shipped refine_net.json pipeline at `--shape`, captured; windows of `steps` replays with history=GazeHistorySpec(fps=30) and
without alternate on one EVEStream, `repeat` windows each (`step_ms`, `plain_step_ms`: the medians; `history_delta_us`)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tools'))
import eve_amd  # noqa: E402
from bench_stream import DTYPES, INPUT_KEYS, detweights, device_ms, launch_floor_us  # noqa: E402

HBM_BYTES_PER_S = 8e12
CHAIN = 32


def chain_us(run, reps):
    """Device time per call of a replayed hipGraph of CHAIN calls of run()."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(CHAIN):
            run()
    graph.replay()
    torch.cuda.synchronize()
    return round(1e3 * device_ms(graph.replay, reps) / CHAIN, 3)


def kernels_line(B, T, size, reps, with_heat):
    k = eve_amd.kernels.default_kernels()
    MW, MH = size
    spec = eve_amd.GazeHistorySpec(size=size, sigma=3.0 * MW / 128.0, decay_per_ms=0.999, fps=30.0)
    P = spec.launch_params()
    g = torch.Generator().manual_seed(MW)
    pog = (torch.rand((B, T, 2), generator=g) * torch.tensor([1920.0, 1080.0])).cuda()
    state = torch.zeros((B, 8), dtype=torch.float64, device='cuda')
    maps = torch.zeros((B, MH, MW), dtype=torch.float32, device='cuda')
    coef, clear = k.gaze_history_plan(P, (1920, 1080), state, T, pog=pog)
    res = {'B': B, 'T': T, 'size': '%dx%d' % size,
           'plan_us': chain_us(lambda: k.gaze_history_plan(P, (1920, 1080), state, T, pog=pog), reps)}
    plane = B * MH * MW * 4
    cases = [('update', dict(), 2 * plane), ('update_frames', dict(per_frame=True), (2 + T) * plane)]
    if with_heat:
        heat = torch.rand((B, T, MH, MW), generator=g).cuda()
        cases.append(('update_heat', dict(heat=heat), (2 + T) * plane))
    for name, kw, nbytes in cases:
        us = chain_us(lambda: k.gaze_history_update(P, coef, clear, maps, **kw), reps)
        res[name + '_us'], res[name + '_bytes'], res[name + '_hbm_fraction'] = us, nbytes, round(nbytes / (us * 1e-6) / HBM_BYTES_PER_S, 4)
    assert bool(torch.isfinite(maps).all())
    return res


def step_line(B, Tc, dtype, steps, repeat):
    cfg = eve_amd.reset_standalone_config()
    cfg.import_json(os.path.join(REPO, 'configs', 'refine_net.json'))
    cfg.import_dict({'eye_net_load_pretrained': False})
    model = eve_amd.EVE(output_predictions=True)
    model.eye_net.compute_dtype = model.refine_net.compute_dtype = DTYPES[dtype]
    detweights.fill_module(model.eye_net, 0)
    detweights.fill_module(model.refine_net, 1)
    model = model.cuda().eval()
    small = detweights.eve_batch(min(B, 4), Tc, seed=1)
    full = {k: torch.cat([v] * ((B + 3) // 4), dim=0)[:B].contiguous().cuda() for k, v in small.items()}
    clip = {k: full[k] for k in INPUT_KEYS if k in full}
    stream = eve_amd.EVEStream(model, B)
    spec = eve_amd.GazeHistorySpec(fps=30)
    step, plain = (lambda: stream.step(clip, history=spec)), (lambda: stream.step(clip))
    for fn in (step, plain):
        for _ in range(3):
            fn()                                             # capture + warm replays
    torch.cuda.synchronize()
    runs, plain_runs = [], []
    for _ in range(max(1, repeat)):
        plain_runs.append(round(device_ms(plain, steps), 4))
        runs.append(round(device_ms(step, steps), 4))
    runs, plain_runs = sorted(runs), sorted(plain_runs)
    res = {'B': B, 'Tc': Tc, 'dtype': dtype, 'size': '%dx%d' % tuple(cfg.gaze_heatmap_size), 'step_ms': runs[len(runs) // 2],
           'plain_step_ms': plain_runs[len(plain_runs) // 2], 'step_ms_runs': runs, 'plain_step_ms_runs': plain_runs}
    res['history_delta_us'] = round(1e3 * (res['step_ms'] - res['plain_step_ms']), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', nargs='+', default=['128x72', '480x270', '960x540'])
    ap.add_argument('--shape', default='32x2')
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--step', action='store_true', help='also the EVEStream step with and without history=')
    ap.add_argument('--dtype', default='bf16', choices=sorted(DTYPES))
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--repeat', type=int, default=5)
    args = ap.parse_args()
    B, T = (int(v) for v in args.shape.split('x'))
    for i, s_ in enumerate(args.sizes):
        size = tuple(int(v) for v in s_.lower().split('x'))
        print(json.dumps(kernels_line(B, T, size, args.reps, with_heat=i == 0)), flush=True)
    print(json.dumps({'launch_floor_us': launch_floor_us()}), flush=True)
    if args.step:
        print(json.dumps(step_line(B, T, args.dtype, args.steps, args.repeat)), flush=True)


if __name__ == '__main__':
    main()
