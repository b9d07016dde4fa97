#!/usr/bin/env python
"""Device time of the areas-of-interest launch (eve_gaze_aoi) and of the EVEStream step with and without aoi=.  One JSON line per
measurement:

    python tools/bench_aoi.py [--shape 32x2] [--reps 50] [--step [--dtype bf16] [--steps 100] [--repeat 5]]

Kernel: B x T frames of random points of gaze on a 1920 x 1080 screen, counted time at 30 fps, two cases -- `rect8`: 8 static
rectangles (a 4 x 2 grid of tiles, shapes [B, 8, 36]); `poly64_dynamic`: 64 polygons of 16 vertices, one table per frame (shapes
[B, T, 64, 36], an 8 x 8 grid of 16-gons).  A captured chain of 32 launches, replayed `reps` times under device events: `aoi_us` per
launch.  `launch_floor_us` is the time per launch of a chain of smallest launches in the same process.
--step: the shipped refine_net.json pipeline at `--shape`, captured; windows of `steps` replays with aoi=AoiSpec(num_aois=8, fps=30)
and without alternate on one EVEStream, `repeat` windows each (`step_ms`, `plain_step_ms`: the medians; `aoi_delta_us`)."""
import argparse
import json
import math
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tools'))
import eve_amd  # noqa: E402
from bench_gaze_history import chain_us  # noqa: E402
from bench_stream import DTYPES, INPUT_KEYS, detweights, device_ms, launch_floor_us  # noqa: E402
from eve_amd import data  # noqa: E402

W, H = 1920.0, 1080.0


def rect_grid(nx, ny):
    return [('rect', W * i / nx, H * j / ny, W * (i + 1) / nx, H * (j + 1) / ny) for j in range(ny) for i in range(nx)]


def polygon_grid(nx, ny, vertices=16):
    cells = []
    for j in range(ny):
        for i in range(nx):
            cx, cy, rx, ry = W * (i + 0.5) / nx, H * (j + 0.5) / ny, 0.5 * W / nx, 0.5 * H / ny
            cells.append(('polygon', [(cx + rx * math.cos(2 * math.pi * v / vertices), cy + ry * math.sin(2 * math.pi * v / vertices))
                                      for v in range(vertices)]))
    return cells


def kernel_line(name, B, T, shapes, reps):
    k = eve_amd.kernels.default_kernels()
    A = shapes.shape[-2]
    spec = eve_amd.AoiSpec(num_aois=A, fps=30.0)
    g = torch.Generator().manual_seed(A)
    pog = (torch.rand((B, T, 2), generator=g) * torch.tensor([W, H])).cuda()
    buffers = data.aoi_buffers(B, A, 256, 'cuda')
    out = k.gaze_aoi(pog, shapes, spec, *buffers)
    hit = float((out['id'] >= 0).float().mean())
    us = chain_us(lambda: k.gaze_aoi(pog, shapes, spec, *buffers), reps)
    return {'case': name, 'B': B, 'T': T, 'A': A, 'per_frame_shapes': shapes.dim() == 4, 'aoi_us': us, 'frames_inside_an_aoi': round(hit, 3)}


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
    with_shapes = dict(clip, aoi_shapes=data.aoi_shapes(rect_grid(4, 2), 8)[None].repeat(B, 1, 1).cuda())
    stream = eve_amd.EVEStream(model, B)
    spec = eve_amd.AoiSpec(num_aois=8, fps=30)
    step, plain = (lambda: stream.step(with_shapes, aoi=spec)), (lambda: stream.step(clip))
    for fn in (step, plain):
        for _ in range(3):
            fn()                                             # capture + warm replays
    torch.cuda.synchronize()
    runs, plain_runs = [], []
    for _ in range(max(1, repeat)):
        plain_runs.append(round(device_ms(plain, steps), 4))
        runs.append(round(device_ms(step, steps), 4))
    runs, plain_runs = sorted(runs), sorted(plain_runs)
    res = {'B': B, 'Tc': Tc, 'dtype': dtype, 'step_ms': runs[len(runs) // 2], 'plain_step_ms': plain_runs[len(plain_runs) // 2],
           'step_ms_runs': runs, 'plain_step_ms_runs': plain_runs}
    res['aoi_delta_us'] = round(1e3 * (res['step_ms'] - res['plain_step_ms']), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', default='32x2')
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--step', action='store_true', help='also the EVEStream step with and without aoi=')
    ap.add_argument('--dtype', default='bf16', choices=sorted(DTYPES))
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--repeat', type=int, default=5)
    args = ap.parse_args()
    B, T = (int(v) for v in args.shape.split('x'))
    rect8 = data.aoi_shapes(rect_grid(4, 2), 8)[None].repeat(B, 1, 1).cuda()
    poly64 = data.aoi_shapes(polygon_grid(8, 8), 64)[None, None].repeat(B, T, 1, 1).contiguous().cuda()
    print(json.dumps(kernel_line('rect8', B, T, rect8, args.reps)), flush=True)
    print(json.dumps(kernel_line('poly64_dynamic', B, T, poly64, args.reps)), flush=True)
    print(json.dumps({'launch_floor_us': launch_floor_us()}), flush=True)
    if args.step:
        print(json.dumps(step_line(B, T, args.dtype, args.steps, args.repeat)), flush=True)


if __name__ == '__main__':
    main()
