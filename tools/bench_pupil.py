#!/usr/bin/env python
"""Device time of the pupillometry launch (eve_pupil_track) and of the EVEStream step with and without pupil=.  One JSON line per
measurement:

    python tools/bench_pupil.py [--shape 32x2] [--reps 50] [--step [--dtype bf16] [--steps 100] [--repeat 5]]

Kernel: B x T frames of pupil sizes that wander around 4 mm, counted time at 30 fps, two cases -- `bare`: the two sizes and eye_valid;
`light_marks`: with pupil_luminance and pupil_baseline as well.  A captured chain of 32 launches, replayed `reps` times under device
events: `pupil_us` per launch.  `aoi_rect8_us` is eve_gaze_aoi's 8-rectangle case of tools/bench_aoi.py and `launch_floor_us` the time
per launch of a chain of smallest launches, both in the same process.
--step: the shipped refine_net.json pipeline at `--shape`, captured; windows of `steps` replays with pupil=PupilSpec(fps=30) and
without alternate on one EVEStream, `repeat` windows each (`step_ms`, `plain_step_ms`: the medians; `pupil_delta_us`)."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tools'))
import eve_amd  # noqa: E402
from bench_aoi import kernel_line as aoi_line, rect_grid  # noqa: E402
from bench_gaze_history import chain_us  # noqa: E402
from bench_stream import DTYPES, INPUT_KEYS, detweights, device_ms, launch_floor_us  # noqa: E402
from eve_amd import data  # noqa: E402


def kernel_line(name, B, T, full, reps):
    k = eve_amd.kernels.default_kernels()
    spec = eve_amd.PupilSpec(fps=30.0, baseline_tau_s=None if full else 10.0)
    g = torch.Generator().manual_seed(T)
    size = (4.0 + 0.05 * torch.randn((2, B, T), generator=g).cumsum(dim=2)).cuda()
    eye_valid = (torch.rand((B, T, 2), generator=g) > 0.1).to(torch.uint8).cuda()
    more = {}
    if full:
        more = {'luminance': (40.0 + 10.0 * torch.rand((B, T), generator=g)).cuda(), 'baseline_mark': (torch.rand((B, T), generator=g) > 0.5).to(torch.uint8).cuda()}
    buffers = data.pupil_buffers(B, 256, 'cuda')
    out = k.pupil_track(size, spec, *buffers, eye_valid=eye_valid, **more)
    samples = float(out['valid'].float().mean())
    us = chain_us(lambda: k.pupil_track(size, spec, *buffers, eye_valid=eye_valid, **more), reps)
    return {'case': name, 'B': B, 'T': T, 'pupil_us': us, 'frames_that_are_samples': round(samples, 3)}


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
    spec = eve_amd.PupilSpec(fps=30, min_mm=1e-3, max_mm=1e3, max_speed_mm_s=1e6)      # (an untrained head's sizes: let them through)
    step, plain = (lambda: stream.step(clip, pupil=spec)), (lambda: stream.step(clip))
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
    res['pupil_delta_us'] = round(1e3 * (res['step_ms'] - res['plain_step_ms']), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', default='32x2')
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--step', action='store_true', help='also the EVEStream step with and without pupil=')
    ap.add_argument('--dtype', default='bf16', choices=sorted(DTYPES))
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--repeat', type=int, default=5)
    args = ap.parse_args()
    B, T = (int(v) for v in args.shape.split('x'))
    print(json.dumps(kernel_line('bare', B, T, False, args.reps)), flush=True)
    print(json.dumps(kernel_line('light_marks', B, T, True, args.reps)), flush=True)
    rect8 = data.aoi_shapes(rect_grid(4, 2), 8)[None].repeat(B, 1, 1).cuda()
    print(json.dumps({'aoi_rect8_us': aoi_line('rect8', B, T, rect8, args.reps)['aoi_us']}), flush=True)
    print(json.dumps({'launch_floor_us': launch_floor_us()}), flush=True)
    if args.step:
        print(json.dumps(step_line(B, T, args.dtype, args.steps, args.repeat)), flush=True)


if __name__ == '__main__':
    main()
