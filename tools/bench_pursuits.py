#!/usr/bin/env python
"""Device time of the smooth-pursuit launch (eve_gaze_pursuits) beside eve_gaze_saccades and eve_gaze_events, and of the EVEStream
step with events= and pursuits= against the step with events= alone.  One JSON line per measurement:

    python tools/bench_pursuits.py [--shapes 32x2 32x64] [--reps 50] [--step [--shape 32x2] [--dtype bf16] [--steps 100] [--repeat 5]]

Kernels: B x T frames per stream of a point that follows a target -- a third of a second at rest, two thirds at 5 .. 15 degrees /
second in a direction of its own, with a tenth of a degree of jitter and a 10 degree jump every 150 frames or so, 120 fps counted
time, the velocity from the filtered point, an eye 600 mm from the screen -- and the target itself.  Per shape a captured chain of 32
launches, replayed `reps` times under device events: `pursuits_us` and `pursuits_no_target_us` (on the _ex arrays of the path's first
launch; the chain carries the state row on, the store fills and then drops; the default PursuitSpec, but with T below 32 a
min_window_s of half a frame, so that the chain's repeated frames still fill windows), `saccades_us` (on the same arrays), `events_us` and
`events_ex_us`, and `launch_floor_us`, the time per launch of a chain of smallest launches, all in the same process.
--step: the shipped refine_net.json pipeline at --shape, captured; windows of `steps` replays with events=GazeEventSpec(fps=30) plus
pursuits=PursuitSpec(), with events= plus saccades= plus pursuits=, and with events= alone alternate, `repeat` windows each:
`step_ms`, `both_step_ms`, `events_step_ms` (the medians; the `_runs` lists are the run-to-run spread), `pursuits_delta_us` and
`both_delta_us`."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tools'))
import eve_amd  # noqa: E402
from bench_gaze_history import chain_us  # noqa: E402
from bench_stream import DTYPES, INPUT_KEYS, detweights, device_ms, launch_floor_us  # noqa: E402
from eve_amd import data, kernels  # noqa: E402

DEG_PX = 600.0 * math.tan(math.radians(1.0)) * 3.6       # one degree on the screen under the eye, in pixels


def pursuit_paths(B, T, fps=120.0, seed=3):
    """-> (pog [B, T, 2], o, inv_cam, ppm, target [B, T, 2]) float32 on the GPU."""
    g = np.random.default_rng(seed)
    pog, target = np.zeros((B, T, 2), dtype=np.float32), np.zeros((B, T, 2), dtype=np.float32)
    for b in range(B):
        p = g.uniform([600, 400], [1200, 700])
        heading, speed = g.uniform(0, 2 * math.pi), g.uniform(5.0, 15.0)
        for t in range(T):
            phase = (t + 7 * b) % 120
            if phase >= 40:                              # two thirds of a second of motion
                p = p + speed * DEG_PX / fps * np.array([math.cos(heading), math.sin(heading)])
            if phase == 0:
                heading, speed = g.uniform(0, 2 * math.pi), g.uniform(5.0, 15.0)
            if (t + 11 * b) % 150 == 149:                # a jump back towards the middle of the screen
                p = np.array([900.0, 550.0]) + g.uniform(-1, 1, 2) * 10 * DEG_PX
            target[b, t] = p
            pog[b, t] = p + g.uniform(-1, 1, 2) * 0.1 * DEG_PX / math.sqrt(2.0)
    o = np.tile(np.array([265.0, 150.0, 600.0], dtype=np.float32), (B, T, 1))
    inv_cam = np.tile(np.eye(4, dtype=np.float32), (B, T, 1, 1))
    return tuple(torch.from_numpy(a).cuda() for a in (pog, o, inv_cam, np.full((B, T, 2), 3.6, dtype=np.float32), target))


def kernel_line(B, T, reps):
    k = kernels.default_kernels()
    # (a chain repeats its T frames, so with T below the 12 frames of min_window_s no window would ever fill and the launch would
    # skip its atan2: the short shapes take a min_window_s of half a frame, with which every other repeated frame has a window)
    spec, sspec = eve_amd.GazeEventSpec(fps=120.0), eve_amd.SaccadeSpec()
    pspec = eve_amd.PursuitSpec() if T >= 32 else eve_amd.PursuitSpec(min_window_s=0.5 / 120.0)
    pog, o, inv_cam, ppm, target = pursuit_paths(B, T)
    z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device='cuda')
    events = lambda: (z(B, 32), z(B, 256, 8), z(B, dtype=torch.int32), z(B, dtype=torch.int32))
    res = k.gaze_events_ex(pog, o, inv_cam, ppm, spec, *events())
    frames = [res['sample'], res['sample_time'], res['gaze_vector'], res['PoG_px_filtered'], res['gaze_event'], res['gaze_velocity'],
              res['fixation_id']]
    buffers, bare, saccades = data.pursuit_buffers(B, 256, 'cuda'), data.pursuit_buffers(B, 256, 'cuda'), data.saccade_buffers(B, 256, 'cuda')
    first = k.gaze_pursuits(*frames, pspec, *buffers, target=target)
    again = k.gaze_pursuits(*frames, pspec, *buffers, target=target)      # (what every later launch of the chain sees: the ring of the one before)
    line = {'B': B, 'T': T, 'pursuit_frames': round(float((first['gaze_class'] == 3).float().mean()), 3),
            'saccade_frames': round(float((res['gaze_event'] == 2).float().mean()), 3),
            'windowed_frames': round(float(torch.isfinite(first['gaze_velocity_windowed']).float().mean()), 3),
            'windowed_frames_in_chain': round(float(torch.isfinite(again['gaze_velocity_windowed']).float().mean()), 3),
            'episodes_per_stream': round(float(buffers[1][:, 0].mean()), 2)}
    line['pursuits_us'] = chain_us(lambda: k.gaze_pursuits(*frames, pspec, *buffers, target=target), reps)
    line['pursuits_no_target_us'] = chain_us(lambda: k.gaze_pursuits(*frames, pspec, *bare), reps)
    line['saccades_us'] = chain_us(lambda: k.gaze_saccades(*frames, sspec, *saccades), reps)
    plain, ex = events(), events()
    line['events_us'] = chain_us(lambda: k.gaze_events(pog, o, inv_cam, ppm, spec, *plain), reps)
    line['events_ex_us'] = chain_us(lambda: k.gaze_events_ex(pog, o, inv_cam, ppm, spec, *ex), reps)
    return line


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
    spec, sspec, pspec = eve_amd.GazeEventSpec(fps=30), eve_amd.SaccadeSpec(), eve_amd.PursuitSpec()
    with_pursuits, with_both, events_only = eve_amd.EVEStream(model, B), eve_amd.EVEStream(model, B), eve_amd.EVEStream(model, B)
    fns = {'step_ms': lambda: with_pursuits.step(clip, events=spec, pursuits=pspec),
           'both_step_ms': lambda: with_both.step(clip, events=spec, saccades=sspec, pursuits=pspec),
           'events_step_ms': lambda: events_only.step(clip, events=spec)}
    for fn in fns.values():
        for _ in range(3):
            fn()                                             # capture + warm replays
    torch.cuda.synchronize()
    runs = {name: [] for name in fns}
    for _ in range(max(1, repeat)):
        for name in sorted(fns):
            runs[name].append(round(device_ms(fns[name], steps), 4))
    res = {'B': B, 'Tc': Tc, 'dtype': dtype}
    for name, r in runs.items():
        res[name], res[name + '_runs'] = sorted(r)[len(r) // 2], sorted(r)
    res['pursuits_delta_us'] = round(1e3 * (res['step_ms'] - res['events_step_ms']), 2)
    res['both_delta_us'] = round(1e3 * (res['both_step_ms'] - res['events_step_ms']), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', nargs='+', default=['32x2', '32x64'])
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--step', action='store_true', help='also the EVEStream step with events= and pursuits= against events= alone')
    ap.add_argument('--shape', default='32x2', help='the shape of --step')
    ap.add_argument('--dtype', default='bf16', choices=sorted(DTYPES))
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--repeat', type=int, default=5)
    args = ap.parse_args()
    for shape in args.shapes:
        B, T = (int(v) for v in shape.split('x'))
        print(json.dumps(kernel_line(B, T, args.reps)), flush=True)
    print(json.dumps({'launch_floor_us': launch_floor_us()}), flush=True)
    if args.step:
        B, T = (int(v) for v in args.shape.split('x'))
        print(json.dumps(step_line(B, T, args.dtype, args.steps, args.repeat)), flush=True)


if __name__ == '__main__':
    main()
