#!/usr/bin/env python
"""Device time of the saccade launch (eve_gaze_saccades) beside its neighbours, of eve_gaze_events_ex against eve_gaze_events, and of
the EVEStream step with events= and saccades= against the step with events= alone.  One JSON line per measurement:

    python tools/bench_saccades.py [--shapes 32x2 32x64] [--reps 50] [--step [--shape 32x2] [--dtype bf16] [--steps 100] [--repeat 5]
                                   [--parent-lib PATH]]

Kernels: B x T frames of a synthetic scan path per stream -- fixations of 6 frames with half a pixel of jitter, 2-frame saccades of a
few hundred pixels between them, 120 fps counted time, the velocity from the raw point, an eye 600 mm from the screen.  Per shape a
captured chain of 32 launches, replayed `reps` times under device events: `saccades_us` (on the _ex arrays of the path's first launch;
the chain carries the state row on, the store fills and then drops), `events_us` and `events_ex_us` (the same chain through either
entry: what the three guarded stores cost), `aoi_rect8_us` (eve_gaze_aoi's 8-rectangle case of tools/bench_aoi.py) and
`launch_floor_us`, the time per launch of a chain of smallest launches, all in the same process.
--step: the shipped refine_net.json pipeline at --shape, captured; windows of `steps` replays with events=GazeEventSpec(fps=30) plus
saccades=SaccadeSpec(), with events= alone, and -- with --parent-lib, a libeve_hip.so built from the parent commit's sources -- with
events= alone on that library (a second kernels object in the same process, its own EVEStream and graph) alternate, `repeat` windows
each: `step_ms`, `events_step_ms`, `parent_events_step_ms` (the medians; the `_runs` lists are the run-to-run spread),
`saccades_delta_us` and `events_vs_parent_us`."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tools'))
import eve_amd  # noqa: E402
from bench_aoi import kernel_line as aoi_line, rect_grid  # noqa: E402
from bench_gaze_history import chain_us  # noqa: E402
from bench_stream import DTYPES, INPUT_KEYS, detweights, device_ms, launch_floor_us  # noqa: E402
from eve_amd import _lib, data, kernels  # noqa: E402


def scan_paths(B, T, seed=3):
    """-> (pog [B, T, 2], o, inv_cam, ppm) float32 on the GPU."""
    g = np.random.default_rng(seed)
    pog = np.zeros((B, T, 2), dtype=np.float32)
    for b in range(B):
        p, target, left = g.uniform([300, 200], [1600, 900]), None, 0
        for t in range(T):
            if (t + b) % 8 == 6:
                target, left = g.uniform([300, 200], [1600, 900]), 2
            if left:
                p, left = p + (target - p) / left, left - 1
            pog[b, t] = p + (g.uniform(-0.5, 0.5, 2) if not left else 0.0)
    o = np.tile(np.array([265.0, 150.0, 600.0], dtype=np.float32), (B, T, 1))
    inv_cam = np.tile(np.eye(4, dtype=np.float32), (B, T, 1, 1))
    return tuple(torch.from_numpy(a).cuda() for a in (pog, o, inv_cam, np.full((B, T, 2), 3.6, dtype=np.float32)))


def kernel_line(B, T, reps):
    k = kernels.default_kernels()
    spec, sspec = eve_amd.GazeEventSpec(fps=120.0, velocity_from='raw'), eve_amd.SaccadeSpec()
    pog, o, inv_cam, ppm = scan_paths(B, T)
    z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device='cuda')
    events = lambda: (z(B, 32), z(B, 256, 8), z(B, dtype=torch.int32), z(B, dtype=torch.int32))
    res = k.gaze_events_ex(pog, o, inv_cam, ppm, spec, *events())
    frames = [res['sample'], res['sample_time'], res['gaze_vector'], pog, res['gaze_event'], res['gaze_velocity'], res['fixation_id']]
    buffers = data.saccade_buffers(B, 256, 'cuda')
    k.gaze_saccades(*frames, sspec, *buffers)
    line = {'B': B, 'T': T, 'saccade_frames': round(float((res['gaze_event'] == 2).float().mean()), 3),
            'saccades_per_stream': round(float(buffers[1][:, 0].mean()), 2)}
    line['saccades_us'] = chain_us(lambda: k.gaze_saccades(*frames, sspec, *buffers), reps)
    plain, ex = events(), events()
    line['events_us'] = chain_us(lambda: k.gaze_events(pog, o, inv_cam, ppm, spec, *plain), reps)
    line['events_ex_us'] = chain_us(lambda: k.gaze_events_ex(pog, o, inv_cam, ppm, spec, *ex), reps)
    rect8 = data.aoi_shapes(rect_grid(4, 2), 8)[None].repeat(B, 1, 1).cuda()
    line['aoi_rect8_us'] = aoi_line('rect8', B, T, rect8, reps)['aoi_us']
    return line


def library_kernels(path):
    """A second kernels object on another build of the library (the parent commit's): the entry points it has, typed."""
    lib = ctypes.CDLL(path)
    for name, argtypes in _lib.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.argtypes, fn.restype = argtypes, ctypes.c_int
    lib.eve_stem_bwd_wgrad_workspace.restype = ctypes.c_ulonglong
    lib.eve_last_kernel.restype = lib.eve_last_error.restype = ctypes.c_char_p
    k = kernels.HipKernels()
    k.lib = lib
    return k


def step_line(B, Tc, dtype, steps, repeat, parent_lib):
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
    spec, sspec = eve_amd.GazeEventSpec(fps=30), eve_amd.SaccadeSpec()
    with_saccades, events_only = eve_amd.EVEStream(model, B), eve_amd.EVEStream(model, B)
    fns = {'step_ms': lambda: with_saccades.step(clip, events=spec, saccades=sspec), 'events_step_ms': lambda: events_only.step(clip, events=spec)}
    for fn in fns.values():
        for _ in range(3):
            fn()                                             # capture + warm replays
    if parent_lib:
        parent_stream = eve_amd.EVEStream(model, B)
        fns['parent_events_step_ms'] = lambda: parent_stream.step(clip, events=spec)
        kernels.set_default_kernels(library_kernels(parent_lib))      # its graph is captured on the parent's library; a replay calls neither
        try:
            for _ in range(3):
                fns['parent_events_step_ms']()
        finally:
            kernels.set_default_kernels(None)
    torch.cuda.synchronize()
    runs = {name: [] for name in fns}
    for _ in range(max(1, repeat)):
        for name in sorted(fns):
            runs[name].append(round(device_ms(fns[name], steps), 4))
    res = {'B': B, 'Tc': Tc, 'dtype': dtype}
    for name, r in runs.items():
        res[name], res[name + '_runs'] = sorted(r)[len(r) // 2], sorted(r)
    res['saccades_delta_us'] = round(1e3 * (res['step_ms'] - res['events_step_ms']), 2)
    if parent_lib:
        res['events_vs_parent_us'] = round(1e3 * (res['events_step_ms'] - res['parent_events_step_ms']), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', nargs='+', default=['32x2', '32x64'])
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--step', action='store_true', help='also the EVEStream step with events= and saccades= against events= alone')
    ap.add_argument('--shape', default='32x2', help='the shape of --step')
    ap.add_argument('--dtype', default='bf16', choices=sorted(DTYPES))
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--parent-lib', default=None, help='a libeve_hip.so built from the parent commit: its events= step joins the alternation')
    args = ap.parse_args()
    for shape in args.shapes:
        B, T = (int(v) for v in shape.split('x'))
        print(json.dumps(kernel_line(B, T, args.reps)), flush=True)
    print(json.dumps({'launch_floor_us': launch_floor_us()}), flush=True)
    if args.step:
        B, T = (int(v) for v in args.shape.split('x'))
        print(json.dumps(step_line(B, T, args.dtype, args.steps, args.repeat, args.parent_lib)), flush=True)


if __name__ == '__main__':
    main()
