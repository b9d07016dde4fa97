#!/usr/bin/env python
"""What per-person gaze calibration costs (eve_amd/stream.py, csrc/calibration.hip): device time per EVEStream.step under hipGraph
replay with the calibration applied, while collecting, and both, next to the plain step -- the shipped refine_net.json pipeline,
synthetic weights and clips -- and device time per eve_calib_fit launch.  One JSON line per measurement:

    python tools/bench_calibration.py --mode plain | applied | collecting | collecting-applied [--shape 32x2] [--dtype bf16]
                                      [--steps 100] [--repeat 5]
    python tools/bench_calibration.py --mode fit [--streams 32] [--samples 64 1024] [--huber 25] [--steps 100] [--repeat 5]

plain: the step of an EVEStream on which no calibration call was made (what tools/bench_stream.py measures).  applied: every
stream calibrated by set_calibration (two more eve_gaze_to_pog launches and the selects per step).  collecting: the chunk carries
calibration_target, so the step holds one eve_calib_append launch; the store is emptied before it would overflow (every 512 steps
at Tc = 2: two small selects inside the timed window).  fit: fit_calibration on 32 streams x 2 eyes with the given number of
samples per eye, noise-free scenes of tests/calib_ref.py's kind made on the device by the float32 path itself.
--repeat N: N windows in one process (`ms_runs`; `ms` is their median)."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import eve_amd  # noqa: E402
from eve_amd import synthetic as detweights  # noqa: E402

DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}
INPUT_KEYS = ('left_eye_patch', 'right_eye_patch', 'left_h', 'right_h', 'left_o', 'right_o', 'left_R', 'right_R', 'head_R',
              'camera_transformation', 'inv_camera_transformation', 'pixels_per_millimeter', 'millimeters_per_pixel', 'screen_frame')
KAPPA = (0.0436, -0.0524)                # 2.5 and -3.0 degrees


def device_ms(fn, steps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / steps


def make_model(dtype):
    cfg = eve_amd.reset_standalone_config()
    cfg.import_json(os.path.join(REPO, 'configs', 'refine_net.json'))
    cfg.import_dict({'eye_net_load_pretrained': False})
    model = eve_amd.EVE(output_predictions=True)
    model.eye_net.compute_dtype = model.refine_net.compute_dtype = dtype
    detweights.fill_module(model.eye_net, 0)
    detweights.fill_module(model.refine_net, 1)
    return model.cuda().eval()


def make_clip(B, Tc):
    small = detweights.eve_batch(min(B, 4), Tc, seed=1)
    full = {k: torch.cat([v] * ((B + 3) // 4), dim=0)[:B].contiguous().cuda() for k, v in small.items()}
    return {k: full[k] for k in INPUT_KEYS if k in full}


def bench_step(args):
    B, Tc = (int(v) for v in args.shape.split('x'))
    model, clip = make_model(DTYPES[args.dtype]), make_clip(B, Tc)
    capacity = 1024
    stream = eve_amd.EVEStream(model, B) if args.mode == 'plain' else eve_amd.EVEStream(model, B, calibration_capacity=capacity)
    if 'applied' in args.mode:
        stream.set_calibration(torch.tensor(KAPPA).expand(B, 2, 2))
    counter = [0]
    if 'collecting' in args.mode:
        clip = dict(clip, calibration_target=torch.full((B, Tc, 2), 700.0, device='cuda'))

        def step():
            counter[0] += Tc
            if counter[0] + Tc > capacity:       # keep appending, not dropping
                stream.clear_calibration_samples()
                counter[0] = 0
            stream.step(clip)
    else:
        step = lambda: stream.step(clip)
    for _ in range(3):
        step()                                   # capture + warm replays
    torch.cuda.synchronize()
    runs = sorted(round(device_ms(step, args.steps), 4) for _ in range(max(1, args.repeat)))
    res = {'mode': args.mode, 'B': B, 'Tc': Tc, 'dtype': args.dtype, 'ms': runs[len(runs) // 2], 'ms_runs': runs}
    if 'collecting' in args.mode:
        count, dropped = stream.calibration_counts()
        res['count_max'], res['dropped'] = int(count.max()), int(dropped.sum())
    print(json.dumps(res), flush=True)


def bench_fit(args):
    """Stores filled through the float32 path itself: random gaze angles, the clip's geometry, targets at KAPPA."""
    B = args.streams
    k = eve_amd.kernels.default_kernels()
    model = make_model(torch.float32)
    screen = tuple(model.config.actual_screen_size)
    for n in args.samples:
        base = make_clip(B, 8)                   # the geometry of 8 frames, repeated: the random gaze angles make the samples differ
        geo = {key: v.repeat((1, n // 8) + (1,) * (v.dim() - 2)) for key, v in base.items() if not key.endswith(('_patch', 'screen_frame'))}
        N = B * n
        flat = lambda key, *s: geo[key].reshape((N,) + s).float().contiguous()
        gen = torch.Generator(device='cuda').manual_seed(n)
        stream = eve_amd.EVEStream(model, B, use_graph=False, calibration_capacity=n)
        samples, count, dropped = stream._store()
        g = [(torch.rand((N, 2), generator=gen, device='cuda') - 0.5) * 0.5 for _ in range(2)]
        kap = torch.tensor(KAPPA, device='cuda').expand(N, 2).contiguous()
        _, mm, _, _ = k.gaze_to_pog(g[0], flat('left_o', 3), flat('left_R', 3, 3), flat('inv_camera_transformation', 4, 4),
                                    flat('pixels_per_millimeter', 2), screen, flat('head_R', 3, 3), kap)
        target = (mm * flat('pixels_per_millimeter', 2)).view(B, n, 2).contiguous()
        five = lambda key, *s: torch.stack([geo['left' + key], geo['right' + key]]).reshape((2, B, n) + s).float().contiguous()
        k.calib_append(torch.stack(g).view(2, B, n, 2).contiguous(), geo['head_R'].float().contiguous(), five('_o', 3), five('_R', 3, 3),
                       geo['inv_camera_transformation'].float().contiguous(), geo['pixels_per_millimeter'].float().contiguous(), target,
                       samples, count, dropped)
        fit = lambda: stream.fit_calibration(huber_mm=args.huber)
        out = fit()
        torch.cuda.synchronize()
        runs = sorted(round(1e3 * device_ms(fit, args.steps), 2) for _ in range(max(1, args.repeat)))
        print(json.dumps({'mode': 'fit', 'streams': B, 'eyes': 2, 'samples': n, 'huber_mm': args.huber, 'us': runs[len(runs) // 2], 'us_runs': runs,
                          'count_min': int(count.min()), 'ok': int(out['ok'].sum()), 'rms_mm_max': float(out['rms_mm'].max()),
                          'left_kappa_error_max': float((out['kappa'][:, 0] - torch.tensor(KAPPA, device='cuda', dtype=torch.float64)).abs().max())}),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', required=True, choices=('plain', 'applied', 'collecting', 'collecting-applied', 'fit'))
    ap.add_argument('--shape', default='32x2')
    ap.add_argument('--dtype', default='bf16', choices=sorted(DTYPES))
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--streams', type=int, default=32)
    ap.add_argument('--samples', type=int, nargs='+', default=[64, 1024], help='per eye; multiples of 8')
    ap.add_argument('--huber', type=float, default=None)
    args = ap.parse_args()
    with torch.no_grad():
        bench_fit(args) if args.mode == 'fit' else bench_step(args)


if __name__ == '__main__':
    main()
