#!/usr/bin/env python
"""What per-person gaze calibration costs (eve_amd/stream.py, csrc/calibration.hip): device time per EVEStream.step under hipGraph
replay with the calibration applied, while collecting, and both, next to the plain step -- the shipped refine_net.json pipeline,
synthetic weights and clips -- and device time per eve_calib_fit launch.  One JSON line per measurement:

    python tools/bench_calibration.py --mode plain | applied | collecting | collecting-applied [--shape 32x2] [--dtype bf16]
                                      [--steps 100] [--repeat 5]
    python tools/bench_calibration.py --mode fit [--streams 32] [--samples 64 1024] [--huber 25] [--steps 100] [--repeat 5]
    python tools/bench_calibration.py --mode screen-applied | screen-collecting [--shape 32x2] [--dtype bf16]
    python tools/bench_calibration.py --mode screen-fit [--model offset | affine | quadratic] [--streams 32] [--samples 64 1024] [--huber 25]

plain: the step of an EVEStream on which no calibration call was made (what tools/bench_stream.py measures).  applied: every
stream calibrated by set_calibration (two more eve_gaze_to_pog launches and the selects per step).  collecting: the chunk carries
calibration_target, so the step holds one eve_calib_append launch; the store is emptied before it would overflow (every 512 steps
at Tc = 2: two small selects inside the timed window).  fit: fit_calibration on 32 streams x 2 eyes with the given number of
samples per eye, noise-free scenes of tests/calib_ref.py's kind made on the device by the float32 path itself.
screen-applied: every stream holds an affine screen-space map (set_screen_calibration): one eve_screen_calib_apply launch, PoG_cm and
g recomputed and selected per stream.  screen-collecting: the chunk carries screen_calibration_target, so the step holds one
eve_screen_calib_append launch (the store emptied as above).  screen-fit: fit_screen_calibration on 32 streams with the given number
of samples per stream: a 5 x 3 grid of dots, 8 mm of Gaussian noise, every tenth sample moved 80 .. 200 mm, made on the device.
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
SCREEN_COEF = ((9.0, -12.0, 7.0, 11.0, -8.0, 6.0), (-10.0, 8.0, 12.0, -7.0, 9.0, -11.0))      # a screen-space map, millimetres per term


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
    screen = args.mode.startswith('screen-')
    stream = eve_amd.EVEStream(model, B) if args.mode == 'plain' else eve_amd.EVEStream(model, B, calibration_capacity=capacity,
                                                                                      screen_calibration_capacity=capacity)
    if args.mode == 'screen-applied':
        coef = torch.zeros((B, 2, 6), dtype=torch.float64)
        coef[:, :, :3] = torch.tensor(SCREEN_COEF, dtype=torch.float64)[:, :3]
        stream.set_screen_calibration(coef, [2] * B)
    elif 'applied' in args.mode:
        stream.set_calibration(torch.tensor(KAPPA).expand(B, 2, 2))
    counter = [0]
    if 'collecting' in args.mode:
        clip = dict(clip, **{('screen_' if screen else '') + 'calibration_target': torch.full((B, Tc, 2), 700.0, device='cuda')})
        clear = stream.clear_screen_calibration_samples if screen else stream.clear_calibration_samples

        def step():
            counter[0] += Tc
            if counter[0] + Tc > capacity:       # keep appending, not dropping
                clear()
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
        count, dropped = stream.screen_calibration_counts() if screen else stream.calibration_counts()
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


def bench_screen_fit(args):
    """Stores filled by eve_screen_calib_append: dots on a 5 x 3 grid, the raw points the dots moved back by the known map's value at
    the dot (SCREEN_COEF cut to the model's terms) plus 8 mm of noise, every tenth sample moved 80 .. 200 mm."""
    B, kind = args.streams, {'offset': 1, 'affine': 2, 'quadratic': 3}[args.model]
    K = (0, 1, 3, 6)[kind]
    k = eve_amd.kernels.default_kernels()
    model = make_model(torch.float32)
    W, H = (float(v) for v in model.config.actual_screen_size)
    star = torch.zeros((2, 6), dtype=torch.float64, device='cuda')
    star[:, :K] = torch.tensor(SCREEN_COEF, dtype=torch.float64, device='cuda')[:, :K]
    for n in args.samples:
        base = make_clip(B, 8)
        geo = {key: v.repeat((1, n // 8) + (1,) * (v.dim() - 2)).float().contiguous() for key, v in base.items()
               if key in ('left_o', 'right_o', 'inv_camera_transformation', 'pixels_per_millimeter')}
        gen = torch.Generator(device='cuda').manual_seed(n)
        i = torch.arange(n, device='cuda')
        dots = torch.stack([(0.1 + 0.2 * (i % 5)) * W, (0.1 + 0.4 * ((i // 5) % 3)) * H], dim=1).expand(B, n, 2)
        u, v = (dots[..., 0] + dots[..., 0]) / W - 1.0, (dots[..., 1] + dots[..., 1]) / H - 1.0
        phi = torch.stack([torch.ones_like(u), u, v, u * u, u * v, v * v], dim=-1).double()
        shift_mm = (phi @ star.T).float() + 8.0 * torch.randn((B, n, 2), generator=gen, device='cuda')
        ang, far = 6.2832 * torch.rand((B, n), generator=gen, device='cuda'), 80.0 + 120.0 * torch.rand((B, n), generator=gen, device='cuda')
        far = torch.where(i % 10 == 9, far, torch.zeros_like(far))
        shift_mm = shift_mm + torch.stack([far * torch.cos(ang), far * torch.sin(ang)], dim=-1)
        pog = (dots - shift_mm * geo['pixels_per_millimeter']).contiguous()
        stream = eve_amd.EVEStream(model, B, use_graph=False, screen_calibration_capacity=n)
        samples, count, dropped = stream._screen_samples()
        k.screen_calib_append(pog, (0.5 * (geo['left_o'] + geo['right_o'])).contiguous(), geo['inv_camera_transformation'],
                              geo['pixels_per_millimeter'], dots.contiguous(), (W, H), samples, count, dropped)
        fit = lambda: stream.fit_screen_calibration(model=args.model, huber_mm=args.huber, max_shift_mm=400.0)
        out = fit()
        torch.cuda.synchronize()
        runs = sorted(round(1e3 * device_ms(fit, args.steps), 2) for _ in range(max(1, args.repeat)))
        print(json.dumps({'mode': 'screen-fit', 'model': args.model, 'streams': B, 'samples': n, 'huber_mm': args.huber, 'us': runs[len(runs) // 2],
                          'us_runs': runs, 'count_min': int(count.min()), 'ok': int(out['ok'].sum()), 'solves_max': int(out['solves'].max()),
                          'rms_mm_max': float(out['rms_mm'].max()), 'rms_mm_raw_max': float(out['rms_mm_raw'].max())}),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', required=True, choices=('plain', 'applied', 'collecting', 'collecting-applied', 'fit', 'screen-applied',
                                                       'screen-collecting', 'screen-fit'))
    ap.add_argument('--model', default='affine', choices=('offset', 'affine', 'quadratic'))
    ap.add_argument('--shape', default='32x2')
    ap.add_argument('--dtype', default='bf16', choices=sorted(DTYPES))
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--streams', type=int, default=32)
    ap.add_argument('--samples', type=int, nargs='+', default=[64, 1024], help='per eye; multiples of 8')
    ap.add_argument('--huber', type=float, default=None)
    args = ap.parse_args()
    with torch.no_grad():
        bench_fit(args) if args.mode == 'fit' else bench_screen_fit(args) if args.mode == 'screen-fit' else bench_step(args)


if __name__ == '__main__':
    main()
