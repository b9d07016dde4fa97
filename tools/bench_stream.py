#!/usr/bin/env python
"""Device time per EVEStream.step under hipGraph replay (eve_amd/stream.py), the shipped refine_net.json pipeline (GRU EyeNet,
CLSTM RefineNet), synthetic weights and clips.  One JSON line per shape:

    python tools/bench_stream.py --shapes 1x1 32x1 32x30 [--dtype bf16] [--steps 50] [--fused-tail] [--ragged | --masked] [--repeat N]
                                 [--screen 1920x1080 [--screen-format nv12] [--render]] [--events] [--face] [--gate]

B x Tc = streams x frames per step.  For Tc > 1 the same clips also go through one EVE.eval() pass (`eval_ms`): what the
stream costs over the plain clip pass.  --fused-tail runs the EyeNet tail as one eve_eye_tail_stream_fwd launch
(EyeNet.stream_fused_tail) instead of layer by layer: the A/B of the fused kernel, e.g. under `rocprofv3 --kernel-trace --stats`.
--ragged steps with seeded random lengths in 0..Tc, a new pattern every step (step(chunk, lengths=...): one graph serves them
all).  --masked steps with a seeded random eye mask with about 20 % holes, a new pattern every step, handed over as a host array
(step(chunk, eye_mask=...): the plan launch, the row gathers and the pinned upload of the mask are in the step); the line then
also holds `launch_floor_us`, the device time per launch of a captured chain of 64 smallest launches (eve_stream_state_rows on 16
floats) in the same process: what one more launch in the graph costs at the least.
--screen WxH feeds uint8 screen captures of that size, [B, Tc, H, W, 3], instead of the pre-resized float screens: the step
then holds the area resize (eve_screen_u8_area_to_nchw) and the copy of the captures into the graph's input buffer; with
--screen-format nv12 | i420 | yuyv the captures go in as a decoder delivers them, under screen_frame_<format> (eve_screen_area_fmt_to_nchw;
`screen_bytes` is what one step copies into the graph for the screen).  --render (with --screen) steps with render=OverlaySpec(heat=True):
the default two markers, the heat map and the eyes inset drawn onto the capture by one eve_overlay_render launch inside the graph, NV12
out (`rendered_bytes` per step); the A/B of the overlay is the same command line without it.  --events steps with
events=GazeEventSpec(fps=30): the one-euro filter, the gaze velocity and the fixation / saccade events by one eve_gaze_events launch
at the end of the graph.  The line then also holds `plain_step_ms`, the same step without events in the same process (windows of the
two alternate, `plain_step_ms_runs` with --repeat), `events_delta_us`, their difference, `events_kernel_us`, the device time per launch
of a captured chain of 64 eve_gaze_events launches on the step's own PoG_px_final (the kernel alone), and `launch_floor_us`.  --face feeds the face-landmark form
in place of pre-cut patches: 640 x 480 camera frames, 20 landmarks per frame and one face_rig row per stream (synthetic heads some 600 mm
in front of the camera), eye_net.face_huber_px = 2: the step then holds the pose solve, the normalisation and the eye-patch warps.
--gate (implies --face) steps with gate=EyeGateSpec(...) with every criterion on and eye_contours in the chunk: one eve_eye_gate launch
before the mask plan.  The line then also holds `masked_step_ms`, the same chunk's masked step with a random eye mask uploaded from
the host, in the same process (windows of the two alternate, `masked_step_ms_runs` with --repeat), `gate_delta_us`, their difference,
`gate_kernel_us`, the device time per launch of a captured chain of 64 eve_eye_gate launches on a step's own derived quantities (the
kernel alone), and `launch_floor_us`.  --repeat N measures every shape N times in one process (`step_ms_runs`; `step_ms` is their median): the run-to-run spread."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import eve_amd  # noqa: E402
from eve_amd import synthetic as detweights  # noqa: E402

DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}
INPUT_KEYS = ('left_eye_patch', 'right_eye_patch', 'left_h', 'right_h', 'left_o', 'right_o', 'left_R', 'right_R', 'head_R',
              'camera_transformation', 'inv_camera_transformation', 'pixels_per_millimeter', 'millimeters_per_pixel', 'screen_frame')


def device_ms(fn, steps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / steps


def launch_floor_us(n=64, reps=50):
    """Device time per launch of a replayed hipGraph of n dependent eve_stream_state_rows launches on a [2, 8] tensor."""
    k = eve_amd.kernels.default_kernels()
    a, b = torch.zeros((2, 8), device='cuda'), torch.zeros((2, 8), device='cuda')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        k.stream_state_rows(a, b)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(n):
            k.stream_state_rows(a, b)
    graph.replay()
    torch.cuda.synchronize()
    return round(1e3 * device_ms(graph.replay, reps) / n, 3)


def events_kernel_us(clip, out, spec, n=64, reps=50):
    """Device time per launch of a replayed hipGraph of n dependent eve_gaze_events launches on one step's results: every launch
    carries the state on (the counted time keeps running, the store fills and then drops)."""
    k = eve_amd.kernels.default_kernels()
    B, Tc = out['PoG_px_final'].shape[:2]
    pog = out['PoG_px_final'].float().contiguous().clone()
    o = torch.stack([clip['left_o'], clip['right_o']], dim=-1).mean(dim=-1).float().contiguous()
    cam, ppm = clip['inv_camera_transformation'].float().contiguous(), clip['pixels_per_millimeter'].float().contiguous()
    state = torch.zeros((B, 32), dtype=torch.float64, device='cuda')
    store = torch.zeros((B, 256, 8), dtype=torch.float64, device='cuda')
    count, dropped = torch.zeros((B,), dtype=torch.int32, device='cuda'), torch.zeros((B,), dtype=torch.int32, device='cuda')
    run = lambda: k.gaze_events(pog, o, cam, ppm, spec, state, store, count, dropped)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(n):
            run()
    graph.replay()
    torch.cuda.synchronize()
    return round(1e3 * device_ms(graph.replay, reps) / n, 3)


FACE_CAMERA = (480, 640)                     # (IH, IW) of --face's camera frames
FACE_K = (600.0, 600.0, 320.0, 240.0)


def face_form(B, Tc, seed):
    """--face's keys: camera_frame uint8 [B, Tc, 480, 640, 3], face_landmarks float32 [B, Tc, 20, 2], face_rig [B, 12 + 60] and
    eye_contours float32 [B, Tc, 2, 6, 2] (an open eye, every 17th frame closed), on the GPU.  Heads of 20 points within 70 mm, turned
    by up to 0.2 rad and drifting by 0.01 rad and 2 mm per frame, 550 .. 650 mm in front of the camera; 0.2 px of landmark noise."""
    from eve_amd import data
    g = np.random.default_rng(seed)
    L = 20
    fx, fy, cx, cy = FACE_K
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    lm, rigs = np.zeros((B, Tc, L, 2), dtype=np.float32), []
    for b in range(B):
        model = g.uniform(-70, 70, (L, 3)) * np.array([1.0, 1.0, 0.4])
        eyes = np.array([[32.0, -30.0, -20.0], [-32.0, -30.0, -20.0]])
        rigs.append(data.face_rig(K, model, eyes, 1300.0, 600.0))
        rv, t = g.uniform(-0.2, 0.2, 3), np.array([g.uniform(-40, 40), g.uniform(-30, 30), g.uniform(550, 650)])
        for f in range(Tc):
            rv, t = rv + g.uniform(-0.01, 0.01, 3), t + g.uniform(-2, 2, 3)
            th = np.linalg.norm(rv)
            kx = np.array([[0, -rv[2], rv[1]], [rv[2], 0, -rv[0]], [-rv[1], rv[0], 0]]) / max(th, 1e-12)
            R = np.eye(3) + np.sin(th) * kx + (1 - np.cos(th)) * kx @ kx
            p = model @ R.T + t
            lm[b, f] = np.stack([fx * p[:, 0] / p[:, 2] + cx, fy * p[:, 1] / p[:, 2] + cy], axis=1) + g.normal(0, 0.2, (L, 2))
    contours = np.zeros((B, Tc, 2, 6, 2), dtype=np.float32)
    for b in range(B):
        for f in range(Tc):
            half = 0.5 * (0.05 if (b + f) % 17 == 16 else 0.30 + g.uniform(-0.01, 0.01)) * 30.0
            for e in range(2):
                x0, y0 = 300.0 + 60.0 * e, 200.0
                contours[b, f, e] = [(x0 - 15, y0), (x0 - 5, y0 - half), (x0 + 5, y0 - half), (x0 + 15, y0), (x0 + 5, y0 + half), (x0 - 5, y0 + half)]
    frames = torch.randint(0, 256, (B, Tc) + FACE_CAMERA + (3,), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    return {'camera_frame': frames.cuda(), 'face_landmarks': torch.from_numpy(lm).cuda(),
            'face_rig': torch.from_numpy(np.stack(rigs).astype(np.float32)).cuda(), 'eye_contours': torch.from_numpy(contours).cuda()}


def gate_kernel_us(model, clip, spec, n=64, reps=50):
    """Device time per launch of a replayed hipGraph of n dependent eve_eye_gate launches on what one step derives from the clip:
    every launch carries the state on (the ticks keep running, the store fills and then drops)."""
    from eve_amd.eye_net import eye_pose_batch
    k = eve_amd.kernels.default_kernels()
    B, Tc = clip['camera_frame'].shape[:2]
    d = eye_pose_batch(clip, model.config, torch.zeros((B, 13), dtype=torch.float64, device='cuda'), huber_px=model.eye_net.face_huber_px)
    both = lambda key, m: torch.stack([d['left' + key], d['right' + key]]).reshape(2, B * Tc, m).float().contiguous()
    pose_valid, rms, inliers = d['pose_valid'].to(torch.uint8).contiguous(), d['face_reproj_rms'].contiguous(), d['face_inliers'].contiguous()
    warp, h, contours = both('_eye_warp', 9), both('_h', 2), clip['eye_contours'].contiguous()
    ph, pw = eve_amd.data.eye_patch_hw(model.config)
    state = torch.zeros((B, 2, 8), dtype=torch.float64, device='cuda')
    store = torch.zeros((B, 256, 4), dtype=torch.float64, device='cuda')
    count, dropped = torch.zeros((B,), dtype=torch.int32, device='cuda'), torch.zeros((B,), dtype=torch.int32, device='cuda')
    run = lambda: k.eye_gate(spec, B, Tc, state, store, count, dropped, pose_valid=pose_valid, reproj_rms=rms, inliers=inliers, warp=warp, h=h,
                             contours=contours, frame_size=(FACE_CAMERA[1], FACE_CAMERA[0]), patch_size=(pw, ph))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(n):
            run()
    graph.replay()
    torch.cuda.synchronize()
    return round(1e3 * device_ms(graph.replay, reps) / n, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', nargs='+', default=['1x1', '32x1', '32x30'])
    ap.add_argument('--dtype', default='bf16', choices=sorted(DTYPES))
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--fused-tail', action='store_true')
    ap.add_argument('--ragged', action='store_true')
    ap.add_argument('--masked', action='store_true', help='step with a random eye mask, about 20 %% of the eyes masked out')
    ap.add_argument('--repeat', type=int, default=1)
    ap.add_argument('--screen', default=None, metavar='WxH', help='feed uint8 screen captures of this size, e.g. 1920x1080')
    ap.add_argument('--screen-format', default='rgb', choices=('rgb', 'nv12', 'i420', 'yuyv'), help='the layout of the --screen captures')
    ap.add_argument('--render', action='store_true', help='step with render=OverlaySpec(heat=True): the overlay launch inside the graph')
    ap.add_argument('--events', action='store_true', help='step with events=GazeEventSpec(fps=30): the gaze filter and the fixation / saccade events')
    ap.add_argument('--face', action='store_true', help='feed the face-landmark form (camera frames, landmarks, face_rig) in place of pre-cut patches')
    ap.add_argument('--gate', action='store_true', help='step with gate=EyeGateSpec(...), every criterion on (implies --face)')
    ap.add_argument('--luminance', action='store_true', help='step with luminance=ScreenLuminanceSpec(radii_px=(60, 200)) feeding pupil=, against '
                    'the same step with pupil= and an uploaded pupil_luminance (needs --screen)')
    args = ap.parse_args()
    args.face = args.face or args.gate
    if args.luminance and (not args.screen or args.ragged or args.masked or args.events or args.gate or args.render):
        ap.error('--luminance measures the uniform step on a capture: give it with --screen WxH alone')
    if args.gate and (args.ragged or args.masked or args.events):
        ap.error('--gate measures the gated step against the masked one itself: give it alone')
    if args.screen_format != 'rgb' and not args.screen:
        ap.error('--screen-format needs --screen WxH')
    if args.render and not args.screen:
        ap.error('--render draws onto a capture: it needs --screen WxH')
    if args.ragged and args.masked:
        ap.error('--ragged and --masked are two measurements: give one')
    cfg = eve_amd.reset_standalone_config()
    cfg.import_json(os.path.join(REPO, 'configs', 'refine_net.json'))
    cfg.import_dict({'eye_net_load_pretrained': False})
    model = eve_amd.EVE(output_predictions=True)
    model.eye_net.compute_dtype = model.refine_net.compute_dtype = DTYPES[args.dtype]
    detweights.fill_module(model.eye_net, 0)
    detweights.fill_module(model.refine_net, 1)
    model = model.cuda().eval()
    model.eye_net.stream_fused_tail = args.fused_tail
    screen = None
    if args.screen:
        if not cfg.load_screen_content:
            ap.error('--screen needs a configuration with load_screen_content')
        screen = tuple(int(v) for v in args.screen.lower().split('x'))
    for shape in args.shapes:
        B, Tc = (int(v) for v in shape.split('x'))
        small = detweights.eve_batch(min(B, 4), Tc, seed=1)
        full = {k: torch.cat([v] * ((B + 3) // 4), dim=0)[:B].contiguous().cuda() for k, v in small.items()}
        if screen is not None:
            g = torch.Generator().manual_seed(B * 1000 + Tc)
            W, H = screen
            shape = {'rgb': (H, W, 3), 'nv12': (H * 3 // 2, W), 'i420': (H * 3 // 2, W), 'yuyv': (H, W, 2)}[args.screen_format]
            del full['screen_frame']
            screen_key = 'screen_frame' if args.screen_format == 'rgb' else 'screen_frame_' + args.screen_format
            full[screen_key] = torch.randint(0, 256, (B, Tc) + shape, generator=g, dtype=torch.uint8).cuda()
        clip = {k: full[k] for k in INPUT_KEYS + ('screen_frame_nv12', 'screen_frame_i420', 'screen_frame_yuyv') if k in full}
        if args.face:
            model.eye_net.face_huber_px = 2.0
            clip = {k: v for k, v in clip.items() if k not in ('left_eye_patch', 'right_eye_patch', 'left_h', 'right_h', 'left_o', 'right_o',
                                                               'left_R', 'right_R', 'head_R')}
            clip.update(face_form(B, Tc, seed=B * 1000 + Tc))
            gated_clip = clip
            clip = {k: v for k, v in clip.items() if k != 'eye_contours'}
        stream = eve_amd.EVEStream(model, B)
        rng = np.random.default_rng(B * 1000 + Tc)
        extra = {'render': eve_amd.OverlaySpec(heat=True)} if args.render else {}
        plain_extra = dict(extra)
        if args.events:
            extra['events'] = eve_amd.GazeEventSpec(fps=30)
        step = (lambda: stream.step(clip, lengths=rng.integers(0, Tc + 1, size=B), **extra)) if args.ragged else (lambda: stream.step(clip, **extra))
        if args.masked:
            step = lambda: stream.step(clip, eye_mask=rng.random((B, Tc, 2)) >= 0.2, **extra)
        if args.gate:
            gate_spec = eve_amd.EyeGateSpec(max_reproj_px=1.0, min_inliers=15, min_coverage=0.9, head_pitch=(-0.4, 0.4), head_yaw_left=(-0.5, 0.3),
                                            head_yaw_right=(-0.3, 0.5), blink=eve_amd.BlinkSpec())
            step = lambda: stream.step(gated_clip, gate=gate_spec, **extra)
        for _ in range(3):
            step()                                           # capture + warm replays
        torch.cuda.synchronize()
        plain_runs = []
        if args.events:                                      # the same step without events, in windows that alternate with the timed ones
            assert not args.ragged and not args.masked, '--events measures the uniform step'
            plain_step = lambda: stream.step(clip, **plain_extra)
            for _ in range(3):
                plain_step()
            torch.cuda.synchronize()
            runs = []
            for _ in range(max(1, args.repeat)):
                plain_runs.append(round(device_ms(plain_step, args.steps), 4))
                runs.append(round(device_ms(step, args.steps), 4))
            runs, plain_runs = sorted(runs), sorted(plain_runs)
        elif args.luminance:                                 # pupil= with an uploaded covariate (what a caller had before), alternating
            pupil = eve_amd.PupilSpec(fps=30)
            lum_spec = eve_amd.ScreenLuminanceSpec(radii_px=(60, 200), to_pupil=(0.5, 0.0, 0.5))
            uploaded = dict(clip, pupil_luminance=torch.rand((B, Tc), device='cuda'))
            step = lambda: stream.step(clip, luminance=lum_spec, pupil=pupil)
            plain_step = lambda: stream.step(uploaded, pupil=pupil)
            for _ in range(3):
                step()
                plain_step()
            torch.cuda.synchronize()
            runs = []
            for _ in range(max(1, args.repeat)):
                plain_runs.append(round(device_ms(plain_step, args.steps), 4))
                runs.append(round(device_ms(step, args.steps), 4))
            runs, plain_runs = sorted(runs), sorted(plain_runs)
        elif args.gate:                                      # the same chunk's masked step, in windows that alternate with the timed ones
            masked_step = lambda: stream.step(clip, eye_mask=rng.random((B, Tc, 2)) >= 0.2, **extra)
            for _ in range(3):
                masked_step()
            torch.cuda.synchronize()
            runs = []
            for _ in range(max(1, args.repeat)):
                plain_runs.append(round(device_ms(masked_step, args.steps), 4))
                runs.append(round(device_ms(step, args.steps), 4))
            runs, plain_runs = sorted(runs), sorted(plain_runs)
        else:
            runs = sorted(round(device_ms(step, args.steps), 4) for _ in range(max(1, args.repeat)))
        res = {'B': B, 'Tc': Tc, 'dtype': args.dtype, 'tail': 'fused' if args.fused_tail else 'layers', 'ragged': args.ragged, 'masked': args.masked,
               'screen': args.screen or 'float', 'step_ms': runs[len(runs) // 2]}
        if screen is not None:
            res['screen_format'], res['screen_bytes'] = args.screen_format, full[screen_key].numel()
        if args.render:
            res['render'], res['rendered_bytes'] = 'nv12', step()['rendered'].numel()
        if len(runs) > 1:
            res['step_ms_runs'] = runs
        if args.masked:
            res['launch_floor_us'] = launch_floor_us()
        if args.events:
            res['events'], res['plain_step_ms'] = True, plain_runs[len(plain_runs) // 2]
            res['events_delta_us'] = round(1e3 * (res['step_ms'] - res['plain_step_ms']), 2)
            if len(plain_runs) > 1:
                res['plain_step_ms_runs'] = plain_runs
            res['events_kernel_us'] = events_kernel_us(clip, {k_: v.clone() for k_, v in step().items()}, extra['events'])
            res['launch_floor_us'] = launch_floor_us()
        if args.luminance:
            res['luminance'], res['uploaded_step_ms'] = True, plain_runs[len(plain_runs) // 2]
            res['luminance_delta_us'] = round(1e3 * (res['step_ms'] - res['uploaded_step_ms']), 2)
            res['uploaded_step_ms_runs'] = plain_runs
        if args.face:
            res['face'] = True
        if args.gate:
            res['gate'], res['masked_step_ms'] = True, plain_runs[len(plain_runs) // 2]
            res['gate_delta_us'] = round(1e3 * (res['step_ms'] - res['masked_step_ms']), 2)
            if len(plain_runs) > 1:
                res['masked_step_ms_runs'] = plain_runs
            res['usable_share'] = round(float(step()['eye_valid'].float().mean()), 3)
            res['gate_kernel_us'] = gate_kernel_us(model, gated_clip, gate_spec)
            res['launch_floor_us'] = launch_floor_us()
        res['us_per_frame'] = round(1e3 * res['step_ms'] / (B * Tc), 3)
        if Tc > 1 and not args.face:                         # (EVE.forward takes no face-landmark form)
            with torch.no_grad():
                for _ in range(2):
                    model(dict(full))
                res['eval_ms'] = round(device_ms(lambda: model(dict(full)), max(5, args.steps // 5)), 4)
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
