#!/usr/bin/env python
"""Device time of the eye-patch warp (eve_eye_warp_u8_to_nchw / _to_stem, csrc/eye_warp.hip) next to the launch it stands in for,
and of one EVEStream step fed whole camera frames next to the same step fed pre-cut uint8 patches.

    python tools/bench_eye_warp.py [--patches 64] [--size 1920x1080] [--iters 500] [--rounds 5] [--shapes 1x1 8x4 32x2]
                                   [--steps 50] [--dtype bf16] [--lens] [--pose] [--format nv12] [--landmarks] [--surface]
                                   [--markdown profiles/table.md]

Part 1, per launch, the four routes interleaved in one process (the median over the rounds of events around `iters` calls):
    warp_nchw / warp_stem   N patches of 128 x 128 cut from N frames of the given size, each by its own rotated, scaled warp with a
                            perspective row; float NCHW and the stem's packed bf16
    crop_nchw / crop_stem   eve_frames_u8_to_nchw / _to_stem on N pre-cut 128 x 128 x 3 patches: what the caller launched before,
                            after two cv2.warpPerspective calls per frame on the host and a second upload (neither is timed here)
    lens_nchw / lens_stem   with --lens: the same patches through eve_eye_warp_lens_u8_to_nchw / _to_stem, every frame behind the
                            rational eight-coefficient lens of lens_rows() (the arithmetic does not depend on the values)
    pose_normalize          with --pose: eve_eye_pose_normalize on N pose rows (both eyes of N frames: 2 N threads) into preallocated
                            outputs -- the launch that derives the warps, R, o, h and head_R from the face tracker's solvePnP result
    fmt_nchw / fmt_stem     with --format {bgr,nv12,i420,yuyv}: the same patches from frames in that layout through
                            eve_eye_warp_fmt_to_nchw / _to_stem (bt601), which convert only the taps they read
    conv_nchw / conv_stem   with --format: what a caller did before -- convert the WHOLE frames to RGB on the device with torch
                            (to_rgb_device: the same integer matrix, several elementwise passes), then the RGB launch; conv_only
                            is the conversion alone.  These three run iters / 20 times per round.
The rate quoted for a warp is (bytes its loads ask for: 4 taps x 3 channels per output pixel) + (bytes stored) over the time; the
taps overlap, so the distinct bytes behind them are about a quarter -- it is a rate of the kernel's traffic, not of HBM.

Part 2, per EVEStream step under graph replay (refine_net config): `camera` feeds camera_frame + two warps per frame, `patches`
the uint8 [B, Tc, 128, 128, 3] patch pair.  The camera step also copies B * Tc whole frames into the graph's input buffer.  With
--lens a third stream, `lens`, feeds the camera keys plus camera_lens.  With --pose another stream, `pose`, feeds camera_frame + eye_pose
and none of the keys the rows derive (warps, <side>_h, <side>_o, <side>_R, head_R): one more launch inside the graph.  With --format
a stream `fmt` feeds camera_frame_<format> in place of camera_frame: fewer bytes copied into the graph, the taps converted inside.

--landmarks (implies --pose): the face-landmark form.  Before part 1, eve_face_pose_solve alone on 32 x 2 and 32 x 30 frames at L = 6
and L = 68 into preallocated outputs: `cold` without a state (every sequence's first frame starts from the closed-form guess, the
later ones from the frame before), `warm` with a carried state that holds the pose of the chunk's last frame (every frame warm), and
`all_cold` on T = 1 chunks of the same sequences for the price of a cold frame alone; beside them the accepted-step counts of
the first 8 sequences, taken from the contract in numpy (tests/face_pose_ref.py: the same arithmetic, so the same counts), and the
fraction of frames that got a solution (a frame that reaches the contract's cap of 32 accepted steps has none).  In
part 2 a stream `face` feeds camera_frame + face_landmarks [B, Tc, 68, 3] + face_rig and none of the derived keys, next to `pose`.
The eye_pose step of ANOTHER checkout (the parent commit's) is measured by running that checkout's own `--pose --shapes 32x2` in
alternating rounds with this one, process by process; this file only measures the tree it lies in.

--landmarks --raw [--huber K]: eve_face_pose_solve_ex at 32 x 2 x 68 next to the plain launch in the same process, route by route
in alternating rounds (raw_solve_launches), and in part 2 a stream `raw` that feeds camera_frame + face_landmarks_raw + face_rig +
camera_lens (with face_huber_px = K) next to `face`; with --lens also `face_lens`, the face stream with the same camera_lens rows.

--surface: nothing of the above; instead the surface launches (eve_eye_warp_surface_to_nchw / _to_stem) on N frames of the given
size as a decoder leaves them -- NV12 in rows of 2048 bytes and 1088 coded rows, then P010 in rows of 4096 -- three routes
interleaved in one process:
    linear_*    the byte-linear launch (eve_eye_warp_fmt_to_*) on the linearised NV12 frames: what the surface launch stands beside
    surface_*   the surface launch on the padded buffer
    copy_*      what a caller did before: a torch de-pitch copy (P010: the high bytes) into a byte-linear NV12 frame, then linear_*;
                copy_only is that pass alone
and, per --shapes, an EVEStream step fed camera_surface + screen_surface (both NV12 in 2048 x 1088) next to the same step fed
camera_frame_nv12 + screen_frame_nv12 on the linearised frames."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import eve_amd  # noqa: E402
from eve_amd import synthetic as detweights  # noqa: E402
from eve_amd.kernels import default_kernels  # noqa: E402

HW = (128, 128)
DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}
STREAM_KEYS = ('left_h', 'right_h', 'left_o', 'right_o', 'left_R', 'right_R', 'head_R', 'camera_transformation',
               'inv_camera_transformation', 'pixels_per_millimeter', 'millimeters_per_pixel', 'screen_frame')


def device_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def warps_for(n, IH, IW, seed):
    """n homographies (patch pixel -> camera pixel) that keep a 128 x 128 patch inside an IH x IW frame."""
    g = np.random.default_rng(seed)
    ms = []
    for _ in range(n):
        s, a = g.uniform(1.0, 1.5), math.radians(g.uniform(-15, 15))
        c, d = s * math.cos(a), s * math.sin(a)
        ms.append([[c, -d, g.uniform(80, IW - 320)], [d, c, g.uniform(80, IH - 320)], [g.uniform(-1e-4, 1e-4), g.uniform(-1e-4, 1e-4), 1.0]])
    return torch.tensor(np.array(ms), dtype=torch.float32)


def lens_rows(n, IH, IW):
    """n rows (fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6) of one camera: a 1080p webcam's focal length scaled to the frame, the
    principal point a little off its centre, a mild rational model."""
    f = 1400.0 * IW / 1920.0
    row = [f, f * 1.01, IW / 2 + 3.5, IH / 2 - 2.25, 0.9, 0.1, 2e-3, 1e-3, 0.01, 1.1, 0.15, 0.02]
    return torch.tensor([row] * n, dtype=torch.float32)


def pose_rows(n, IH, IW, seed):
    """n pose rows of a 1080p-like webcam scaled to the frame: the head 500..700 mm in front of it, the patch one camera pixel per
    patch pixel at the normalised distance, so every 128 x 128 patch stays inside the frame."""
    g = np.random.default_rng(seed)
    f = 1400.0 * IW / 1920.0
    rows = [[f, f, IW / 2, IH / 2] + list(g.uniform(-0.3, 0.3, 3)) + [g.uniform(-60, 60), g.uniform(-40, 40), g.uniform(500, 700)] +
            [-32.0, -35.0, 25.0, 32.0, -35.0, 25.0, f, 600.0] for _ in range(n)]
    return torch.tensor(np.array(rows), dtype=torch.float32)


def face_sequences(B, Tc, L, IH, IW, seed):
    """Landmarks and rigs of B frontal heads 500..700 mm in front of pose_rows' camera, moving by up to 2 degrees and 4 mm a frame,
    with the noise of tests/face_pose_ref.py's cases (1 px at f = 1000) -> numpy (landmarks [B, Tc, L, 3], rig [B, 12 + 3L])."""
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    import face_pose_ref as fr
    f = 1400.0 * IW / 1920.0
    return fr.sequences(B, Tc, L, seed, weights=True, K=(f, f, IW / 2, IH / 2), frontal=True, focal_norm=f, step_deg=2.0, step_mm=4.0,
                        noise=f / 1000.0)


def solve_launches(args, IH, IW):
    """eve_face_pose_solve alone (see the module docstring) -> rows of dicts."""
    import ctypes
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    import face_pose_ref as fr
    k = default_kernels()
    rows = []
    for S_, T_ in ((32, 2), (32, 30)):
        for L in (6, 68):
            lm_np, rig_np = face_sequences(S_, T_, L, IH, IW, seed=L)
            ref = fr.solve(lm_np[:8], rig_np[:8])
            lm, rig = torch.from_numpy(lm_np).cuda(), torch.from_numpy(rig_np).cuda()
            lm1 = lm[:, :1].contiguous()
            outs = [torch.empty((S_, T_, n), device='cuda') for n in (9, 3, 1)] + [torch.empty((S_, T_), dtype=torch.uint8, device='cuda')]
            state = torch.zeros((S_, 13), dtype=torch.float64, device='cuda')
            ptrs = [ctypes.c_void_p(t.data_ptr()) for t in outs]
            stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

            def launch(T=T_, lm_=lm, st=None):
                status = k.lib.eve_face_pose_solve(S_, T, L, 3, ctypes.c_void_p(lm_.data_ptr()), ctypes.c_void_p(rig.data_ptr()), None,
                                                   None if st is None else ctypes.c_void_p(st.data_ptr()), None, *ptrs, stream())
                assert status == 0, k.lib.eve_last_error()
            routes = {'cold': lambda: launch(), 'warm': lambda: launch(st=state), 'all_cold': lambda: launch(T=1, lm_=lm1)}
            for fn in routes.values():
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            launch()
            torch.cuda.synchronize()
            solved = float(outs[3].float().mean())       # a frame that reaches the cap of 32 accepted steps has no solution
            times = {name: [] for name in routes}
            for _ in range(args.rounds):
                for name, fn in routes.items():
                    times[name].append(device_ms(fn, args.iters))
            res = {'S': S_, 'T': T_, 'L': L, 'iters': args.iters, 'rounds': args.rounds, 'kernel': k.lib.eve_last_kernel().decode(),
                   'frames_solved': round(solved, 4), 'frames_solved_contract_first_8': round(float(ref['valid'].mean()), 4),
                   'accepted_cold_first_frame': [int(ref['accepted'][:, 0].min()), int(ref['accepted'][:, 0].max())],
                   'accepted_warm_frames': [int(ref['accepted'][:, 1:].min()), int(ref['accepted'][:, 1:].max())]}
            for name, t in times.items():
                res[name + '_us'] = round(1e3 * median(t), 2)
                res[name + '_us_min_max'] = [round(1e3 * min(t), 2), round(1e3 * max(t), 2)]
            res['warm_us_per_frame'] = round(res['warm_us'] / T_, 2)
            rows.append(res)
            print(json.dumps(res), flush=True)
    return rows


def raw_face_sequences(B, Tc, L, IH, IW, seed):
    """face_sequences seen through a raw camera: lens_rows' mild rational model with the rig's own intrinsics -> numpy (raw landmarks
    [B, Tc, L, 3], rig, lens [B, Tc, 12], the undistorted landmarks)."""
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    import face_pose_raw_ref as rr
    lm, rig = face_sequences(B, Tc, L, IH, IW, seed)
    f = 1400.0 * IW / 1920.0
    row = np.array([f, f, IW / 2, IH / 2, 0.9, 0.1, 2e-3, 1e-3, 0.01, 1.1, 0.15, 0.02], dtype=np.float32)
    return rr.distort_landmarks(lm, row), rig, np.broadcast_to(row, (B, Tc, 12)).copy(), lm


def raw_solve_launches(args, IH, IW):
    """--landmarks --raw: eve_face_pose_solve_ex at 32 x 2 x 68 into preallocated outputs, next to the plain launch on the same
    heads' undistorted landmarks in the same process, the routes interleaved round by round: `plain` (eve_face_pose_solve), `ex_off`
    (the new entry, no lens, no loss), `ex_lens` (raw landmarks + lens rows), and with --huber K `ex_huber` and `ex_lens_huber`;
    every one cold (no carried state) and warm (a carried state that holds the chunk's last pose) -> one dict."""
    import ctypes
    k = default_kernels()
    S_, T_, L = 32, 2, 68
    raw_np, rig_np, lens_np, lm_np = raw_face_sequences(S_, T_, L, IH, IW, seed=L)
    raw, rig, lens, lm = (torch.from_numpy(a).cuda() for a in (raw_np, rig_np, lens_np, lm_np))
    outs = [torch.empty((S_, T_, n), device='cuda') for n in (9, 3, 1)] + [torch.empty((S_, T_), dtype=torch.uint8, device='cuda') for _ in range(2)]
    ptrs = [ctypes.c_void_p(t.data_ptr()) for t in outs]
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    states = {}

    def plain(st=None):
        assert k.lib.eve_face_pose_solve(S_, T_, L, 3, p(lm), p(rig), None, p(st), None, *ptrs[:4], stream()) == 0, k.lib.eve_last_error()

    def ex(pts, rows, huber, st=None):
        assert k.lib.eve_face_pose_solve_ex(S_, T_, L, 3, p(pts), p(rig), p(rows), huber, None, p(st), None, *ptrs, stream()) == 0, k.lib.eve_last_error()
    routes = {'plain': plain, 'ex_off': lambda st=None: ex(lm, None, 0.0, st), 'ex_lens': lambda st=None: ex(raw, lens, 0.0, st)}
    if args.huber:
        routes['ex_huber'] = lambda st=None: ex(lm, None, args.huber, st)
        routes['ex_lens_huber'] = lambda st=None: ex(raw, lens, args.huber, st)
    res = {'S': S_, 'T': T_, 'L': L, 'iters': args.iters, 'rounds': args.rounds, 'huber_px': args.huber}
    for name, fn in routes.items():
        states[name] = torch.zeros((S_, 13), dtype=torch.float64, device='cuda')
        for _ in range(5):
            fn()
            fn(states[name])
        torch.cuda.synchronize()
        res[name + '_frames_solved'] = round(float(outs[3].float().mean()), 4)
        if name != 'plain':
            res[name + '_inliers_min_max'] = [int(outs[4].min()), int(outs[4].max())]
    times = {(name, mode): [] for name in routes for mode in ('cold', 'warm')}
    for _ in range(args.rounds):
        for name, fn in routes.items():
            times[name, 'cold'].append(device_ms(fn, args.iters))
            times[name, 'warm'].append(device_ms(lambda: fn(states[name]), args.iters))
    for (name, mode), t in times.items():
        res['%s_%s_us' % (name, mode)] = round(1e3 * median(t), 2)
        res['%s_%s_us_min_max' % (name, mode)] = [round(1e3 * min(t), 2), round(1e3 * max(t), 2)]
    print(json.dumps(res), flush=True)
    return res


def format_frames(fmt, lead, IH, IW, gen=None, device='cuda'):
    """Random bytes in the layout of fmt with leading dimensions `lead`."""
    shape = {'bgr': (IH, IW, 3), 'nv12': (IH * 3 // 2, IW), 'i420': (IH * 3 // 2, IW), 'yuyv': (IH, IW, 2)}[fmt]
    if gen is None:
        return torch.randint(0, 256, tuple(lead) + shape, dtype=torch.uint8, device=device)
    return torch.randint(0, 256, tuple(lead) + shape, generator=gen, dtype=torch.uint8).to(device)


def to_rgb_device(buf, fmt, IH, IW):
    """Whole frames [N, ...] of fmt -> RGB uint8 [N, IH, IW, 3] with torch on the device: the bt601 integer matrix of
    include/eve_hip.h, chroma replicated -- the pass a caller ran before the RGB launch."""
    if fmt == 'bgr':
        return buf.flip(-1).contiguous()
    N = buf.shape[0]
    if fmt == 'yuyv':
        Y, U, V = buf[..., 0], buf[:, :, 0::2, 1].repeat_interleave(2, dim=2), buf[:, :, 1::2, 1].repeat_interleave(2, dim=2)
    else:
        flat = buf.reshape(N, -1)
        Y = flat[:, :IH * IW].view(N, IH, IW)
        if fmt == 'nv12':
            uv = flat[:, IH * IW:].view(N, IH // 2, IW // 2, 2)
            U, V = uv[..., 0], uv[..., 1]
        else:
            q = (IH // 2) * (IW // 2)
            U, V = flat[:, IH * IW:IH * IW + q].view(N, IH // 2, IW // 2), flat[:, IH * IW + q:].view(N, IH // 2, IW // 2)
        U, V = (c.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2) for c in (U, V))
    yy = (Y.int() - 16).clamp_(min=0) * 1220542 + (1 << 19)
    u, v = U.int() - 128, V.int() - 128
    rgb = [(yy + 1673527 * v) >> 20, (yy - 852492 * v - 409993 * u) >> 20, (yy + 2116026 * u) >> 20]
    return torch.stack([c.clamp_(0, 255) for c in rgb], dim=-1).to(torch.uint8)


def median(v):
    return sorted(v)[len(v) // 2]


def surface_pair(fmt, lead, IH, IW, pitch_px=2048, coded=1088, gen=None):
    """A decoder's surface and its content -> (SurfaceLayout, buf uint8 lead + [coded * 3 / 2, pitch] of random bytes, padding
    included, and the byte-linear NV12 frames lead + [IH * 3 / 2, IW] it holds).  fmt: 'nv12' or 'p010' (2 bytes per sample)."""
    from eve_amd.data import SurfaceLayout
    bpp = 2 if fmt == 'p010' else 1
    L = SurfaceLayout(fmt, IW, IH, pitch=pitch_px * bpp, coded_height=coded)
    shape = tuple(lead) + (coded * 3 // 2, pitch_px * bpp)
    buf = torch.randint(0, 256, shape, dtype=torch.uint8, device='cuda') if gen is None else torch.randint(0, 256, shape, generator=gen, dtype=torch.uint8).cuda()
    return L, buf, depitch(buf, fmt, IH, IW, coded)


def depitch(buf, fmt, IH, IW, coded):
    """The pass a caller ran before the byte-linear launch: the visible luma and chroma rows of a padded NV12 / P010 surface
    [..., coded * 3 / 2, pitch] gathered into one byte-linear NV12 frame [..., IH * 3 / 2, IW] (P010: the high byte of each word)."""
    v = buf.view(buf.shape[:-1] + (buf.shape[-1] // 2, 2))[..., 1] if fmt == 'p010' else buf
    return torch.cat([v[..., :IH, :IW], v[..., coded:coded + IH // 2, :IW]], dim=-2).contiguous()


def surface_launches(args, IH, IW):
    k = default_kernels()
    N = args.patches
    torch.manual_seed(N)
    warps = warps_for(N, IH, IW, seed=N).cuda()
    packed = torch.empty((N, HW[0] + 6, HW[1] + 8, 4), dtype=torch.bfloat16, device='cuda')
    rows = []
    for fmt in ('nv12', 'p010'):
        L, buf, lin = surface_pair(fmt, (N,), IH, IW)
        routes = {'linear_nchw': lambda: k.eye_warp_fmt_to_nchw(lin, warps, HW, 'nv12'),
                  'surface_nchw': lambda: k.eye_warp_surface_to_nchw(buf, warps, HW, L),
                  'copy_nchw': lambda: k.eye_warp_fmt_to_nchw(depitch(buf, fmt, IH, IW, L.coded_height), warps, HW, 'nv12'),
                  'linear_stem': lambda: k.eye_warp_fmt_to_stem(lin, warps, HW, 'nv12', out=packed),
                  'surface_stem': lambda: k.eye_warp_surface_to_stem(buf, warps, HW, L, out=packed),
                  'copy_stem': lambda: k.eye_warp_fmt_to_stem(depitch(buf, fmt, IH, IW, L.coded_height), warps, HW, 'nv12', out=packed),
                  'copy_only': lambda: depitch(buf, fmt, IH, IW, L.coded_height)}
        slow = {'copy_nchw', 'copy_stem', 'copy_only'}
        assert torch.equal(routes['surface_nchw'](), routes['linear_nchw']()) and torch.equal(routes['copy_nchw'](), routes['linear_nchw']())
        for fn in routes.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in routes}
        for _ in range(args.rounds):
            for name, fn in routes.items():
                times[name].append(device_ms(fn, max(1, args.iters // 10) if name in slow else args.iters))
        res = {'surface': fmt, 'patches': N, 'frame': '%dx%d' % (IW, IH), 'pitch': L.pitch, 'coded_height': L.coded_height, 'iters': args.iters,
               'rounds': args.rounds, 'frame_bytes': {'surface': L.frame_bytes, 'linear': lin[0].numel()}}
        for name, t in times.items():
            res[name + '_us'] = round(1e3 * median(t), 2)
            res[name + '_us_min_max'] = [round(1e3 * min(t), 2), round(1e3 * max(t), 2)]
        for form in ('nchw', 'stem'):
            res['surface_over_linear_' + form] = round(median(times['surface_' + form]) / median(times['linear_' + form]), 3)
            res['copy_over_surface_' + form] = round(median(times['copy_' + form]) / median(times['surface_' + form]), 2)
        routes['surface_stem']()
        res['kernel'] = k.lib.eve_last_kernel().decode()
        print(json.dumps(res), flush=True)
        rows.append(res)
        del routes, buf, lin
    return rows


def surface_steps(args, IH, IW):
    cfg = eve_amd.reset_standalone_config()
    cfg.import_json(os.path.join(REPO, 'configs', 'refine_net.json'))
    cfg.import_dict({'eye_net_load_pretrained': False})
    model = eve_amd.EVE(output_predictions=True)
    model.eye_net.compute_dtype = model.refine_net.compute_dtype = DTYPES[args.dtype]
    detweights.fill_module(model.eye_net, 0)
    detweights.fill_module(model.refine_net, 1)
    model = model.cuda().eval()
    rows = []
    for shape in args.shapes:
        B, Tc = (int(v) for v in shape.split('x'))
        small = detweights.eve_batch(min(B, 4), Tc, seed=1)
        rest = {k_: torch.cat([small[k_]] * ((B + 3) // 4), dim=0)[:B].contiguous().cuda() for k_ in STREAM_KEYS if k_ in small and k_ != 'screen_frame'}
        rest.update(left_eye_warp=warps_for(B * Tc, IH, IW, seed=B).view(B, Tc, 3, 3).cuda(),
                    right_eye_warp=warps_for(B * Tc, IH, IW, seed=B + 1).view(B, Tc, 3, 3).cuda())
        g = torch.Generator().manual_seed(B * 1000 + Tc)
        cl, cam, cam_lin = surface_pair('nv12', (B, Tc), IH, IW, gen=g)
        sl, scr, scr_lin = surface_pair('nv12', (B, Tc), IH, IW, gen=g)
        model.eye_net.camera_layout, model.refine_net.screen_layout = cl, sl
        streams = {'surface': (eve_amd.EVEStream(model, B), dict(rest, camera_surface=cam, screen_surface=scr)),
                   'nv12': (eve_amd.EVEStream(model, B), dict(rest, camera_frame_nv12=cam_lin, screen_frame_nv12=scr_lin))}
        outs = {}
        for name, (s, chunk) in streams.items():
            for _ in range(3):
                outs[name] = s.step(chunk)       # capture + warm replays
        torch.cuda.synchronize()
        assert all(torch.equal(outs['surface'][k_], outs['nv12'][k_]) for k_ in outs['nv12']), 'the two steps disagree'
        times = {name: [] for name in streams}
        for _ in range(args.rounds):
            for name, (s, chunk) in streams.items():
                times[name].append(device_ms(lambda: s.step(chunk), args.steps))
        res = {'B': B, 'Tc': Tc, 'dtype': args.dtype, 'frame': '%dx%d' % (IW, IH), 'steps': args.steps, 'rounds': args.rounds}
        for name, t in times.items():
            res[name + '_step_ms'] = round(median(t), 4)
            res[name + '_step_ms_min_max'] = [round(min(t), 4), round(max(t), 4)]
        res['surface_minus_nv12_ms'] = round(res['surface_step_ms'] - res['nv12_step_ms'], 4)
        res['MB_copied'] = {'surface': round((cam.numel() + scr.numel()) / 1e6, 1), 'nv12': round((cam_lin.numel() + scr_lin.numel()) / 1e6, 1)}
        rows.append(res)
        print(json.dumps(res), flush=True)
        del streams, cam, scr, cam_lin, scr_lin
        torch.cuda.empty_cache()
    return rows


def launches(args, IH, IW):
    k = default_kernels()
    N = args.patches
    torch.manual_seed(N)
    frames = torch.randint(0, 256, (N, IH, IW, 3), dtype=torch.uint8, device='cuda')
    warps = warps_for(N, IH, IW, seed=N).cuda()
    crops = torch.randint(0, 256, (N,) + HW + (3,), dtype=torch.uint8, device='cuda')
    packed = torch.empty((N, HW[0] + 6, HW[1] + 8, 4), dtype=torch.bfloat16, device='cuda')
    routes = {'warp_nchw': lambda: k.eye_warp_u8_to_nchw(frames, warps, HW),
              'warp_stem': lambda: k.eye_warp_u8_to_stem(frames, warps, HW, out=packed),
              'crop_nchw': lambda: k.frames_u8_to_nchw(crops, 2.0 / 255.0, -1.0),
              'crop_stem': lambda: k.frames_u8_to_stem(crops, 2.0 / 255.0, -1.0, out=packed)}
    if args.lens:
        lens = lens_rows(N, IH, IW).cuda()
        routes['lens_nchw'] = lambda: k.eye_warp_lens_u8_to_nchw(frames, warps, lens, HW)
        routes['lens_stem'] = lambda: k.eye_warp_lens_u8_to_stem(frames, warps, lens, HW, out=packed)
    if args.pose:
        import ctypes
        rows = pose_rows(N, IH, IW, seed=N).cuda()
        outs = [torch.empty(shape, device='cuda') for shape in ((N, 9), (2, N, 3), (2, N, 9), (2, N, 9), (2, N, 2))]
        outs.append(torch.empty((2, N), dtype=torch.uint8, device='cuda'))
        ptrs = [ctypes.c_void_p(t.data_ptr()) for t in [rows] + outs]

        def pose_launch():
            status = k.lib.eve_eye_pose_normalize(N, ptrs[0], HW[0], HW[1], *ptrs[1:], ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert status == 0, k.lib.eve_last_error()
        routes['pose_normalize'] = pose_launch
    slow = set()
    if args.format:
        fmt = args.format
        raw = format_frames(fmt, (N,), IH, IW)
        routes['fmt_nchw'] = lambda: k.eye_warp_fmt_to_nchw(raw, warps, HW, fmt)
        routes['fmt_stem'] = lambda: k.eye_warp_fmt_to_stem(raw, warps, HW, fmt, out=packed)
        routes['conv_only'] = lambda: to_rgb_device(raw, fmt, IH, IW)
        routes['conv_nchw'] = lambda: k.eye_warp_u8_to_nchw(to_rgb_device(raw, fmt, IH, IW), warps, HW)
        routes['conv_stem'] = lambda: k.eye_warp_u8_to_stem(to_rgb_device(raw, fmt, IH, IW), warps, HW, out=packed)
        slow = {'conv_only', 'conv_nchw', 'conv_stem'}
        assert torch.equal(routes['fmt_nchw'](), routes['conv_nchw']()), 'the direct launch and convert-then-warp disagree'
    for fn in routes.values():                   # warm up: code objects, allocator
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in routes}
    for _ in range(args.rounds):
        for name, fn in routes.items():
            times[name].append(device_ms(fn, max(1, args.iters // 20) if name in slow else args.iters))
    pixels = N * HW[0] * HW[1]
    stored = {'nchw': pixels * 3 * 4, 'stem': packed.numel() * 2}
    res = {'patches': N, 'frame': '%dx%d' % (IW, IH), 'patch': '%dx%d' % HW, 'iters': args.iters, 'rounds': args.rounds}
    for name, t in times.items():
        res[name + '_us'] = round(1e3 * median(t), 2)
        res[name + '_us_min_max'] = [round(1e3 * min(t), 2), round(1e3 * max(t), 2)]
    for form in ('nchw', 'stem'):
        res['warp_%s_bytes' % form] = pixels * 12 + stored[form]
        res['warp_%s_GBps' % form] = round(res['warp_%s_bytes' % form] / (1e-3 * median(times['warp_' + form])) / 1e9, 1)
        res['crop_%s_bytes' % form] = pixels * 3 + stored[form]
        res['crop_%s_GBps' % form] = round(res['crop_%s_bytes' % form] / (1e-3 * median(times['crop_' + form])) / 1e9, 1)
        if args.lens:
            res['lens_%s_bytes' % form] = res['warp_%s_bytes' % form]
            res['lens_%s_GBps' % form] = round(res['lens_%s_bytes' % form] / (1e-3 * median(times['lens_' + form])) / 1e9, 1)
            res['lens_over_warp_%s' % form] = round(median(times['lens_' + form]) / median(times['warp_' + form]), 3)
    if args.format:
        res['format'] = args.format
        res['frame_bytes'] = {'rgb': frames[0].numel(), args.format: raw[0].numel()}
        for form in ('nchw', 'stem'):
            res['fmt_over_warp_%s' % form] = round(median(times['fmt_' + form]) / median(times['warp_' + form]), 3)
            res['conv_over_fmt_%s' % form] = round(median(times['conv_' + form]) / median(times['fmt_' + form]), 2)
        k.eye_warp_fmt_to_stem(raw, warps, HW, args.format, out=packed)
        res['fmt_kernel'] = k.lib.eve_last_kernel().decode()
    if args.pose:
        assert outs[5].all(), 'bench poses must be valid'
        pose_launch()
        res['pose_kernel'] = k.lib.eve_last_kernel().decode()
    k.eye_warp_u8_to_stem(frames, warps, HW, out=packed)
    res['kernel'] = k.lib.eve_last_kernel().decode()
    if args.lens:
        k.eye_warp_lens_u8_to_stem(frames, warps, lens, HW, out=packed)
        res['lens_kernel'] = k.lib.eve_last_kernel().decode()
    return res


class _HuberStream:
    """An EVEStream whose steps run with model.eye_net.face_huber_px = k (the graph's key holds the value, so the other streams of
    the same model keep theirs)."""

    def __init__(self, stream, model, k):
        self.stream, self.model, self.k = stream, model, k

    def step(self, chunk):
        self.model.eye_net.face_huber_px = self.k
        try:
            return self.stream.step(chunk)
        finally:
            self.model.eye_net.face_huber_px = None


def stream_steps(args, IH, IW):
    cfg = eve_amd.reset_standalone_config()
    cfg.import_json(os.path.join(REPO, 'configs', 'refine_net.json'))
    cfg.import_dict({'eye_net_load_pretrained': False})
    model = eve_amd.EVE(output_predictions=True)
    model.eye_net.compute_dtype = model.refine_net.compute_dtype = DTYPES[args.dtype]
    detweights.fill_module(model.eye_net, 0)
    detweights.fill_module(model.refine_net, 1)
    model = model.cuda().eval()
    rows = []
    for shape in args.shapes:
        B, Tc = (int(v) for v in shape.split('x'))
        small = detweights.eve_batch(min(B, 4), Tc, seed=1)
        rest = {k_: torch.cat([small[k_]] * ((B + 3) // 4), dim=0)[:B].contiguous().cuda() for k_ in STREAM_KEYS if k_ in small}
        g = torch.Generator().manual_seed(B * 1000 + Tc)
        cam = dict(rest, camera_frame=torch.randint(0, 256, (B, Tc, IH, IW, 3), generator=g, dtype=torch.uint8).cuda(),
                   left_eye_warp=warps_for(B * Tc, IH, IW, seed=B).view(B, Tc, 3, 3).cuda(),
                   right_eye_warp=warps_for(B * Tc, IH, IW, seed=B + 1).view(B, Tc, 3, 3).cuda())
        pat = dict(rest, left_eye_patch=torch.randint(0, 256, (B, Tc) + HW + (3,), generator=g, dtype=torch.uint8).cuda(),
                   right_eye_patch=torch.randint(0, 256, (B, Tc) + HW + (3,), generator=g, dtype=torch.uint8).cuda())
        streams = {'camera': (eve_amd.EVEStream(model, B), cam), 'patches': (eve_amd.EVEStream(model, B), pat)}
        if args.lens:
            streams['lens'] = (eve_amd.EVEStream(model, B), dict(cam, camera_lens=lens_rows(B * Tc, IH, IW).view(B, Tc, 12).cuda()))
        if args.pose:
            from eve_amd.eye_net import EYE_POSE_DERIVED
            streams['pose'] = (eve_amd.EVEStream(model, B), dict({k_: v for k_, v in cam.items() if k_ not in EYE_POSE_DERIVED},
                                                                 eye_pose=pose_rows(B * Tc, IH, IW, seed=B).view(B, Tc, 18).cuda()))
        if args.landmarks:
            from eve_amd.eye_net import EYE_POSE_DERIVED
            lm, rig = face_sequences(B, Tc, 68, IH, IW, seed=B)
            streams['face'] = (eve_amd.EVEStream(model, B), dict({k_: v for k_, v in cam.items() if k_ not in EYE_POSE_DERIVED},
                                                                 face_landmarks=torch.from_numpy(lm).cuda(), face_rig=torch.from_numpy(rig).cuda()))
        if args.landmarks and args.raw:
            raw_np, rig_np, lens_np, _ = raw_face_sequences(B, Tc, 68, IH, IW, seed=B)
            streams['raw'] = (_HuberStream(eve_amd.EVEStream(model, B), model, args.huber),
                              dict({k_: v for k_, v in cam.items() if k_ not in EYE_POSE_DERIVED}, face_landmarks_raw=torch.from_numpy(raw_np).cuda(),
                                   face_rig=torch.from_numpy(rig_np).cuda(), camera_lens=torch.from_numpy(lens_np).cuda()))
            if args.lens:                        # what `raw` stands beside: the same pixels' undistortion, landmarks of the undistorted image
                streams['face_lens'] = (eve_amd.EVEStream(model, B), dict(streams['face'][1], camera_lens=torch.from_numpy(lens_np).cuda()))
        if args.format:
            fmt_chunk = {k_: v for k_, v in cam.items() if k_ != 'camera_frame'}
            fmt_chunk['camera_frame_' + args.format] = format_frames(args.format, (B, Tc), IH, IW, gen=g)
            streams['fmt'] = (eve_amd.EVEStream(model, B), fmt_chunk)
        for s, chunk in streams.values():
            for _ in range(3):
                s.step(chunk)                    # capture + warm replays
        torch.cuda.synchronize()
        times = {name: [] for name in streams}
        for _ in range(args.rounds):
            for name, (s, chunk) in streams.items():
                times[name].append(device_ms(lambda: s.step(chunk), args.steps))
        res = {'B': B, 'Tc': Tc, 'dtype': args.dtype, 'frame': '%dx%d' % (IW, IH), 'steps': args.steps, 'rounds': args.rounds}
        for name, t in times.items():
            res[name + '_step_ms'] = round(median(t), 4)
            res[name + '_step_ms_min_max'] = [round(min(t), 4), round(max(t), 4)]
        res['camera_minus_patches_ms'] = round(res['camera_step_ms'] - res['patches_step_ms'], 4)
        if args.lens:
            res['lens_minus_camera_ms'] = round(res['lens_step_ms'] - res['camera_step_ms'], 4)
        if args.pose:
            res['pose_minus_camera_ms'] = round(res['pose_step_ms'] - res['camera_step_ms'], 4)
        res['camera_frame_MB_copied'] = round(B * Tc * IH * IW * 3 / 1e6, 1)
        if args.landmarks:
            res['face_minus_pose_ms'] = round(res['face_step_ms'] - res['pose_step_ms'], 4)
            res['face_pose_valid'] = round(float(streams['face'][0].step(streams['face'][1])['pose_valid'].float().mean()), 4)
        if args.landmarks and args.raw:
            res['raw_huber_px'] = args.huber
            res['raw_minus_face_ms'] = round(res['raw_step_ms'] - res['face_step_ms'], 4)
            if args.lens:
                res['raw_minus_face_lens_ms'] = round(res['raw_step_ms'] - res['face_lens_step_ms'], 4)
            last = streams['raw'][0].step(streams['raw'][1])
            res['raw_pose_valid'] = round(float(last['pose_valid'].float().mean()), 4)
            res['raw_inliers_min_max'] = [int(last['face_inliers'].min()), int(last['face_inliers'].max())]
        if args.format:
            res['fmt_minus_camera_ms'] = round(res['fmt_step_ms'] - res['camera_step_ms'], 4)
            res['fmt_frame_MB_copied'] = round(fmt_chunk['camera_frame_' + args.format].numel() / 1e6, 1)
        rows.append(res)
        print(json.dumps(res), flush=True)
        del streams, cam, pat
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--patches', type=int, default=64)
    ap.add_argument('--size', default='1920x1080', metavar='WxH')
    ap.add_argument('--iters', type=int, default=500)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--shapes', nargs='*', default=['1x1', '8x4', '32x2'], help='EVEStream B x Tc shapes (none: skip part 2)')
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--dtype', default='bf16', choices=sorted(DTYPES))
    ap.add_argument('--lens', action='store_true', help='also time the lens launches and an EVEStream step with camera_lens')
    ap.add_argument('--pose', action='store_true', help='also time eve_eye_pose_normalize and an EVEStream step with eye_pose rows')
    ap.add_argument('--format', default=None, choices=['bgr', 'nv12', 'i420', 'yuyv'],
                    help='also time the launches and an EVEStream step on frames in this layout, and convert-then-warp beside them')
    ap.add_argument('--landmarks', action='store_true',
                    help='also time eve_face_pose_solve and an EVEStream step with face_landmarks + face_rig (implies --pose)')
    ap.add_argument('--raw', action='store_true',
                    help='with --landmarks: also time eve_face_pose_solve_ex next to the plain launch and an EVEStream step with face_landmarks_raw + camera_lens')
    ap.add_argument('--huber', type=float, default=None, metavar='K', help='with --raw: the Huber loss of K pixels (face_huber_px) in those')
    ap.add_argument('--surface', action='store_true',
                    help='time the surface launches and an EVEStream step with camera_surface + screen_surface instead (NV12 / P010 in 2048 x 1088)')
    ap.add_argument('--markdown', default=None, help='also write the tables to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_eye_warp: no GPU (a time is only measured on one)')
    IW, IH = (int(v) for v in args.size.lower().split('x'))
    if args.surface:
        with torch.no_grad():
            surface_launches(args, IH, IW)
            surface_steps(args, IH, IW)
        return
    args.pose = args.pose or args.landmarks
    with torch.no_grad():
        solves = solve_launches(args, IH, IW) if args.landmarks else []
        raw_solves = raw_solve_launches(args, IH, IW) if args.landmarks and args.raw else None
        one = launches(args, IH, IW)
        print(json.dumps(one), flush=True)
        rows = stream_steps(args, IH, IW) if args.shapes else []
    lines = ['| launch (%d patches, %s frames) | us | min .. max | bytes | GB/s |' % (one['patches'], one['frame']), '|---|---|---|---|---|']
    if args.pose:
        one['pose_normalize_bytes'] = one['patches'] * (18 * 4 + 9 * 4 + 2 * (3 + 9 + 9 + 2) * 4 + 2)
        one['pose_normalize_GBps'] = round(one['pose_normalize_bytes'] / (1e-6 * one['pose_normalize_us']) / 1e9, 2)
    names = ('warp_nchw', 'lens_nchw', 'crop_nchw', 'warp_stem', 'lens_stem', 'crop_stem') if args.lens else ('warp_nchw', 'crop_nchw', 'warp_stem', 'crop_stem')
    for name in names + (('pose_normalize',) if args.pose else ()):
        lines.append('| %s | %.2f | %.2f .. %.2f | %d | %.1f |' % (name, one[name + '_us'], one[name + '_us_min_max'][0], one[name + '_us_min_max'][1],
                                                                  one[name + '_bytes'], one[name + '_GBps']))
    if rows:
        lines += ['', '| B x Tc (%s) | camera step ms | patches step ms | difference ms | frames copied MB |' % args.dtype, '|---|---|---|---|---|']
        for r in rows:
            lines.append('| %d x %d | %.4f | %.4f | %.4f | %.1f |' % (r['B'], r['Tc'], r['camera_step_ms'], r['patches_step_ms'],
                                                                      r['camera_minus_patches_ms'], r['camera_frame_MB_copied']))
    if rows and args.lens:
        lines += ['', '| B x Tc (%s) | lens step ms | min .. max | camera step ms | min .. max | lens - camera ms |' % args.dtype, '|---|---|---|---|---|---|']
        for r in rows:
            lines.append('| %d x %d | %.4f | %.4f .. %.4f | %.4f | %.4f .. %.4f | %.4f |' % (
                r['B'], r['Tc'], r['lens_step_ms'], r['lens_step_ms_min_max'][0], r['lens_step_ms_min_max'][1], r['camera_step_ms'],
                r['camera_step_ms_min_max'][0], r['camera_step_ms_min_max'][1], r['lens_minus_camera_ms']))
    if rows and args.pose:
        lines += ['', '| B x Tc (%s) | pose step ms | min .. max | camera step ms | min .. max | pose - camera ms |' % args.dtype, '|---|---|---|---|---|---|']
        for r in rows:
            lines.append('| %d x %d | %.4f | %.4f .. %.4f | %.4f | %.4f .. %.4f | %.4f |' % (
                r['B'], r['Tc'], r['pose_step_ms'], r['pose_step_ms_min_max'][0], r['pose_step_ms_min_max'][1], r['camera_step_ms'],
                r['camera_step_ms_min_max'][0], r['camera_step_ms_min_max'][1], r['pose_minus_camera_ms']))
    if args.format:
        lines += ['', '| %s launch (%d patches, %s frames) | us | min .. max |' % (args.format, one['patches'], one['frame']), '|---|---|---|']
        for name in ('warp_nchw', 'fmt_nchw', 'conv_nchw', 'warp_stem', 'fmt_stem', 'conv_stem', 'conv_only'):
            lines.append('| %s | %.2f | %.2f .. %.2f |' % (name, one[name + '_us'], one[name + '_us_min_max'][0], one[name + '_us_min_max'][1]))
    if rows and args.format:
        lines += ['', '| B x Tc (%s) | %s step ms | min .. max | camera step ms | min .. max | %s - camera ms | MB copied %s | MB copied rgb |' % (
            args.dtype, args.format, args.format, args.format), '|---|---|---|---|---|---|---|---|']
        for r in rows:
            lines.append('| %d x %d | %.4f | %.4f .. %.4f | %.4f | %.4f .. %.4f | %.4f | %.1f | %.1f |' % (
                r['B'], r['Tc'], r['fmt_step_ms'], r['fmt_step_ms_min_max'][0], r['fmt_step_ms_min_max'][1], r['camera_step_ms'],
                r['camera_step_ms_min_max'][0], r['camera_step_ms_min_max'][1], r['fmt_minus_camera_ms'], r['fmt_frame_MB_copied'],
                r['camera_frame_MB_copied']))
    if solves:
        lines += ['', '| face_pose_solve S x T, L | cold us | min .. max | warm us | min .. max | warm us / frame | T = 1 all cold us | accepted steps cold | warm | frames solved |',
                  '|---|---|---|---|---|---|---|---|---|---|']
        for r in solves:
            lines.append('| %d x %d, %d | %.2f | %.2f .. %.2f | %.2f | %.2f .. %.2f | %.2f | %.2f | %d .. %d | %d .. %d | %.4f |' % (
                r['S'], r['T'], r['L'], r['cold_us'], r['cold_us_min_max'][0], r['cold_us_min_max'][1], r['warm_us'], r['warm_us_min_max'][0],
                r['warm_us_min_max'][1], r['warm_us_per_frame'], r['all_cold_us'], r['accepted_cold_first_frame'][0],
                r['accepted_cold_first_frame'][1], r['accepted_warm_frames'][0], r['accepted_warm_frames'][1], r['frames_solved']))
    if rows and args.landmarks:
        lines += ['', '| B x Tc (%s) | face step ms | min .. max | pose step ms | min .. max | face - pose ms |' % args.dtype, '|---|---|---|---|---|---|']
        for r in rows:
            lines.append('| %d x %d | %.4f | %.4f .. %.4f | %.4f | %.4f .. %.4f | %.4f |' % (
                r['B'], r['Tc'], r['face_step_ms'], r['face_step_ms_min_max'][0], r['face_step_ms_min_max'][1], r['pose_step_ms'],
                r['pose_step_ms_min_max'][0], r['pose_step_ms_min_max'][1], r['face_minus_pose_ms']))
    if raw_solves:
        r = raw_solves
        lines += ['', '| launch, %d x %d, L = %d | cold us | min .. max | warm us | min .. max | frames solved |' % (r['S'], r['T'], r['L']), '|---|---|---|---|---|---|']
        for name in ('plain', 'ex_off', 'ex_lens') + (('ex_huber', 'ex_lens_huber') if args.huber else ()):
            lines.append('| %s | %.2f | %.2f .. %.2f | %.2f | %.2f .. %.2f | %.4f |' % (
                name, r[name + '_cold_us'], r[name + '_cold_us_min_max'][0], r[name + '_cold_us_min_max'][1], r[name + '_warm_us'],
                r[name + '_warm_us_min_max'][0], r[name + '_warm_us_min_max'][1], r[name + '_frames_solved']))
    if rows and args.landmarks and args.raw:
        lines += ['', '| B x Tc (%s) | raw step ms (huber %s) | min .. max | face step ms | min .. max | raw - face ms |' % (args.dtype, args.huber),
                  '|---|---|---|---|---|---|']
        for r in rows:
            lines.append('| %d x %d | %.4f | %.4f .. %.4f | %.4f | %.4f .. %.4f | %.4f |' % (
                r['B'], r['Tc'], r['raw_step_ms'], r['raw_step_ms_min_max'][0], r['raw_step_ms_min_max'][1], r['face_step_ms'],
                r['face_step_ms_min_max'][0], r['face_step_ms_min_max'][1], r['raw_minus_face_ms']))
    table = '\n'.join(lines)
    print(table, flush=True)
    if args.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(args.markdown)), exist_ok=True)
        with open(args.markdown, 'w') as f:
            f.write(table + '\n')


if __name__ == '__main__':
    main()
