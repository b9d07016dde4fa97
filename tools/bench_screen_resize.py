#!/usr/bin/env python
"""Device time of the screen-capture area resize (eve_screen_u8_area_to_nchw, csrc/screen_resize.hip) next to two yardsticks, the
three routes interleaved in one process:

    area    HipKernels.screen_u8_area_to_nchw(frames, (72, 128)): reads N*IH*IW*C bytes once, writes 110 KB per frame
    clone   frames.clone(): a read plus a write of the same bytes -- a read-only kernel's floor is about half of it
    aten    what a caller had before: permute + float + F.interpolate(mode='area') + scale (a float tensor four times the
            capture; for fractional ratios not the same values)

    python tools/bench_screen_resize.py [--sizes 1920x1080 2560x1440] [--frames 1 32 240] [--channels 3] [--iters 20] [--rounds 5]
                                        [--markdown profiles/table.md] [--format rgb|bgr|nv12|i420|yuyv] [--surface]
                                        [--luminance [--radii 60,200]]

One JSON line per (size, N): per route the median over the rounds of the device time per call (events around `iters` calls), and
for `area` and `clone` the rate N*IH*IW*C / time as a fraction of the 8 TB/s HBM peak (`clone` moves twice those bytes).  Every
route rotates over enough separately allocated captures to exceed the 256 MiB Infinity Cache, so the reads come from HBM; a live
caller whose capture was just copied in may see it served from that cache instead.

--format bgr times eve_screen_u8_area_bgr_to_nchw as `area`.  --format nv12 | i420 | yuyv measures the capture as a decoder
delivers it (eve_screen_area_fmt_to_nchw), three other routes interleaved round by round in one process:

    fmt        HipKernels.screen_area_fmt_to_nchw(buf, (72, 128), format): N*IH*IW*3/2 bytes (YUYV: *2) read once, converted in registers
    rgb        HipKernels.screen_u8_area_to_nchw on the SAME frames converted beforehand (conversion not timed): the launch the new one stands beside
    torch+rgb  what a caller had before: a whole-frame conversion with torch (the same integer matrix), then the RGB launch

One JSON line per (size, N) with each route's median, minimum and maximum over the rounds.

--surface measures the capture as it lies in a decoder's memory (eve_screen_area_surface_to_nchw): NV12 in rows of 2048 bytes and
1088 coded rows, then P010 in rows of 4096 -- the routes interleaved round by round in one process:

    linear       HipKernels.screen_area_fmt_to_nchw on the linearised NV12 frames: the launch the new one stands beside
    surface      HipKernels.screen_area_surface_to_nchw on the padded buffer (NV12: the vector form; P010: the generic form)
    copy+linear  what a caller had before: a torch de-pitch copy (P010: the high bytes) into byte-linear NV12, then `linear`;
                 copy_only is that pass alone

--luminance measures eve_screen_luminance (csrc/screen_luminance.hip) on --format rgb | nv12 | i420 | yuyv frames, or with --surface on
NV12 in rows of 2048 bytes and 1088 coded rows, beside the resize of the SAME frames through the same SurfaceLayout, the two
interleaved round by round in one process:

    resize      HipKernels.screen_area_surface_to_nchw(buf, (72, 128), layout): the launch the new one stands beside
    luminance   HipKernels.screen_luminance(buf, layout, ...): two memsets, the kernel and the finish kernel; --radii 60,200 adds discs
                around random centres on the screen

`bytes` is what the address rule names (the visible pixels' samples), and the rates are bytes / time over 8 TB/s."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from eve_amd.kernels import default_kernels  # noqa: E402

HBM_PEAK = 8.0e12
OUT_HW = (72, 128)
ROTATE_BYTES = 512 << 20


def device_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(i)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def aten_route(frames):
    x = frames[..., :3].permute(0, 3, 1, 2).float()
    return F.interpolate(x, size=OUT_HW, mode='area') * (1.0 / 255.0)


def bench_format(args, k):
    """The --format nv12 | i420 | yuyv measurement: one JSON line per (size, N)."""
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    from bench_eye_warp import format_frames, to_rgb_device
    fmt = args.format
    for size in args.sizes:
        IW, IH = (int(v) for v in size.lower().split('x'))
        for N in args.frames:
            nbytes = N * IH * IW * (2 if fmt == 'yuyv' else 3) // (1 if fmt == 'yuyv' else 2)
            copies = max(2, min(64, -(-ROTATE_BYTES // nbytes)))
            torch.manual_seed(N + IW)
            bufs = [format_frames(fmt, (N,), IH, IW) for _ in range(2)]
            bufs += [bufs[i % 2].clone() for i in range(copies - 2)]
            rgbs = [to_rgb_device(b, fmt, IH, IW) for b in bufs[:2]]
            rgbs += [rgbs[i % 2].clone() for i in range(2 * copies - 2)]                    # twice the captures: the same bytes rotated
            routes = {'fmt': lambda i: k.screen_area_fmt_to_nchw(bufs[i % copies], OUT_HW, fmt),
                      'rgb': lambda i: k.screen_u8_area_to_nchw(rgbs[i % len(rgbs)], OUT_HW),
                      'torch+rgb': lambda i: k.screen_u8_area_to_nchw(to_rgb_device(bufs[i % copies], fmt, IH, IW), OUT_HW)}
            with torch.no_grad():
                assert torch.equal(routes['fmt'](0), routes['rgb'](0)) and torch.equal(routes['fmt'](1), routes['torch+rgb'](1))
                for fn in routes.values():               # warm up: code objects, allocator
                    for i in range(3):
                        fn(i)
                torch.cuda.synchronize()
                times = {name: [] for name in routes}
                for _ in range(args.rounds):
                    for name, fn in routes.items():
                        times[name].append(device_ms(fn, max(2, args.iters // 4) if name == 'torch+rgb' else args.iters))
            res = {'size': size, 'N': N, 'format': fmt, 'bytes': nbytes, 'rgb_bytes': N * IH * IW * 3, 'captures_rotated': copies}
            for name, t in times.items():
                res[name + '_us'] = round(1e3 * sorted(t)[len(t) // 2], 2)
                res[name + '_us_min_max'] = [round(1e3 * min(t), 2), round(1e3 * max(t), 2)]
            res['fmt_frac_of_8TBps'] = round(nbytes / (1e-6 * res['fmt_us']) / HBM_PEAK, 4)
            res['rgb_frac_of_8TBps'] = round(res['rgb_bytes'] / (1e-6 * res['rgb_us']) / HBM_PEAK, 4)
            k.screen_area_fmt_to_nchw(bufs[0], OUT_HW, fmt)
            res['kernel'] = k.lib.eve_last_kernel().decode()
            print(json.dumps(res), flush=True)
            del bufs, rgbs, routes
            torch.cuda.empty_cache()


def bench_surface(args, k):
    """The --surface measurement: one JSON line per (size, N, layout)."""
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    from bench_eye_warp import depitch, surface_pair
    for size in args.sizes:
        IW, IH = (int(v) for v in size.lower().split('x'))
        pitch_px, coded = -(-IW // 256) * 256 + (256 if IW % 256 == 0 else 0), -(-IH // 16) * 16 + (16 if IH % 16 == 0 else 0)
        for N in args.frames:
            for fmt in ('nv12', 'p010'):
                torch.manual_seed(N + IW)
                L, first, _ = surface_pair(fmt, (N,), IH, IW, pitch_px, coded)
                copies = max(2, min(64, -(-ROTATE_BYTES // first.numel())))
                bufs = [first] + [surface_pair(fmt, (N,), IH, IW, pitch_px, coded)[1]]
                bufs += [bufs[i % 2].clone() for i in range(copies - 2)]
                lins = [depitch(b, fmt, IH, IW, coded) for b in bufs]
                routes = {'linear': lambda i: k.screen_area_fmt_to_nchw(lins[i % copies], OUT_HW, 'nv12'),
                          'surface': lambda i: k.screen_area_surface_to_nchw(bufs[i % copies], OUT_HW, L),
                          'copy+linear': lambda i: k.screen_area_fmt_to_nchw(depitch(bufs[i % copies], fmt, IH, IW, coded), OUT_HW, 'nv12'),
                          'copy_only': lambda i: depitch(bufs[i % copies], fmt, IH, IW, coded)}
                slow = {'copy+linear', 'copy_only'}
                with torch.no_grad():
                    assert torch.equal(routes['surface'](0), routes['linear'](0)) and torch.equal(routes['surface'](1), routes['copy+linear'](1))
                    for fn in routes.values():               # warm up: code objects, allocator
                        for i in range(3):
                            fn(i)
                    torch.cuda.synchronize()
                    times = {name: [] for name in routes}
                    for _ in range(args.rounds):
                        for name, fn in routes.items():
                            times[name].append(device_ms(fn, max(2, args.iters // 4) if name in slow else args.iters))
                res = {'size': size, 'N': N, 'surface': fmt, 'pitch': L.pitch, 'coded_height': coded, 'surface_bytes': first.numel(),
                       'visible_bytes': N * IH * IW * 3 // 2 * (2 if fmt == 'p010' else 1), 'linear_bytes': lins[0].numel(), 'captures_rotated': copies}
                for name, t in times.items():
                    res[name + '_us'] = round(1e3 * sorted(t)[len(t) // 2], 2)
                    res[name + '_us_min_max'] = [round(1e3 * min(t), 2), round(1e3 * max(t), 2)]
                res['surface_over_linear'] = round(res['surface_us'] / res['linear_us'], 3)
                res['pitch_over_width'] = round(pitch_px / IW, 3)
                res['copy_plus_linear_over_surface'] = round(res['copy+linear_us'] / res['surface_us'], 2)
                routes['surface'](0)
                res['kernel'] = k.lib.eve_last_kernel().decode()
                print(json.dumps(res), flush=True)
                del bufs, lins, routes, first
                torch.cuda.empty_cache()


def bench_luminance(args, k):
    """The --luminance measurement: one JSON line per (size, N)."""
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    from bench_eye_warp import format_frames, surface_pair
    from eve_amd.data import SurfaceLayout, display_response
    from eve_amd.kernels import LUM_REC709
    radii = tuple(int(v) for v in args.radii.split(',')) if args.radii else ()
    table = display_response().cuda()
    for size in args.sizes:
        IW, IH = (int(v) for v in size.lower().split('x'))
        for N in args.frames:
            torch.manual_seed(N + IW)
            if args.surface:
                fmt = 'nv12'
                L, first, _ = surface_pair('nv12', (N,), IH, IW, 2048, 1088)
                make = lambda: surface_pair('nv12', (N,), IH, IW, 2048, 1088)[1]
            else:
                fmt = args.format
                L = SurfaceLayout(fmt, IW, IH)
                make = (lambda: torch.randint(0, 256, (N, IH, IW, 3), dtype=torch.uint8, device='cuda')) if fmt == 'rgb' else \
                    (lambda: format_frames(fmt, (N,), IH, IW))
                first = make()
            nbytes = N * IH * IW * {'rgb': 6, 'nv12': 3, 'i420': 3, 'yuyv': 4}[fmt] // 2
            copies = max(2, min(64, -(-ROTATE_BYTES // first.numel())))
            bufs = [first, make()]
            bufs += [bufs[i % 2].clone() for i in range(copies - 2)]
            bufs = [b.reshape(N, -1) for b in bufs]
            centres = (torch.rand((N, 2), device='cuda') * torch.tensor([IW, IH], device='cuda')).contiguous() if radii else None
            routes = {'resize': lambda i: k.screen_area_surface_to_nchw(bufs[i % copies], OUT_HW, L),
                      'luminance': lambda i: k.screen_luminance(bufs[i % copies], L, table, LUM_REC709, N, 1, radii=radii, centres=centres)}
            with torch.no_grad():
                for fn in routes.values():               # warm up: code objects, allocator
                    for i in range(3):
                        fn(i)
                torch.cuda.synchronize()
                times = {name: [] for name in routes}
                for _ in range(args.rounds):
                    for name, fn in routes.items():
                        times[name].append(device_ms(fn, args.iters))
            res = {'size': size, 'N': N, 'format': fmt, 'surface': bool(args.surface), 'pitch': L.pitch, 'radii': list(radii), 'bytes': nbytes,
                   'buffer_bytes': first.numel(), 'captures_rotated': copies}
            for name, t in times.items():
                res[name + '_us'] = round(1e3 * sorted(t)[len(t) // 2], 2)
                res[name + '_us_min_max'] = [round(1e3 * min(t), 2), round(1e3 * max(t), 2)]
                res[name + '_frac_of_8TBps'] = round(nbytes / (1e-6 * res[name + '_us']) / HBM_PEAK, 4)
            res['luminance_over_resize'] = round(res['luminance_us'] / res['resize_us'], 3)
            routes['luminance'](0)
            res['kernel'] = k.lib.eve_last_kernel().decode()
            print(json.dumps(res), flush=True)
            del bufs, routes, first
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', nargs='+', default=['1920x1080', '2560x1440'])
    ap.add_argument('--frames', nargs='+', type=int, default=[1, 32, 240])
    ap.add_argument('--channels', type=int, default=3, choices=(3, 4))
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--markdown', default=None, help='also write the table to this file')
    ap.add_argument('--format', default='rgb', choices=('rgb', 'bgr', 'nv12', 'i420', 'yuyv'), help='the capture\'s layout (see above)')
    ap.add_argument('--surface', action='store_true', help='measure eve_screen_area_surface_to_nchw on padded NV12 / P010 surfaces instead (see above)')
    ap.add_argument('--luminance', action='store_true', help='measure eve_screen_luminance beside the resize of the same frames (see above)')
    ap.add_argument('--radii', default='', help='with --luminance: disc radii in capture pixels, e.g. 60,200')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_screen_resize: no GPU (a time is only measured on one)')
    k = default_kernels()
    if args.luminance:
        if args.format == 'bgr':
            ap.error('--luminance takes --format rgb, nv12, i420 or yuyv, or --surface')
        return bench_luminance(args, k)
    if args.surface:
        return bench_surface(args, k)
    if args.format in ('nv12', 'i420', 'yuyv'):
        return bench_format(args, k)
    area = k.screen_u8_area_bgr_to_nchw if args.format == 'bgr' else k.screen_u8_area_to_nchw
    rows = []
    for size in args.sizes:
        IW, IH = (int(v) for v in size.lower().split('x'))
        for N in args.frames:
            nbytes = N * IH * IW * args.channels
            copies = max(1, min(64, -(-ROTATE_BYTES // nbytes)))
            torch.manual_seed(N + IW)
            caps = [torch.randint(0, 256, (N, IH, IW, args.channels), dtype=torch.uint8, device='cuda') for _ in range(min(copies, 2))]
            caps += [caps[i % 2].clone() for i in range(copies - len(caps))]
            routes = {'area': lambda i: area(caps[i % copies], OUT_HW),
                      'clone': lambda i: caps[i % copies].clone(),
                      'aten': lambda i: aten_route(caps[i % copies])}
            with torch.no_grad():
                for fn in routes.values():               # warm up: code objects, allocator
                    for i in range(3):
                        fn(i)
                torch.cuda.synchronize()
                times = {name: [] for name in routes}
                for _ in range(args.rounds):
                    for name, fn in routes.items():
                        times[name].append(device_ms(fn, args.iters))
            med = {name: sorted(t)[len(t) // 2] for name, t in times.items()}
            res = {'size': size, 'N': N, 'C': args.channels, 'format': args.format, 'bytes': nbytes, 'captures_rotated': copies,
                   'area_us': round(1e3 * med['area'], 2), 'clone_us': round(1e3 * med['clone'], 2), 'aten_us': round(1e3 * med['aten'], 2),
                   'area_us_min_max': [round(1e3 * min(times['area']), 2), round(1e3 * max(times['area']), 2)],
                   'area_frac_of_8TBps': round(nbytes / (1e-3 * med['area']) / HBM_PEAK, 4),
                   'clone_frac_of_8TBps_read_plus_write': round(2 * nbytes / (1e-3 * med['clone']) / HBM_PEAK, 4),
                   'aten_over_area': round(med['aten'] / med['area'], 2)}
            area(caps[0], OUT_HW)
            res['kernel'] = k.lib.eve_last_kernel().decode()
            print(json.dumps(res), flush=True)
            rows.append(res)
            del caps, routes
            torch.cuda.empty_cache()
    lines = ['| size | N | MB in | area us | of 8 TB/s | clone us | (r+w) of 8 TB/s | ATen us | ATen / area |', '|---|---|---|---|---|---|---|---|---|']
    for r in rows:
        lines.append('| %s | %d | %.1f | %.2f | %.1f %% | %.2f | %.1f %% | %.2f | %.1fx |' % (
            r['size'], r['N'], r['bytes'] / 1e6, r['area_us'], 100 * r['area_frac_of_8TBps'], r['clone_us'],
            100 * r['clone_frac_of_8TBps_read_plus_write'], r['aten_us'], r['aten_over_area']))
    table = '\n'.join(lines)
    print(table, flush=True)
    if args.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(args.markdown)), exist_ok=True)
        with open(args.markdown, 'w') as f:
            f.write(table + '\n')


if __name__ == '__main__':
    main()
