#!/usr/bin/env python
"""Device time of the tracking overlay's one launch (eve_overlay_render, csrc/overlay.hip) per input and output format, next to its
yardstick, both interleaved round by round in one process:

    overlay   HipKernels.overlay_render on N frames: reads the capture once, writes the annotated frame once
    copy      a torch device-to-device copy of the SAME number of bytes (the capture's plus the result's, half of them read and half
              written): what moving those bytes costs with no arithmetic at all

    python tools/bench_overlay.py [--size 1920x1080] [--frames 64] [--formats nv12 rgb ...] [--out-formats nv12 rgb ...]
                                  [--layers rich plain] [--iters 20] [--rounds 5]

--layers rich draws the default look: two markers (radii 10 / 14), a 72 x 128 heat map and the 128 x 256 eyes inset; plain converts
only.  One JSON line per (format, out_format, layers): the median, minimum and maximum over the rounds of the device time per call
(events around `iters` calls), the copy's, and copy / overlay (1.0: the launch moves its bytes as fast as a copy does).  Both routes
rotate over enough separately allocated captures to exceed the 256 MiB Infinity Cache, so the reads come from HBM."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from eve_amd.data import OverlaySpec  # noqa: E402
from eve_amd.kernels import OVERLAY_IN_FORMATS, OVERLAY_OUT_FORMATS, default_kernels, overlay_out_shape  # noqa: E402

ROTATE_BYTES = 512 << 20


def device_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(i)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def in_shape(fmt, N, IH, IW):
    return {'rgb': (N, IH, IW, 3), 'bgr': (N, IH, IW, 3), 'rgba': (N, IH, IW, 4), 'bgra': (N, IH, IW, 4), 'nv12': (N, IH * 3 // 2, IW),
            'i420': (N, IH * 3 // 2, IW), 'yuyv': (N, IH, IW, 2)}[fmt]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', default='1920x1080')
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--formats', nargs='+', default=sorted(OVERLAY_IN_FORMATS), choices=sorted(OVERLAY_IN_FORMATS))
    ap.add_argument('--out-formats', nargs='+', default=sorted(OVERLAY_OUT_FORMATS), choices=sorted(OVERLAY_OUT_FORMATS))
    ap.add_argument('--layers', nargs='+', default=['rich', 'plain'], choices=('rich', 'plain'))
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_overlay: no GPU (a time is only measured on one)')
    k = default_kernels()
    IW, IH = (int(v) for v in args.size.lower().split('x'))
    N = args.frames
    spec = OverlaySpec(heat=True)
    torch.manual_seed(N + IW)
    g = torch.Generator().manual_seed(N + IW)
    centres = (torch.rand((N, 2, 2), generator=g) * torch.tensor([IW, IH])).cuda()
    table = torch.tensor(spec.marker_table(), dtype=torch.int32).cuda()
    yy, xx = torch.meshgrid(torch.arange(72.0), torch.arange(128.0), indexing='ij')
    c = centres[:, 1].cpu() * torch.tensor([128.0 / IW, 72.0 / IH])
    heat = torch.exp(-((xx[None] - c[:, 0, None, None]) ** 2 + (yy[None] - c[:, 1, None, None]) ** 2) / 18.0).cuda().contiguous()
    inset = torch.randint(0, 256, (N, 128, 256, 3), dtype=torch.uint8, device='cuda')
    rich = dict(centres=centres, marker_table=table, heat=heat, heat_color=spec.heat_color, amax=spec.heat_amax, inset=inset,
                inset_xy=(IW - 256, IH - 128), zoom=1, mirror=True)
    for fmt in args.formats:
        for out_fmt in args.out_formats:
            shape, oshape = in_shape(fmt, N, IH, IW), overlay_out_shape(out_fmt, N, IH, IW)
            nin, nout = int(torch.tensor(shape).prod()), int(torch.tensor(oshape).prod())
            copies = max(2, min(64, -(-ROTATE_BYTES // nin)))
            caps = [torch.randint(0, 256, shape, dtype=torch.uint8, device='cuda') for _ in range(2)]
            caps += [caps[i % 2].clone() for i in range(copies - 2)]
            out = torch.empty(oshape, dtype=torch.uint8, device='cuda')
            half = (nin + nout) // 2                           # a copy that reads and writes nin + nout bytes in all
            srcs = [torch.randint(0, 256, (half,), dtype=torch.uint8, device='cuda') for _ in range(2)]
            srcs += [srcs[i % 2].clone() for i in range(max(2, -(-ROTATE_BYTES // half)) - 2)]
            dst = torch.empty((half,), dtype=torch.uint8, device='cuda')
            for layers in args.layers:
                kw = rich if layers == 'rich' else {}
                routes = {'overlay': lambda i: k.overlay_render(caps[i % copies], fmt, out_fmt, out=out, **kw),
                          'copy': lambda i: dst.copy_(srcs[i % len(srcs)])}
                for fn in routes.values():                     # warm up: code objects
                    for i in range(3):
                        fn(i)
                torch.cuda.synchronize()
                times = {name: [] for name in routes}
                for _ in range(args.rounds):
                    for name, fn in routes.items():
                        times[name].append(device_ms(fn, args.iters))
                res = {'size': args.size, 'N': N, 'format': fmt, 'out_format': out_fmt, 'layers': layers, 'bytes_in': nin, 'bytes_out': nout}
                for name, t in times.items():
                    res[name + '_us'] = round(1e3 * sorted(t)[len(t) // 2], 2)
                    res[name + '_us_min_max'] = [round(1e3 * min(t), 2), round(1e3 * max(t), 2)]
                res['copy_over_overlay'] = round(res['copy_us'] / res['overlay_us'], 3)
                res['overlay_TBps'] = round((nin + nout) / (1e-6 * res['overlay_us']) / 1e12, 3)
                k.overlay_render(caps[0], fmt, out_fmt, out=out, **kw)
                res['kernel'] = k.lib.eve_last_kernel().decode()
                print(json.dumps(res), flush=True)
            del caps, srcs, out, dst
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
