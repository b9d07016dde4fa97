#!/usr/bin/env python
"""Per-shape timing of the conv kernels on the EyeNet trunk shapes (GPU box): R back-to-back launches
between one HIP event pair, algorithmic TFLOP/s per shape and pass."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eve_amd.kernels import HipKernels  # noqa: E402

SHAPES = [  # name, IH, Cin, Cout, K, stride, pad
    ('stem7x7s2', 128, 8, 64, 7, 2, 3),
    ('l1_3x3', 32, 64, 64, 3, 1, 1),
    ('l2.0_3x3s2', 32, 64, 128, 3, 2, 1),
    ('l2.0_ds1x1s2', 32, 64, 128, 1, 2, 0),
    ('l2_3x3', 16, 128, 128, 3, 1, 1),
    ('l3.0_3x3s2', 16, 128, 256, 3, 2, 1),
    ('l3_3x3', 8, 256, 256, 3, 1, 1),
    ('l4.0_3x3s2', 8, 256, 512, 3, 2, 1),
    ('l4_3x3', 4, 512, 512, 3, 1, 1),
]


def timeit(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 1920
    dt = torch.bfloat16 if (len(sys.argv) < 3 or sys.argv[2] == 'bf16') else torch.float32
    reps = 10
    k = HipKernels()
    tot = {'fwd': 0.0, 'dgrad': 0.0, 'wgrad': 0.0}
    print('%-14s %9s %9s %9s   (ms | TFLOP/s)   N=%d %s' % ('shape', 'fwd', 'dgrad', 'wgrad', N, dt))
    for name, IH, Cin, Cout, K, s, p in SHAPES:
        x = torch.randn((N, IH, IH, Cin), device='cuda').to(dt)
        w = (torch.randn((Cout, K, K, Cin), device='cuda') * 0.05).to(dt)
        wt = w.permute(3, 1, 2, 0).contiguous()
        y = k.conv2d_fwd(x, w, None, s, p)
        dy = torch.randn_like(y)
        dw = torch.zeros((Cout, K, K, Cin), device='cuda')
        real_cin = 3 if name.startswith('stem') else Cin
        flops = 2.0 * y.shape[0] * y.shape[1] * y.shape[2] * Cout * K * K * real_cin
        t_f = timeit(lambda: k.conv2d_fwd(x, w, None, s, p), reps)
        t_d = timeit(lambda: k.conv2d_dgrad(dy, wt, (IH, IH), s, p), reps) if not name.startswith('stem') else 0.0
        t_w = timeit(lambda: k.conv2d_wgrad(x, dy, K, K, s, p, dw), reps)
        mult = {'l1_3x3': 4, 'l2_3x3': 3, 'l3_3x3': 3, 'l4_3x3': 3}.get(name, 1)
        tot['fwd'] += mult * t_f; tot['dgrad'] += mult * t_d; tot['wgrad'] += mult * t_w
        f = lambda t: '%6.3f|%4.0f' % (t, flops / t / 1e9) if t > 0 else '     -    '
        print('%-14s %s %s %s  x%d' % (name, f(t_f), f(t_d), f(t_w), mult))
    print('trunk totals per step (ms): fwd %.2f dgrad %.2f wgrad %.2f' % (tot['fwd'], tot['dgrad'], tot['wgrad']))


def wgrad_ab(args):
    """python tools/bench_conv.py wgrad-ab [N ...] [f16]: the 128-input-channel 3x3 weight gradients (layer 2 stride 1, layer 3's
    stride-2 convolution) on wgrad_tr_kernel (dispatch_override(wgrad_wg8=3)) and on the 128 x 384 eight-wave tile (wgrad_wg8=2), the
    latter with slab partials (the process's workspace) and with float atomics (no workspace).  Warm: 20 launches between one event
    pair; cold: one launch after a 1 GB fill has displaced the operands from L2 and the Infinity Cache.  min..max of 5 repeats, us."""
    dt = torch.float16 if 'f16' in args else torch.bfloat16
    Ns = [int(a) for a in args if a.isdigit()] or [1920, 480]
    k = HipKernels()
    flush = torch.empty(1 << 30, dtype=torch.uint8, device='cuda')
    variants = (('wgrad_tr_kernel', 3, True), ('tile128 slab', 2, True), ('tile128 atomic', 2, False))
    print('%-12s %5s %-16s %-34s %17s %17s' % ('shape', 'N', 'variant', 'kernel', 'warm us min..max', 'cold us min..max'))
    for N in Ns:
        for name, IH, Cin, Cout, K, s, p in [r for r in SHAPES if r[0] in ('l2_3x3', 'l3.0_3x3s2')]:
            x = torch.randn((N, IH, IH, Cin), device='cuda').to(dt)
            OH = (IH + 2 * p - K) // s + 1
            dy = torch.randn((N, OH, OH, Cout), device='cuda').to(dt)
            dw = torch.zeros((Cout, K, K, Cin), device='cuda')
            for label, mode, use_ws in variants:
                ws_bytes = k.WORKSPACE_BYTES
                with k.dispatch_override(wgrad_wg8=mode):
                    if not use_ws:
                        k.WORKSPACE_BYTES = 0
                    try:
                        fn = lambda: k.conv2d_wgrad(x, dy, K, K, s, p, dw)
                        warm = [timeit(fn, 20) * 1e3 for _ in range(5)]
                        used = k.lib.eve_last_kernel().decode()
                        cold = []
                        for _ in range(5):
                            flush.fill_(1)
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record(); fn(); e1.record()
                            torch.cuda.synchronize()
                            cold.append(e0.elapsed_time(e1) * 1e3)
                    finally:
                        k.WORKSPACE_BYTES = ws_bytes
                print('%-12s %5d %-16s %-34s %7.1f..%-7.1f  %7.1f..%-7.1f' % (name, N, label, used.replace('eve::', ''), min(warm), max(warm),
                                                                            min(cold), max(cold)), flush=True)


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == 'wgrad-ab':
        wgrad_ab(sys.argv[2:])
    else:
        main()
