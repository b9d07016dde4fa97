#!/usr/bin/env python
"""Time the stem's data-gradient kernel (eve_stem_dgrad) at training batch sizes against its HBM roof, and the EyeNet backward
with and without patch gradients.

    python tools/bench_stem_dgrad.py [N]        (N images per launch, default 1 920 = configs[1]'s 2 x 32 x 30 eye patches)

Roof: bytes of dconv read once (N x H/2 x W/2 x 64 elements) + float32 dx written once (N x 3 x H x W), at 8 TB/s."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import eve_amd  # noqa: E402
from eve_amd.kernels import default_kernels  # noqa: E402
from oracle import detweights  # noqa: E402

HBM = 8.0e12
N = next((int(a) for a in sys.argv[1:] if a.isdigit()), 1920)
k = default_kernels()


def timeit(fn, reps=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def kernel(dtype, size):
    w = torch.randn((64, 3, 7, 7), device='cuda') * 0.05
    wp = k.stem_dgrad_pack(w, dtype)
    dconv = torch.randn((N, size // 2, size // 2, 64), device='cuda').to(dtype)
    dx = torch.empty((N, 3, size, size), device='cuda')
    ms = timeit(lambda: k.stem_dgrad(dconv, wp, 3, out=dx))
    nbytes = dconv.numel() * dconv.element_size() + dx.numel() * 4
    floor = nbytes / HBM * 1e3
    print('stem_dgrad %-14s %3d^2 N=%d: %.3f ms, %.2f TB/s = %.0f %% of 8 TB/s (floor %.3f ms)' % (
        str(dtype).split('.')[1], size, N, ms, nbytes / ms / 1e9, 100.0 * floor / ms, floor), flush=True)


def backward(dtype, size, B, T):
    cfg = eve_amd.reset_standalone_config()
    net = eve_amd.EyeNet()
    net.compute_dtype = dtype
    detweights.fill_module(net, seed=0)
    net.cuda()
    batch = {kk: v.cuda() for kk, v in detweights.eyenet_batch(B, T, size=size, seed=0).items()}
    res = {}
    for want in (False, True):
        for side in ('left', 'right'):
            batch[side + '_eye_patch'].requires_grad_(want)

        def step():
            net.zero_grad(set_to_none=True)
            out = net.forward_sequence(batch)
            (out['left_g_initial'].sum() + out['right_pupil_size'].sum()).backward()
        res[want] = timeit(step, reps=3, warm=2)
    print('EyeNet %s %d^2 B=%d T=%d forward + backward: %.2f ms, with patch gradients %.2f ms (+%.2f ms)' % (
        str(dtype).split('.')[1], size, B, T, res[False], res[True], res[True] - res[False]), flush=True)


if __name__ == '__main__':
    kernel(torch.bfloat16, 128)
    kernel(torch.float16, 128)
    kernel(torch.float16, 256)
    kernel(torch.float32, 128)
    if '--kernel-only' not in sys.argv:
        backward(torch.bfloat16, 128, N // 60, 30)
        backward(torch.float16, 256, N // 60, 30)
