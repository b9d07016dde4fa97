"""The contract of eve_screen_u8_area_to_nchw (include/eve_hip.h) in numpy with int64 sums, two independent restatements of it,
and a stand-in `screen_u8_area_to_nchw` for the torch-CPU FakeKernels.

For a frame v[IH][IW][C] (uint8) and a target OH x OW, OH <= IH, OW <= IW:
    wy[oy][iy] = |[iy*OH, (iy+1)*OH) n [oy*IH, (oy+1)*IH)|        wx[ox][ix] the same from IW, OW
    S[c][oy][ox] = sum wy * wx * v[iy][ix][c]                     (an integer <= 255 * IH * IW < 2^32)
    y[c][oy][ox] = float32(float64(S) / float64(IH * IW)) * float32(1 / 255)
Channels beyond the third are ignored and the channel order is kept.  Nothing here is a reproduction of the reference's
screen.128x72.mp4 (ffmpeg's bicubic scaler, then lossy coding); it is what a live capture gets instead."""
import numpy as np
import torch

MAX_PIXELS = 16843009          # 255 * IH * IW <= 2^32 - 1


def axis_weights(I, O):
    """int64 [O, I]: the overlap of source pixel i's footprint [i*O, (i+1)*O) with output pixel o's [o*I, (o+1)*I)."""
    i = np.arange(I, dtype=np.int64)[None, :]
    o = np.arange(O, dtype=np.int64)[:, None]
    return np.maximum(np.minimum((i + 1) * O, (o + 1) * I) - np.maximum(i * O, o * I), 0)


def check_shapes(shape, out_hw):
    N, IH, IW, C = shape
    OH, OW = int(out_hw[0]), int(out_hw[1])
    if C not in (3, 4):
        raise ValueError('screen frames have 3 or 4 channels, got %d' % C)
    if not (0 < OH <= IH and 0 < OW <= IW):
        raise ValueError('upscaling is not supported: %dx%d -> %dx%d' % (IH, IW, OH, OW))
    if IH * IW > MAX_PIXELS:
        raise ValueError('frame too large: %d x %d > %d pixels' % (IH, IW, MAX_PIXELS))
    return N, IH, IW, C, OH, OW


def area_sums(frames, out_hw):
    """uint8 [N, IH, IW, C] -> int64 S [N, 3, OH, OW], summed over each output pixel's own source rows and columns only."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8
    N, IH, IW, C, OH, OW = check_shapes(frames.shape, out_hw)
    wy, wx = axis_weights(IH, OH), axis_weights(IW, OW)
    cols = np.zeros((N, OH, IW, 3), dtype=np.int64)
    for oy in range(OH):
        iy0, iy1 = oy * IH // OH, ((oy + 1) * IH + OH - 1) // OH
        assert wy[oy, :iy0].sum() == 0 and wy[oy, iy1:].sum() == 0
        cols[:, oy] = np.tensordot(wy[oy, iy0:iy1], frames[:, iy0:iy1, :, :3].astype(np.int64), axes=(0, 1))
    S = np.zeros((N, 3, OH, OW), dtype=np.int64)
    for ox in range(OW):
        ix0, ix1 = ox * IW // OW, ((ox + 1) * IW + OW - 1) // OW
        assert wx[ox, :ix0].sum() == 0 and wx[ox, ix1:].sum() == 0
        S[:, :, :, ox] = np.tensordot(cols[:, :, ix0:ix1], wx[ox, ix0:ix1], axes=(2, 0)).transpose(0, 2, 1)
    return S


def finish(S, IH, IW):
    """The two float steps of the contract: one float64 division rounded to float32, one float32 multiply."""
    q = (S.astype(np.float64) / np.float64(IH * IW)).astype(np.float32)
    return q * np.float32(1.0 / 255.0)


def area_resize(frames, out_hw):
    """THE CONTRACT: uint8 [N, IH, IW, C] -> float32 [N, 3, OH, OW]."""
    frames = np.asarray(frames)
    return finish(area_sums(frames, out_hw), frames.shape[1], frames.shape[2])


def area_sums_by_replication(frames, out_hw):
    """Restatement 1, any ratio: every source pixel repeated OH times down and OW times across is an (IH*OH) x (IW*OW) image in
    which each output pixel is an exact IH x IW block; its block sums are S.  No weight appears."""
    frames = np.asarray(frames)
    N, IH, IW, C, OH, OW = check_shapes(frames.shape, out_hw)
    big = np.repeat(np.repeat(frames[..., :3].astype(np.int64), OH, axis=1), OW, axis=2)     # [N, IH*OH, IW*OW, 3]
    return big.reshape(N, OH, IH, OW, IW, 3).sum(axis=(2, 4)).transpose(0, 3, 1, 2)


def area_resize_avg_pool(frames, out_hw):
    """Restatement 2, integer ratios only: F.avg_pool2d in float64 (the plain box mean), then the same two float steps."""
    frames = np.asarray(frames)
    N, IH, IW, C, OH, OW = check_shapes(frames.shape, out_hw)
    assert IH % OH == 0 and IW % OW == 0
    x = torch.from_numpy(frames[..., :3].copy()).permute(0, 3, 1, 2).double()
    mean = torch.nn.functional.avg_pool2d(x, (IH // OH, IW // OW)).numpy()
    return mean.astype(np.float32) * np.float32(1.0 / 255.0)


def screen_u8_area_to_nchw(self, frames, out_hw):
    """Stand-in of HipKernels.screen_u8_area_to_nchw for the torch-CPU FakeKernels: attach it to an instance's class, e.g.
    `class Fakes(FakeKernels): screen_u8_area_to_nchw = screen_resize_ref.screen_u8_area_to_nchw`."""
    assert frames.dtype == torch.uint8 and frames.dim() == 4
    check_shapes(tuple(frames.shape), out_hw)                  # (before the data is touched)
    return torch.from_numpy(area_resize(frames.cpu().numpy(), out_hw))
