"""Tensor-level launcher over the C ABI of libeve_hip.so.

`HipKernels` takes torch tensors (device memory owned by torch's allocator), checks layout/dtype,
and calls the `extern "C"` entry points of include/eve_hip.h with raw pointers, explicit shapes and
torch's current HIP stream.  PyTorch is plumbing here: allocation and stream only.

Activations are NHWC (`[N, H, W, C]` contiguous) in the compute dtype (float32, bfloat16 or float16).
"""
import ctypes

import torch

from . import _lib
from ._lib import ConvDesc

ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_SELU, ACT_TANH, ACT_SIGMOID = range(6)
EPI_ACCUMULATE = 0x100          # include/eve_hip.h EVE_EPI_ACCUMULATE: y += act(conv + bias)
DT_F32, DT_BF16, DT_F16 = 0, 1, 2
HALF_DTYPES = (torch.bfloat16, torch.float16)      # the two 16-bit instantiations of the MFMA kernels
SCAN_WIDTHS = (32, 64, 128)                        # bottleneck widths the clip-long conv-RNN scans are instantiated for (csrc/cell_scan_f32.hip)


def dt_code(dtype):
    if dtype == torch.float32:
        return DT_F32
    if dtype == torch.bfloat16:
        return DT_BF16
    if dtype == torch.float16:
        return DT_F16
    raise TypeError('eve_amd kernels support float32, bfloat16 and float16, got %s' % dtype)


# include/eve_hip.h EVE_PIX_* / EVE_YUV_*: the frame layouts and YUV matrices of eve_eye_warp_fmt_to_nchw / _to_stem
PIXEL_FORMATS = {'bgr': 0, 'bgra': 1, 'nv12': 2, 'i420': 3, 'yuyv': 4}
YUV_MATRICES = {'bt601': 0, 'bt709': 1, 'jfif': 2}


def pixel_format_shape(frames, format, lead=1, name='frames'):
    """The frame tensor of one pixel format checked -> (IH, IW, C): uint8 with `lead` leading dimensions, then [IH, IW, 3 | 4] for
    'bgr' (and 'rgb'), [IH*3/2, IW] for 'nv12' / 'i420' (IH and IW even), [IH, IW, 2] for 'yuyv' (IW even); C is the last
    dimension, 1 for the planar forms.  TypeError for a wrong dtype or shape, ValueError for odd sizes or an unknown format."""
    if format not in ('rgb', 'bgr', 'nv12', 'i420', 'yuyv'):
        raise ValueError('%s: the format must be rgb, bgr, nv12, i420 or yuyv, got %r' % (name, format))
    dims = {'rgb': 3, 'bgr': 3, 'yuyv': 3, 'nv12': 2, 'i420': 2}[format]
    last = {'rgb': (3, 4), 'bgr': (3, 4), 'yuyv': (2,)}.get(format)
    layout = {'rgb': '[IH, IW, 3 | 4]', 'bgr': '[IH, IW, 3 | 4]', 'yuyv': '[IH, IW, 2]', 'nv12': '[IH*3/2, IW]', 'i420': '[IH*3/2, IW]'}[format]
    if (not torch.is_tensor(frames) or frames.dtype != torch.uint8 or frames.dim() != lead + dims or
            (last is not None and frames.shape[-1] not in last)):
        raise TypeError('%s must be uint8 with %d leading dimension%s and %s (%s), got %s %s' % (
            name, lead, '' if lead == 1 else 's', layout, format, getattr(frames, 'dtype', type(frames)), tuple(getattr(frames, 'shape', ()))))
    if dims == 3:
        IH, IW, C = (int(v) for v in frames.shape[lead:])
        if format == 'yuyv' and IW % 2:
            raise ValueError('%s: yuyv frames need an even width (chroma pairs), got %d' % (name, IW))
        return IH, IW, C
    rows, IW = (int(v) for v in frames.shape[lead:])
    if rows % 3 or IW % 2:                     # (IH = two thirds of the rows is then even)
        raise ValueError('%s: %s frames are [IH*3/2, IW] with IH and IW even, got %d rows of %d' % (name, format, rows, IW))
    return rows // 3 * 2, IW, 1


# eve_screen_luminance: the rows of one workgroup's band (csrc/screen_luminance.hip LUM_BAND_ROWS; the tests place discs across it)
LUM_BAND_ROWS = 32
LUM_REC709 = (13933, 46871, 4732)         # Rec.709's luminance weights in 1 / 65536, summing to 65536


# include/eve_hip.h eve_overlay_render: the capture formats it reads (EVE_PIX_RGB / _RGBA are its own two codes) and writes
OVERLAY_IN_FORMATS = dict(PIXEL_FORMATS, rgb=5, rgba=6)
OVERLAY_OUT_FORMATS = {'rgb': 5, 'bgr': 0, 'nv12': 2, 'i420': 3}
OVERLAY_MAX_MARKERS = 8
OVERLAY_MAX_HEAT = 1024


def overlay_out_shape(out_format, N, IH, IW):
    return (N, IH, IW, 3) if out_format in ('rgb', 'bgr') else (N, IH * 3 // 2, IW)


def overlay_check(frames, format, out_format, matrix, centres=None, marker_valid=None, marker_table=None, sx=1.0, sy=1.0, heat=None,
                  heat_color=(255, 0, 0), amax=128, inset=None, inset_xy=(0, 0), zoom=1, mirror=False, frame_valid=None, out=None):
    """The argument checks of overlay_render, shared with the torch-CPU stand-in of the tests -> a dict of the C call's scalars.
    Every failure is a ValueError that names the argument."""
    import math
    if format not in OVERLAY_IN_FORMATS:
        raise ValueError('overlay_render: format must be one of %s, got %r' % (', '.join(sorted(OVERLAY_IN_FORMATS)), format))
    if out_format not in OVERLAY_OUT_FORMATS:
        raise ValueError('overlay_render: out_format must be rgb, bgr, nv12 or i420, got %r' % (out_format,))
    if matrix not in YUV_MATRICES:
        raise ValueError('overlay_render: matrix must be one of %s, got %r' % (', '.join(YUV_MATRICES), matrix))
    try:
        IH, IW, C = pixel_format_shape(frames, {'rgba': 'rgb', 'bgra': 'bgr'}.get(format, format), lead=1)
    except TypeError as e:
        raise ValueError('overlay_render: %s' % e)
    if format in ('rgba', 'bgra') and C != 4:
        raise ValueError('overlay_render: frames of format %s must have four channels, got %d' % (format, C))
    if not frames.is_contiguous():
        raise ValueError('overlay_render: frames must be contiguous')
    name = format + 'a' if format in ('rgb', 'bgr') and C == 4 else format
    N, dev = int(frames.shape[0]), frames.device
    if N < 1 or IH < 1 or IW < 1 or IH > 16384 or IW > 16384:
        raise ValueError('overlay_render: frames must hold at least one frame of at most 16384 x 16384, got %s' % (tuple(frames.shape),))
    if out_format in ('nv12', 'i420') and (IH % 2 or IW % 2):
        raise ValueError('overlay_render: out_format %s needs even IH and IW (2 x 2 chroma blocks), got %d x %d' % (out_format, IH, IW))

    def tensor(t, what, dtype, shape):
        if (not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev):
            raise ValueError('overlay_render: %s must be a contiguous %s tensor %s on the frames\' device, got %s %s' % (
                what, str(dtype).replace('torch.', ''), list(shape), getattr(t, 'dtype', type(t)), tuple(getattr(t, 'shape', ()))))

    M = 0
    if centres is not None or marker_table is not None:
        if centres is None or marker_table is None:
            raise ValueError('overlay_render: centres and marker_table come together')
        if not torch.is_tensor(marker_table) or marker_table.dim() != 2:
            raise ValueError('overlay_render: marker_table must be an int32 tensor [M, 4]')
        M = int(marker_table.shape[0])
        if M > OVERLAY_MAX_MARKERS:
            raise ValueError('overlay_render: marker_table holds %d markers, at most %d are drawn' % (M, OVERLAY_MAX_MARKERS))
        tensor(marker_table, 'marker_table', torch.int32, (M, 4))
        tensor(centres, 'centres', torch.float32, (N, M, 2))
        if marker_valid is not None:
            tensor(marker_valid, 'marker_valid', torch.uint8, (N, M))
        if not (math.isfinite(sx) and math.isfinite(sy)):
            raise ValueError('overlay_render: sx and sy must be finite, got %r, %r' % (sx, sy))
    elif marker_valid is not None:
        raise ValueError('overlay_render: marker_valid without centres')
    HH = HW = 0
    color = 0
    if heat is not None:
        if not torch.is_tensor(heat) or heat.dim() != 3:
            raise ValueError('overlay_render: heat must be a float32 tensor [N, HH, HW]')
        HH, HW = int(heat.shape[1]), int(heat.shape[2])
        if not (1 <= HH <= OVERLAY_MAX_HEAT and 1 <= HW <= OVERLAY_MAX_HEAT):
            raise ValueError('overlay_render: heat must be at most %d x %d, got %d x %d' % (OVERLAY_MAX_HEAT, OVERLAY_MAX_HEAT, HH, HW))
        tensor(heat, 'heat', torch.float32, (N, HH, HW))
        if not 0 <= int(amax) <= 255:
            raise ValueError('overlay_render: amax must be in 0..255, got %r' % (amax,))
        if len(heat_color) != 3 or not all(0 <= int(c) <= 255 for c in heat_color):
            raise ValueError('overlay_render: heat_color must be three values in 0..255, got %r' % (heat_color,))
        color = (int(heat_color[0]) << 16) | (int(heat_color[1]) << 8) | int(heat_color[2])
    ih = iw = 0
    ix0, iy0 = int(inset_xy[0]), int(inset_xy[1])
    if inset is not None:
        if not torch.is_tensor(inset) or inset.dim() != 4:
            raise ValueError('overlay_render: inset must be a uint8 tensor [N, h, w, 3]')
        ih, iw = int(inset.shape[1]), int(inset.shape[2])
        tensor(inset, 'inset', torch.uint8, (N, ih, iw, 3))
        if not 1 <= int(zoom) <= 4:
            raise ValueError('overlay_render: zoom must be in 1..4, got %r' % (zoom,))
        if ih < 1 or iw < 1 or ix0 < 0 or iy0 < 0 or ix0 + int(zoom) * iw > IW or iy0 + int(zoom) * ih > IH:
            raise ValueError('overlay_render: the inset rectangle (inset_xy %s, %d x %d at zoom %d) does not lie inside the %d x %d frame' % (
                (ix0, iy0), ih, iw, int(zoom), IH, IW))
    if frame_valid is not None:
        tensor(frame_valid, 'frame_valid', torch.uint8, (N,))
    if out is not None:
        tensor(out, 'out', torch.uint8, overlay_out_shape(out_format, N, IH, IW))
    return dict(in_code=OVERLAY_IN_FORMATS[name], out_code=OVERLAY_OUT_FORMATS[out_format], matrix=YUV_MATRICES[matrix], N=N, IH=IH, IW=IW,
                M=M, HH=HH, HW=HW, heat_rgb=color, amax=int(amax), ih=ih, iw=iw, ix0=ix0, iy0=iy0, zoom=int(zoom), mirror=int(bool(mirror)),
                in_name=name)


def vec_of(dtype):
    return 4 if dtype == torch.float32 else 8


def pad_channels(c, dtype):
    v = vec_of(dtype)
    return (c + v - 1) // v * v


def conv_out_size(i, k, stride, pad):
    return (i + 2 * pad - k) // stride + 1


class HipKernels(object):
    """One instance per process; loads the library lazily and fails loudly if it is absent."""

    name = 'hip'

    def __init__(self):
        self.lib = _lib.load()
        self.prof = None          # list of (tag, flops, start_event, end_event) while profiling
        self._workspaces = {}     # (device, stream) -> uint8 scratch tensor, allocated once and never replaced

    WORKSPACE_BYTES = int(__import__('os').environ.get('EVE_AMD_WORKSPACE_MB', '128')) << 20

    def workspace(self, device):
        """(pointer, bytes) of this process's device scratch for the library calls that take one (include/eve_hip.h: the
        split-K partial filters of the weight-gradient kernels -- 7 splits x 512 x 4608 floats = 66 MB for ResNet layer 4 --
        and the re-packed filters of the stride-2 data gradient).  Passed PER CALL; allocated once per device by torch (the
        library never allocates) and kept for the life of the process, so a pointer captured into a hipGraph stays valid.
        Launches on one stream use it one after the other; the scratch is keyed by (device, current stream), so work issued
        from a second stream (a warm-up side stream, another trainer) gets its own and cannot corrupt split-K partials."""
        if device.type != 'cuda' or self.WORKSPACE_BYTES <= 0:
            return None, 0
        index = device.index if device.index is not None else torch.cuda.current_device()
        stream = torch.cuda.current_stream(index)
        if torch.cuda.is_current_stream_capturing():
            # a capture stream stands for the stream the graph will replay on; launches of one graph are ordered by the
            # captured dependencies, so they share one scratch whatever stream object carried the capture
            key = (index, 'graph')
        else:
            key = (index, stream.cuda_stream)
        ws = self._workspaces.get(key)
        if ws is None:
            ws = self._workspaces[key] = torch.empty(self.WORKSPACE_BYTES, dtype=torch.uint8, device=device)
        return ctypes.c_void_p(ws.data_ptr()), ws.numel()

    def prepare_graph_workspace(self, device):
        """Allocate the scratch of captured launches BEFORE a capture begins: first touched inside one it would come out of the
        graph's private memory pool and keep that pool's segment alive after the graph is destroyed."""
        if device.type == 'cuda' and self.WORKSPACE_BYTES > 0:
            index = device.index if device.index is not None else torch.cuda.current_device()
            if (index, 'graph') not in self._workspaces:
                self._workspaces[(index, 'graph')] = torch.empty(self.WORKSPACE_BYTES, dtype=torch.uint8, device=device)

    # ------------------------------------------------------------------ kernel selection (eve_dispatch_config)
    def dispatch_config(self):
        c = _lib.DispatchConfig()
        self._ck(self.lib.eve_get_dispatch_config(ctypes.byref(c)))
        return c

    def default_dispatch_config(self):
        c = _lib.DispatchConfig()
        self._ck(self.lib.eve_get_default_dispatch_config(ctypes.byref(c)))
        return c

    def dispatch_override(self, **fields):
        """Context manager: force kernel-selection fields for the calls inside it (tests comparing two kernels on the same
        inputs, tuning sweeps); the previous table is restored on exit."""
        import contextlib

        @contextlib.contextmanager
        def ctx():
            old = self.dispatch_config()
            new = self.dispatch_config()
            for n, v in fields.items():
                assert hasattr(new, n), 'eve_dispatch_config has no field %r' % n
                setattr(new, n, int(v))
            self._ck(self.lib.eve_set_dispatch_config(ctypes.byref(new)))
            try:
                yield new
            finally:
                self._ck(self.lib.eve_set_dispatch_config(ctypes.byref(old)))
        return ctx()

    # ------------------------------------------------------------------ per-launch timing (bench roofline)
    def start_profile(self):
        """Record a HIP event pair around every conv launch on the stream it is launched on."""
        self.prof = []

    def stop_profile(self):
        """-> {tag: {'launches', 'ms', 'flops'}}; synchronises the device."""
        rec, self.prof = self.prof or [], None
        # an event pair with nothing between it still reads a few us..tens of us on this runtime: calibrate and
        # subtract, so the per-launch figure agrees with rocprofv3's kernel durations
        null = []
        for _ in range(32):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            e1.record()
            null.append((e0, e1))
        torch.cuda.synchronize()
        overhead = sorted(a.elapsed_time(b) for a, b in null)[len(null) // 2]
        out, by_kernel = {}, {}
        for tag, flops, nbytes, e0, e1, sym in rec:
            ms = max(e0.elapsed_time(e1) - overhead, 1e-4)
            for table, key in ((out, tag), (by_kernel, sym)):
                d = table.setdefault(key, {'launches': 0, 'ms': 0.0, 'flops': 0.0, 'bytes': 0.0})
                d['launches'] += 1
                d['ms'] += ms
                d['flops'] += flops
                d['bytes'] += nbytes
        out['_event_overhead_ms'] = overhead
        out['_by_kernel'] = by_kernel          # keyed by the kernel symbol the library reports (eve_last_kernel)
        return out

    def _timed(self, tag, flops, fn, tensors=()):
        """tensors: what the launch reads and writes once (its ALGORITHMIC bytes, for HBM-bound kernels)."""
        if self.prof is None:
            return fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        sym = self.lib.eve_last_kernel()
        nbytes = float(sum(t.numel() * t.element_size() for t in tensors if t is not None))
        self.prof.append((tag, flops, nbytes, e0, e1, sym.decode() if sym else ''))
        return r

    # ------------------------------------------------------------------ helpers
    @staticmethod
    def _p(t):
        if t is None:
            return None
        if not t.is_cuda:
            raise RuntimeError('eve_amd: tensor is not on the GPU (the hot path has no CPU fallback)')
        if not t.is_contiguous():
            raise RuntimeError('eve_amd: non-contiguous tensor handed to a kernel')
        return ctypes.c_void_p(t.data_ptr())

    @staticmethod
    def _stream():
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def _ck(self, status):
        if status != 0:
            _lib.check(status, self.lib)

    @staticmethod
    def _f32(t, what):
        if t is not None and t.dtype != torch.float32:
            raise TypeError('%s must be float32' % what)
        return t

    @staticmethod
    def _desc(dtype, N, IH, IW, Cin, Cout, KH, KW, stride, pad):
        d = ConvDesc()
        d.dtype = dt_code(dtype)
        d.N, d.IH, d.IW, d.Cin = N, IH, IW, Cin
        d.OH, d.OW, d.Cout = conv_out_size(IH, KH, stride, pad), conv_out_size(IW, KW, stride, pad), Cout
        d.KH, d.KW, d.stride, d.pad = KH, KW, stride, pad
        return d

    # ------------------------------------------------------------------ convolution
    def conv2d_fwd(self, x, w_ohwi, bias, stride, pad, epi_act=ACT_NONE, ss=None, pro_act=ACT_NONE, algo=None,
                   accumulate_into=None):
        """algo = (true Cout, true KH*KW*Cin) when channels are zero-padded (algorithmic FLOP count).
        accumulate_into: a contiguous [N, OH, OW, Cout] tensor the result is ADDED to in the kernel epilogue
        (EVE_EPI_ACCUMULATE; the block's `layers(x) + skip_layer(x)` without an add launch); returned."""
        N, IH, IW, Cin = x.shape
        Cout, KH, KW, Cin2 = w_ohwi.shape
        assert Cin2 == Cin and w_ohwi.dtype == x.dtype
        d = self._desc(x.dtype, N, IH, IW, Cin, Cout, KH, KW, stride, pad)
        if accumulate_into is not None:
            y = accumulate_into
            assert tuple(y.shape) == (N, d.OH, d.OW, Cout) and y.dtype == x.dtype and y.is_contiguous() and ss is None
            epi_act = epi_act | EPI_ACCUMULATE
        else:
            y = torch.empty((N, d.OH, d.OW, Cout), dtype=x.dtype, device=x.device)
        co, kk = algo or (Cout, KH * KW * Cin)
        self._timed('conv_fwd', 2.0 * N * d.OH * d.OW * co * kk, lambda: self._ck(self.lib.eve_conv2d_fwd(
            ctypes.byref(d), self._p(x), self._p(w_ohwi), self._p(self._f32(bias, 'bias')), epi_act,
            self._p(self._f32(ss, 'scale/shift')), pro_act, self._p(y), self._stream())),
            (x, w_ohwi, y) + ((y,) if accumulate_into is not None else ()))
        return y

    def conv2d_fwd_stats(self, x, w_ohwi, bias, stride, pad, epi_act=ACT_NONE, eps=1e-5, algo=None):
        """conv2d_fwd that also returns the InstanceNorm statistics (mean, rstd) [N, Cout, 2] of its output when the dispatched
        kernel can form them in its epilogue (the row-streaming 3x3 kernel walks whole images), else None: -> (y, mean_rstd | None)."""
        N, IH, IW, Cin = x.shape
        Cout, KH, KW, Cin2 = w_ohwi.shape
        assert Cin2 == Cin and w_ohwi.dtype == x.dtype
        d = self._desc(x.dtype, N, IH, IW, Cin, Cout, KH, KW, stride, pad)
        y = torch.empty((N, d.OH, d.OW, Cout), dtype=x.dtype, device=x.device)
        mr = torch.empty((N, Cout, 2), dtype=torch.float32, device=x.device)
        written = ctypes.c_int(0)
        co, kk = algo or (Cout, KH * KW * Cin)
        self._timed('conv_fwd', 2.0 * N * d.OH * d.OW * co * kk, lambda: self._ck(self.lib.eve_conv2d_fwd_stats(
            ctypes.byref(d), self._p(x), self._p(w_ohwi), self._p(self._f32(bias, 'bias')), epi_act, self._p(y), self._p(mr),
            float(eps), ctypes.byref(written), self._stream())), (x, w_ohwi, y))
        return y, (mr if written.value else None)

    def conv2d_dgrad(self, dy, w_ihwo, in_hw, stride, pad, algo=None, accumulate_into=None):
        """Data gradient; with accumulate_into (a contiguous [N, IH, IW, Cin] tensor) it is ADDED to that tensor in
        the kernel epilogue and the same tensor is returned."""
        N, OH, OW, Cout = dy.shape
        Cin, KH, KW, Cout2 = w_ihwo.shape
        assert Cout2 == Cout and w_ihwo.dtype == dy.dtype
        IH, IW = in_hw
        d = self._desc(dy.dtype, N, IH, IW, Cin, Cout, KH, KW, stride, pad)
        assert (d.OH, d.OW) == (OH, OW)
        co, kk = algo or (Cout, KH * KW * Cin)
        # (the stride-2 data gradient re-packs its filters into the scratch; dgrad_acc takes none)
        wsp, wsn = self.workspace(dy.device) if (stride == 2 and dy.dtype in HALF_DTYPES) else (None, 0)
        if accumulate_into is not None:
            dx = accumulate_into
            assert tuple(dx.shape) == (N, IH, IW, Cin) and dx.dtype == dy.dtype and dx.is_contiguous()
            fn = lambda: self.lib.eve_conv2d_dgrad_acc(ctypes.byref(d), self._p(dy), self._p(w_ihwo), self._p(dx), self._stream())
        else:
            dx = torch.empty((N, IH, IW, Cin), dtype=dy.dtype, device=dy.device)
            fn = lambda: self.lib.eve_conv2d_dgrad(ctypes.byref(d), self._p(dy), self._p(w_ihwo), self._p(dx), wsp, wsn, self._stream())
        self._timed('conv_dgrad', 2.0 * N * OH * OW * co * kk, lambda: self._ck(fn()), (dy, w_ihwo, dx))
        return dx

    def conv2d_wgrad(self, x, dy, KH, KW, stride, pad, dw_ohwi, ss=None, pro_act=ACT_NONE, algo=None, db=None):
        """Accumulates into dw_ohwi (float32 [Cout, KH, KW, Cin]) and, when given, the column sums of dy into db
        (float32 [Cout]) in the same pass."""
        N, IH, IW, Cin = x.shape
        Cout = dy.shape[3]
        assert dw_ohwi.shape == (Cout, KH, KW, Cin) and dw_ohwi.dtype == torch.float32
        d = self._desc(x.dtype, N, IH, IW, Cin, Cout, KH, KW, stride, pad)
        assert tuple(dy.shape) == (N, d.OH, d.OW, Cout) and dy.dtype == x.dtype
        co, kk = algo or (Cout, KH * KW * Cin)
        wsp, wsn = self.workspace(x.device) if x.dtype in HALF_DTYPES else (None, 0)
        if db is not None:
            assert ss is None and db.shape == (Cout,) and db.dtype == torch.float32 and db.is_contiguous()
            self._timed('conv_wgrad', 2.0 * N * d.OH * d.OW * co * kk, lambda: self._ck(self.lib.eve_conv2d_wgrad_bias(
                ctypes.byref(d), self._p(x), self._p(dy), self._p(dw_ohwi), self._p(db), wsp, wsn, self._stream())), (x, dy, dw_ohwi))
            return dw_ohwi
        self._timed('conv_wgrad', 2.0 * N * d.OH * d.OW * co * kk, lambda: self._ck(self.lib.eve_conv2d_wgrad(
            ctypes.byref(d), self._p(x), self._p(dy), self._p(self._f32(ss, 'scale/shift')), pro_act,
            self._p(dw_ohwi), wsp, wsn, self._stream())), (x, dy, dw_ohwi))
        return dw_ohwi

    def stem_pack_input(self, src_nchw, out=None, dtype=torch.bfloat16):
        N, C, H, W = src_nchw.shape
        src = self._f32(src_nchw.contiguous(), 'src')
        dst = out if out is not None else torch.empty((N, H + 6, W + 8, 4), dtype=dtype, device=src.device)
        assert tuple(dst.shape) == (N, H + 6, W + 8, 4) and dst.dtype in HALF_DTYPES
        self._ck(self.lib.eve_stem_pack_input(dt_code(dst.dtype), N, C, H, W, self._p(src), self._p(dst), self._stream()))
        return dst

    def stem7x7s2_fwd(self, x_padded, w_ohwi8):
        N, Hp, Wp, four = x_padded.shape
        IH, IW = Hp - 6, Wp - 8
        assert four == 4 and tuple(w_ohwi8.shape) == (64, 7, 7, 8) and w_ohwi8.dtype == x_padded.dtype and x_padded.dtype in HALF_DTYPES
        y = torch.empty((N, IH // 2, IW // 2, 64), dtype=x_padded.dtype, device=x_padded.device)
        flops = 2.0 * N * (IH // 2) * (IW // 2) * 64 * 147
        self._timed('conv_fwd', flops, lambda: self._ck(self.lib.eve_stem7x7s2_fwd(
            dt_code(x_padded.dtype), N, IH, IW, self._p(x_padded), self._p(w_ohwi8), self._p(y), self._stream())))
        return y

    def stem_fwd_fused(self, x_padded, w_ohwi8, eps=1e-5):
        N, Hp, Wp, four = x_padded.shape
        IH, IW = Hp - 6, Wp - 8
        assert four == 4 and tuple(w_ohwi8.shape) == (64, 7, 7, 8) and w_ohwi8.dtype == x_padded.dtype and x_padded.dtype in HALF_DTYPES
        y = torch.empty((N, IH // 4, IW // 4, 64), dtype=x_padded.dtype, device=x_padded.device)
        idx = torch.empty((N, IH // 4, IW // 4, 64), dtype=torch.uint8, device=x_padded.device)
        mr = torch.empty((N, 64, 2), dtype=torch.float32, device=x_padded.device)
        flops = 2.0 * N * (IH // 2) * (IW // 2) * 64 * 147
        self._timed('conv_fwd', flops, lambda: self._ck(self.lib.eve_stem_fwd_fused(
            dt_code(x_padded.dtype), N, IH, IW, self._p(x_padded), self._p(w_ohwi8), eps, self._p(y), self._p(idx), self._p(mr),
            self._stream())))
        return y, idx, mr

    def stem_wgrad(self, x_padded, dconv, dw):
        """dw [64, 7, 8, 4] float32 += weight gradient of conv1 from the packed patches (filter column 7 / channel 3 unused)."""
        N, Hp, Wp, _ = x_padded.shape
        IH, IW = Hp - 6, Wp - 8
        assert tuple(dw.shape) == (64, 7, 8, 4) and dw.dtype == torch.float32 and dw.is_contiguous()
        assert tuple(dconv.shape) == (N, IH // 2, IW // 2, 64) and dconv.dtype == x_padded.dtype
        flops = 2.0 * N * (IH // 2) * (IW // 2) * 64 * 147
        self._timed('conv_wgrad', flops, lambda: self._ck(self.lib.eve_stem_wgrad(
            dt_code(x_padded.dtype), N, IH, IW, self._p(x_padded), self._p(dconv), self._p(dw), self._stream())))

    def stem_bwd_dx(self, x_padded, w_ohwi8, mr, dy_pool, y_pool, idx, dy_pool2=None):
        N, Hp, Wp, _ = x_padded.shape
        IH, IW = Hp - 6, Wp - 8
        dx = torch.empty((N, IH // 2, IW // 2, 64), dtype=x_padded.dtype, device=x_padded.device)
        assert dy_pool.dtype == x_padded.dtype and dy_pool.is_contiguous() and dy_pool.shape == y_pool.shape == idx.shape
        # (the convolution is RE-computed here: no algorithmic FLOPs are credited)
        self._timed('stem_bwd', 0.0, lambda: self._ck(self.lib.eve_stem_bwd_dx(
            dt_code(x_padded.dtype), N, IH, IW, self._p(x_padded), self._p(w_ohwi8), self._p(self._f32(mr, 'mean_rstd')), self._p(dy_pool),
            self._p(dy_pool2), self._p(y_pool), self._p(idx), self._p(dx), self._stream())))
        return dx

    def stem_dgrad_pack(self, w_oihw, dtype):
        """conv1's float OIHW weight [64, C, 7, 7] -> the filter operand of stem_dgrad in `dtype` (1024 x 16 elements)."""
        w = self._f32(w_oihw.detach().contiguous(), 'w_oihw')
        assert w.dim() == 4 and w.shape[0] == 64 and 1 <= w.shape[1] <= 4 and tuple(w.shape[2:]) == (7, 7)
        out = torch.empty((1024, 16), dtype=dtype, device=w.device)
        self._ck(self.lib.eve_stem_dgrad_pack(dt_code(dtype), w.shape[1], self._p(w), self._p(out), self._stream()))
        return out

    def stem_dgrad(self, dconv, w_packed, C, out=None):
        """d(conv1 out) [N, IH/2, IW/2, 64] NHWC (float32 / bf16 / f16) -> the patch gradient [N, C, IH, IW] float32 NCHW
        (include/eve_hip.h eve_stem_dgrad); w_packed from stem_dgrad_pack in dconv's dtype."""
        N, OH, OW, co = dconv.shape
        assert co == 64 and dconv.is_contiguous() and w_packed.dtype == dconv.dtype and tuple(w_packed.shape) == (1024, 16)
        dx = out if out is not None else torch.empty((N, C, 2 * OH, 2 * OW), dtype=torch.float32, device=dconv.device)
        assert tuple(dx.shape) == (N, C, 2 * OH, 2 * OW) and dx.dtype == torch.float32
        flops = 2.0 * N * OH * OW * 64 * 49 * C
        self._timed('stem_dgrad', flops, lambda: self._ck(self.lib.eve_stem_dgrad(
            dt_code(dconv.dtype), N, 2 * OH, 2 * OW, C, self._p(dconv), self._p(w_packed), self._p(dx), self._stream())),
            (dconv, dx))
        return dx

    def stem_bwd_wgrad(self, x_padded, w_ohwi8, mr, dy_pool, y_pool, idx, dw, dy_pool2=None):
        """dw [64, 7, 8, 4] float32 += the stem's weight gradient straight from d(pooled output): backward of the fused stem and
        its weight gradient in one launch, d(conv1 out) never written (include/eve_hip.h eve_stem_bwd_wgrad)."""
        N, Hp, Wp, _ = x_padded.shape
        IH, IW = Hp - 6, Wp - 8
        assert tuple(dw.shape) == (64, 7, 8, 4) and dw.dtype == torch.float32 and dw.is_contiguous()
        assert dy_pool.dtype == x_padded.dtype and dy_pool.is_contiguous() and dy_pool.shape == y_pool.shape == idx.shape
        # the weight gradient's FLOPs are algorithmic; the recomputed convolution is not credited
        flops = 2.0 * N * (IH // 2) * (IW // 2) * 64 * 147
        # the call's scratch (the masked, summed gradient + the per-plane constants: 252 MB at N = 1 920), from torch's allocator
        # like any activation: stream-ordered, and part of the graph's pool under capture
        nbytes = int(self.lib.eve_stem_bwd_wgrad_workspace(dt_code(x_padded.dtype), N, IH))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=x_padded.device)
        self._timed('conv_wgrad', flops, lambda: self._ck(self.lib.eve_stem_bwd_wgrad(
            dt_code(x_padded.dtype), N, IH, IW, self._p(x_padded), self._p(w_ohwi8), self._p(self._f32(mr, 'mean_rstd')), self._p(dy_pool),
            self._p(dy_pool2), self._p(y_pool), self._p(idx), self._p(dw), self._p(ws), nbytes, self._stream())),
            (x_padded, dy_pool, dy_pool2, y_pool, idx))

    # ------------------------------------------------------------------ chains of small float32 linear layers (the tail)
    def linear_wgrad_batch(self, problems):
        """All weight / bias gradients of the tail in one launch.  problems: dicts dY [M,N], Y (or None) + act, X [M,K1], X2 (or
        None), dW [N,K] (accumulated), db [N] or None."""
        n = len(problems)
        assert 0 < n <= _lib.WGRAD_BATCH_MAX
        arr = (_lib.WgradProblem * n)()
        for q, pr in zip(arr, problems):
            dY, X, dW = pr['dY'], pr['X'], pr['dW']
            for t in (dY, X, dW, pr.get('Y'), pr.get('X2'), pr.get('db')):
                assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda)
            q.dY, q.X, q.dW = dY.data_ptr(), X.data_ptr(), dW.data_ptr()
            q.Y = pr['Y'].data_ptr() if pr.get('Y') is not None else None
            q.X2 = pr['X2'].data_ptr() if pr.get('X2') is not None else None
            q.db = pr['db'].data_ptr() if pr.get('db') is not None else None
            q.M, q.N, q.K = dY.shape[0], dW.shape[0], dW.shape[1]
            q.K1, q.K2 = pr.get('K1', X.shape[1]), (pr['X2'].shape[1] if pr.get('X2') is not None else 0)
            q.act = pr.get('act', ACT_NONE)
            q.ldY = dY.shape[1] if dY.shape[1] != q.N else 0
            q.ldX = X.shape[1] if X.shape[1] != q.K1 else 0           # the leading K1 columns of a wider X
            q.ldW, q.x_shift_T, q.reserved = 0, int(pr.get('x_shift_T', 0)), 0
            assert dY.shape[1] >= q.N and q.K1 + q.K2 <= q.K and X.shape[0] == q.M and X.shape[1] >= q.K1
            assert not q.x_shift_T or (q.K2 == 0 and q.K1 == q.K and q.M % q.x_shift_T == 0)    # (the kernel reads column k of X for every k < K)
            assert pr.get('Y') is None or pr['Y'].shape == dY.shape
        self._timed('tail', 0.0, lambda: self._ck(self.lib.eve_linear_wgrad_batch(arr, n, self._stream())))

    def stem_fused_wgrad_enabled(self):
        return bool(self.dispatch_config().stem_fused_wgrad)

    # ------------------------------------------------------------------ decoded uint8 frames (input pipeline)
    def frames_u8_to_nchw(self, frames, scale, shift=None):
        """uint8 [N,H,W,C] -> float32 [N,C,H,W] = frames * scale (+ shift)."""
        N, H, W, C = frames.shape
        assert frames.dtype == torch.uint8
        out = torch.empty((N, C, H, W), dtype=torch.float32, device=frames.device)
        self._ck(self.lib.eve_frames_u8_to_nchw(N, H, W, C, self._p(frames), float(scale), float(shift or 0.0),
                                                0 if shift is None else 1, self._p(out), self._stream()))
        return out

    def screen_u8_area_to_nchw(self, frames, out_hw):
        """uint8 [N,IH,IW,C] (C 3 or 4, a fourth channel ignored, channel order kept) -> float32 [N,3,OH,OW] in [0, 1]: the exact
        area average over each output pixel's footprint (include/eve_hip.h eve_screen_u8_area_to_nchw).  out_hw = (OH, OW), no
        larger than the frames; the library refuses upscaling and frames beyond 16 843 009 pixels."""
        N, IH, IW, C = frames.shape
        assert frames.dtype == torch.uint8
        OH, OW = int(out_hw[0]), int(out_hw[1])
        out = torch.empty((N, 3, OH, OW), dtype=torch.float32, device=frames.device)
        self._ck(self.lib.eve_screen_u8_area_to_nchw(N, IH, IW, C, self._p(frames), OH, OW, self._p(out), self._stream()))
        return out

    def screen_u8_area_bgr_to_nchw(self, frames, out_hw):
        """screen_u8_area_to_nchw for a BGR(A) capture: plane c of the result comes from source channel 2 - c, so it equals
        screen_u8_area_to_nchw on the channel-reversed capture bit for bit (include/eve_hip.h eve_screen_u8_area_bgr_to_nchw)."""
        N, IH, IW, C = frames.shape
        assert frames.dtype == torch.uint8
        OH, OW = int(out_hw[0]), int(out_hw[1])
        out = torch.empty((N, 3, OH, OW), dtype=torch.float32, device=frames.device)
        self._ck(self.lib.eve_screen_u8_area_bgr_to_nchw(N, IH, IW, C, self._p(frames), OH, OW, self._p(out), self._stream()))
        return out

    def screen_area_fmt_to_nchw(self, frames, out_hw, format, matrix='bt601'):
        """screen_u8_area_to_nchw for a capture as decoders and capture paths deliver it, uint8 and contiguous: format 'nv12' /
        'i420' [N,IH*3/2,IW], 'yuyv' [N,IH,IW,2] or 'bgr' [N,IH,IW,3|4]; matrix 'bt601' | 'bt709' | 'jfif' for the YUV formats.
        Every pixel is converted as it is read, by the integer matrix of include/eve_hip.h eve_eye_warp_fmt_to_nchw, and the
        converted values are averaged: the result is screen_u8_area_to_nchw's on the converted frame, bit for bit, and no RGB frame
        is made (include/eve_hip.h eve_screen_area_fmt_to_nchw)."""
        IH, IW, C = pixel_format_shape(frames, format, lead=1)
        if format == 'rgb':
            raise ValueError('screen_area_fmt_to_nchw takes bgr, nv12, i420 or yuyv; an RGB capture goes to screen_u8_area_to_nchw')
        if matrix not in YUV_MATRICES:
            raise ValueError('screen_area_fmt_to_nchw: matrix must be one of %s, got %r' % (', '.join(YUV_MATRICES), matrix))
        if not frames.is_contiguous():
            raise RuntimeError('eve_amd: non-contiguous tensor handed to a kernel')
        N, (OH, OW) = frames.shape[0], (int(out_hw[0]), int(out_hw[1]))
        out = torch.empty((N, 3, OH, OW), dtype=torch.float32, device=frames.device)
        code = PIXEL_FORMATS['bgra' if format == 'bgr' and C == 4 else format]
        self._ck(self.lib.eve_screen_area_fmt_to_nchw(code, YUV_MATRICES[matrix], N, IH, IW, self._p(frames), OH, OW, self._p(out),
                                                      self._stream()))
        return out

    def overlay_render(self, frames, format, out_format='nv12', matrix='bt601', centres=None, marker_valid=None, marker_table=None,
                       sx=1.0, sy=1.0, heat=None, heat_color=(255, 0, 0), amax=128, inset=None, inset_xy=(0, 0), zoom=1, mirror=False,
                       frame_valid=None, out=None):
        """The tracking overlay in one launch (include/eve_hip.h eve_overlay_render; tests/overlay_ref.py is the contract): frames
        uint8 [N, ...] of `format` ('rgb' | 'bgr' [N,IH,IW,3|4], 'rgba' | 'bgra', 'nv12' | 'i420' [N,IH*3/2,IW], 'yuyv' [N,IH,IW,2])
        -> uint8 [N,IH,IW,3] for out_format 'rgb' | 'bgr', [N,IH*3/2,IW] for 'nv12' | 'i420'.  Layers, each optional: heat float32
        [N,HH,HW] blended in heat_color up to alpha amax; inset uint8 [N,h,w,3] RGB replacing the zoom*h x zoom*w rectangle at
        inset_xy = (x0, y0); discs at centres float32 [N,M,2] (scaled by sx, sy to output pixels) where marker_valid uint8 [N,M] is
        not 0, by marker_table int32 [M,4] = (r_fill, r_outline, fill 0xRRGGBB, outline 0xRRGGBB).  frame_valid uint8 [N]: a 0
        gives the converted capture alone.  out: the buffer to write (a graph's output).  ValueError names a bad argument."""
        a = overlay_check(frames, format, out_format, matrix, centres, marker_valid, marker_table, sx, sy, heat, heat_color, amax, inset,
                          inset_xy, zoom, mirror, frame_valid, out)
        if out is None:
            out = torch.empty(overlay_out_shape(out_format, a['N'], a['IH'], a['IW']), dtype=torch.uint8, device=frames.device)
        self._ck(self.lib.eve_overlay_render(a['in_code'], a['out_code'], a['matrix'], a['N'], a['IH'], a['IW'], self._p(frames), self._p(out),
                                             a['M'], self._p(centres), self._p(marker_valid), self._p(marker_table), float(sx), float(sy),
                                             self._p(heat), a['HH'], a['HW'], a['heat_rgb'], a['amax'], self._p(inset), a['ih'], a['iw'],
                                             a['ix0'], a['iy0'], a['zoom'], a['mirror'], self._p(frame_valid), self._stream()))
        return out

    def frames_u8_to_stem(self, frames, scale, shift, out=None, dtype=torch.bfloat16):
        """uint8 [N,H,W,C<=4] -> the stem's packed 16-bit input [N,H+6,W+8,4]."""
        N, H, W, C = frames.shape
        assert frames.dtype == torch.uint8
        dst = out if out is not None else torch.empty((N, H + 6, W + 8, 4), dtype=dtype, device=frames.device)
        assert tuple(dst.shape) == (N, H + 6, W + 8, 4) and dst.dtype in HALF_DTYPES
        self._ck(self.lib.eve_frames_u8_to_stem(dt_code(dst.dtype), N, C, H, W, self._p(frames), float(scale), float(shift), self._p(dst), self._stream()))
        return dst

    @staticmethod
    def _eye_warp_args(frames, warps, out_hw):
        """The checks of the two eye_warp_u8_* calls -> (N, IH, IW, C, OH, OW)."""
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] not in (3, 4):
            raise TypeError('eye_warp: frames must be uint8 [N, IH, IW, 3 | 4], got %s %s' % (frames.dtype, tuple(frames.shape)))
        N, IH, IW, C = frames.shape
        if warps.dtype != torch.float32 or tuple(warps.shape) != (N, 3, 3):
            raise TypeError('eye_warp: warps must be float32 [%d, 3, 3], got %s %s' % (N, warps.dtype, tuple(warps.shape)))
        if not (frames.is_contiguous() and warps.is_contiguous()):
            raise RuntimeError('eve_amd: non-contiguous tensor handed to a kernel')
        if warps.device != frames.device:
            raise RuntimeError('eye_warp: frames and warps are on different devices')
        OH, OW = int(out_hw[0]), int(out_hw[1])
        return N, IH, IW, C, OH, OW

    def eye_warp_u8_to_nchw(self, frames, warps, out_hw):
        """Whole uint8 camera frames [N,IH,IW,C] (C 3 or 4, a fourth channel ignored, channel order kept) and one homography per
        frame, float32 [N,3,3] mapping a patch pixel to a camera pixel (cv2.warpPerspective's WARP_INVERSE_MAP matrix: inv(W) of
        the normalisation matrix W) -> the eye patches, float32 [N,3,OH,OW] in [-1, 1]: bilinear with 8 fractional bits, zero
        outside the frame, normalised as preprocess_frames normalises (include/eve_hip.h eve_eye_warp_u8_to_nchw)."""
        N, IH, IW, C, OH, OW = self._eye_warp_args(frames, warps, out_hw)
        out = torch.empty((N, 3, OH, OW), dtype=torch.float32, device=frames.device)
        self._ck(self.lib.eve_eye_warp_u8_to_nchw(N, IH, IW, C, self._p(frames), self._p(warps), OH, OW, self._p(out), self._stream()))
        return out

    def eye_warp_u8_to_stem(self, frames, warps, out_hw, out=None, dtype=torch.bfloat16):
        """The same patches straight into the stem's packed 16-bit input [N,OH+6,OW+8,4] (what frames_u8_to_stem writes from
        pre-cut patches): the pad ring and the fourth channel zero."""
        N, IH, IW, C, OH, OW = self._eye_warp_args(frames, warps, out_hw)
        dst = out if out is not None else torch.empty((N, OH + 6, OW + 8, 4), dtype=dtype, device=frames.device)
        if tuple(dst.shape) != (N, OH + 6, OW + 8, 4) or dst.dtype not in HALF_DTYPES:
            raise TypeError('eye_warp: out must be bf16 / f16 [%d, %d, %d, 4], got %s %s' % (N, OH + 6, OW + 8, dst.dtype, tuple(dst.shape)))
        self._ck(self.lib.eve_eye_warp_u8_to_stem(dt_code(dst.dtype), N, IH, IW, C, self._p(frames), self._p(warps), OH, OW, self._p(dst),
                                                  self._stream()))
        return dst

    def _eye_warp_lens_args(self, frames, warps, lens, out_hw):
        """_eye_warp_args plus the lens rows: float32 [N, 12], contiguous, on the frames' device."""
        args = self._eye_warp_args(frames, warps, out_hw)
        if not torch.is_tensor(lens) or lens.dtype != torch.float32 or tuple(lens.shape) != (args[0], 12):
            raise TypeError('eye_warp: lens must be float32 [%d, 12], got %s %s' % (args[0], getattr(lens, 'dtype', type(lens)),
                                                                                  tuple(getattr(lens, 'shape', ()))))
        if not lens.is_contiguous():
            raise RuntimeError('eve_amd: non-contiguous tensor handed to a kernel')
        if lens.device != frames.device:
            raise RuntimeError('eye_warp: frames and lens are on different devices')
        return args

    def eye_warp_lens_u8_to_nchw(self, frames, warps, lens, out_hw):
        """eye_warp_u8_to_nchw on RAW frames of a camera with lens distortion: `warps` point into the undistorted image, and lens,
        float32 [N,12] = (fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6) per frame (data.camera_lens; OpenCV's pinhole + radial /
        tangential / rational model), carries each coordinate to the raw frame before the taps are read.  A row with all eight
        coefficients zero gives eye_warp_u8_to_nchw's bits (include/eve_hip.h eve_eye_warp_lens_u8_to_nchw)."""
        N, IH, IW, C, OH, OW = self._eye_warp_lens_args(frames, warps, lens, out_hw)
        out = torch.empty((N, 3, OH, OW), dtype=torch.float32, device=frames.device)
        self._ck(self.lib.eve_eye_warp_lens_u8_to_nchw(N, IH, IW, C, self._p(frames), self._p(warps), self._p(lens), OH, OW, self._p(out),
                                                       self._stream()))
        return out

    def eye_warp_lens_u8_to_stem(self, frames, warps, lens, out_hw, out=None, dtype=torch.bfloat16):
        """The same patches straight into the stem's packed 16-bit input [N,OH+6,OW+8,4], as eye_warp_u8_to_stem lays it out."""
        N, IH, IW, C, OH, OW = self._eye_warp_lens_args(frames, warps, lens, out_hw)
        dst = out if out is not None else torch.empty((N, OH + 6, OW + 8, 4), dtype=dtype, device=frames.device)
        if tuple(dst.shape) != (N, OH + 6, OW + 8, 4) or dst.dtype not in HALF_DTYPES:
            raise TypeError('eye_warp: out must be bf16 / f16 [%d, %d, %d, 4], got %s %s' % (N, OH + 6, OW + 8, dst.dtype, tuple(dst.shape)))
        self._ck(self.lib.eve_eye_warp_lens_u8_to_stem(dt_code(dst.dtype), N, IH, IW, C, self._p(frames), self._p(warps), self._p(lens), OH, OW,
                                                       self._p(dst), self._stream()))
        return dst

    @staticmethod
    def _eye_warp_fmt_args(frames, warps, out_hw, format, matrix, lens):
        """The checks of the two eye_warp_fmt_* calls -> (format code, matrix code, N, IH, IW, OH, OW): the frame's shape per
        pixel_format_shape (TypeError for a wrong dtype or shape, ValueError for odd sizes or an unknown format or matrix)."""
        IH, IW, C = pixel_format_shape(frames, format, lead=1)
        N = frames.shape[0]
        if matrix not in YUV_MATRICES:
            raise ValueError('eye_warp: matrix must be one of %s, got %r' % (', '.join(YUV_MATRICES), matrix))
        if warps.dtype != torch.float32 or tuple(warps.shape) != (N, 3, 3):
            raise TypeError('eye_warp: warps must be float32 [%d, 3, 3], got %s %s' % (N, warps.dtype, tuple(warps.shape)))
        if lens is not None and (not torch.is_tensor(lens) or lens.dtype != torch.float32 or tuple(lens.shape) != (N, 12)):
            raise TypeError('eye_warp: lens must be float32 [%d, 12], got %s %s' % (N, getattr(lens, 'dtype', type(lens)),
                                                                                  tuple(getattr(lens, 'shape', ()))))
        if not (frames.is_contiguous() and warps.is_contiguous() and (lens is None or lens.is_contiguous())):
            raise RuntimeError('eve_amd: non-contiguous tensor handed to a kernel')
        if warps.device != frames.device or (lens is not None and lens.device != frames.device):
            raise RuntimeError('eye_warp: frames, warps and lens are on different devices')
        code = PIXEL_FORMATS['bgra' if format == 'bgr' and C == 4 else format]
        return code, YUV_MATRICES[matrix], N, IH, IW, int(out_hw[0]), int(out_hw[1])

    def eye_warp_fmt_to_nchw(self, frames, warps, out_hw, format, matrix='bt601', lens=None):
        """eye_warp_u8_to_nchw (lens=None) / eye_warp_lens_u8_to_nchw on frames as cameras and decoders deliver them, uint8 and
        contiguous: format 'bgr' [N,IH,IW,3|4], 'nv12' / 'i420' [N,IH*3/2,IW], 'yuyv' [N,IH,IW,2]; matrix 'bt601' | 'bt709' | 'jfif'
        for the YUV formats.  Only the taps read are converted, by the integer matrix of include/eve_hip.h
        eve_eye_warp_fmt_to_nchw: the result is the RGB call's on the converted frame, bit for bit."""
        fmt, mat, N, IH, IW, OH, OW = self._eye_warp_fmt_args(frames, warps, out_hw, format, matrix, lens)
        out = torch.empty((N, 3, OH, OW), dtype=torch.float32, device=frames.device)
        self._ck(self.lib.eve_eye_warp_fmt_to_nchw(fmt, mat, N, IH, IW, self._p(frames), self._p(warps),
                                                   None if lens is None else self._p(lens), OH, OW, self._p(out), self._stream()))
        return out

    def eye_warp_fmt_to_stem(self, frames, warps, out_hw, format, matrix='bt601', lens=None, out=None, dtype=torch.bfloat16):
        """The same patches straight into the stem's packed 16-bit input [N,OH+6,OW+8,4], as eye_warp_u8_to_stem lays it out."""
        fmt, mat, N, IH, IW, OH, OW = self._eye_warp_fmt_args(frames, warps, out_hw, format, matrix, lens)
        dst = out if out is not None else torch.empty((N, OH + 6, OW + 8, 4), dtype=dtype, device=frames.device)
        if tuple(dst.shape) != (N, OH + 6, OW + 8, 4) or dst.dtype not in HALF_DTYPES:
            raise TypeError('eye_warp: out must be bf16 / f16 [%d, %d, %d, 4], got %s %s' % (N, OH + 6, OW + 8, dst.dtype, tuple(dst.shape)))
        self._ck(self.lib.eve_eye_warp_fmt_to_stem(dt_code(dst.dtype), fmt, mat, N, IH, IW, self._p(frames), self._p(warps),
                                                   None if lens is None else self._p(lens), OH, OW, self._p(dst), self._stream()))
        return dst

    # ------------------------------------------------------------------ surfaces (data.SurfaceLayout; include/eve_hip.h eve_surface)
    @staticmethod
    def _surface_args(who, frames, layout, matrix):
        """The checks the three surface calls share -> (N, matrix code): frames uint8, contiguous, [N, ...] holding
        (N - 1) * frame_stride + frame_bytes bytes with frame_stride bytes per frame."""
        from .data import SurfaceLayout
        if not isinstance(layout, SurfaceLayout):
            raise TypeError('%s: layout must be a data.SurfaceLayout, got %s' % (who, type(layout).__name__))
        if not torch.is_tensor(frames) or frames.dtype != torch.uint8 or frames.dim() < 2:
            raise TypeError('%s: frames must be uint8 [N, one frame\'s bytes], got %s %s' % (
                who, getattr(frames, 'dtype', type(frames)), tuple(getattr(frames, 'shape', ()))))
        if matrix not in YUV_MATRICES:
            raise ValueError('%s: matrix must be one of %s, got %r' % (who, ', '.join(YUV_MATRICES), matrix))
        N = int(frames.shape[0])
        per_frame = frames.numel() // max(N, 1)
        if N < 1 or per_frame != layout.frame_stride or frames.numel() < (N - 1) * layout.frame_stride + layout.frame_bytes:
            raise ValueError('%s: frames %s hold %d bytes per frame, the layout needs a stride of %d and %d readable bytes (%r)' % (
                who, tuple(frames.shape), per_frame, layout.frame_stride, layout.frame_bytes, layout))
        if not frames.is_contiguous():
            raise RuntimeError('eve_amd: non-contiguous tensor handed to a kernel')
        return N, YUV_MATRICES[matrix]

    @staticmethod
    def _surface_warp_args(who, frames, warps, lens, N):
        if not torch.is_tensor(warps) or warps.dtype != torch.float32 or tuple(warps.shape) != (N, 3, 3):
            raise TypeError('%s: warps must be float32 [%d, 3, 3], got %s %s' % (who, N, getattr(warps, 'dtype', type(warps)),
                                                                                  tuple(getattr(warps, 'shape', ()))))
        if lens is not None and (not torch.is_tensor(lens) or lens.dtype != torch.float32 or tuple(lens.shape) != (N, 12)):
            raise TypeError('%s: lens must be float32 [%d, 12], got %s %s' % (who, N, getattr(lens, 'dtype', type(lens)),
                                                                               tuple(getattr(lens, 'shape', ()))))
        if not (warps.is_contiguous() and (lens is None or lens.is_contiguous())):
            raise RuntimeError('eve_amd: non-contiguous tensor handed to a kernel')
        if warps.device != frames.device or (lens is not None and lens.device != frames.device):
            raise RuntimeError('%s: frames, warps and lens are on different devices' % who)

    def eye_warp_surface_to_nchw(self, frames, warps, out_hw, layout, matrix='bt601', lens=None):
        """eye_warp_fmt_to_nchw on surfaces as they lie in memory: frames uint8 [N, ...] with layout.frame_stride bytes per frame,
        layout a data.SurfaceLayout; the four taps of an output pixel are read through its address rule, so the result is the
        format call's on the de-pitched, cropped, byte-linear frame, bit for bit (include/eve_hip.h eve_eye_warp_surface_to_nchw)."""
        N, mat = self._surface_args('eye_warp_surface_to_nchw', frames, layout, matrix)
        self._surface_warp_args('eye_warp_surface_to_nchw', frames, warps, lens, N)
        OH, OW = int(out_hw[0]), int(out_hw[1])
        out = torch.empty((N, 3, OH, OW), dtype=torch.float32, device=frames.device)
        surf = layout.as_ctypes()
        self._ck(self.lib.eve_eye_warp_surface_to_nchw(ctypes.byref(surf), mat, N, self._p(frames), self._p(warps),
                                                       None if lens is None else self._p(lens), OH, OW, self._p(out), self._stream()))
        return out

    def eye_warp_surface_to_stem(self, frames, warps, out_hw, layout, matrix='bt601', lens=None, out=None, dtype=torch.bfloat16):
        """The same patches straight into the stem's packed 16-bit input [N,OH+6,OW+8,4], as eye_warp_u8_to_stem lays it out."""
        N, mat = self._surface_args('eye_warp_surface_to_stem', frames, layout, matrix)
        self._surface_warp_args('eye_warp_surface_to_stem', frames, warps, lens, N)
        OH, OW = int(out_hw[0]), int(out_hw[1])
        dst = out if out is not None else torch.empty((N, OH + 6, OW + 8, 4), dtype=dtype, device=frames.device)
        if tuple(dst.shape) != (N, OH + 6, OW + 8, 4) or dst.dtype not in HALF_DTYPES:
            raise TypeError('eye_warp: out must be bf16 / f16 [%d, %d, %d, 4], got %s %s' % (N, OH + 6, OW + 8, dst.dtype, tuple(dst.shape)))
        surf = layout.as_ctypes()
        self._ck(self.lib.eve_eye_warp_surface_to_stem(dt_code(dst.dtype), ctypes.byref(surf), mat, N, self._p(frames), self._p(warps),
                                                       None if lens is None else self._p(lens), OH, OW, self._p(dst), self._stream()))
        return dst

    def screen_area_surface_to_nchw(self, frames, out_hw, layout, matrix='bt601'):
        """screen_area_fmt_to_nchw on surfaces as they lie in memory (frames and layout as for eye_warp_surface_to_nchw): every
        visible pixel is read through the layout's address rule, converted, then averaged -- the format call's bits on the
        de-pitched, cropped, byte-linear frame (include/eve_hip.h eve_screen_area_surface_to_nchw)."""
        N, mat = self._surface_args('screen_area_surface_to_nchw', frames, layout, matrix)
        OH, OW = int(out_hw[0]), int(out_hw[1])
        out = torch.empty((N, 3, OH, OW), dtype=torch.float32, device=frames.device)
        surf = layout.as_ctypes()
        self._ck(self.lib.eve_screen_area_surface_to_nchw(ctypes.byref(surf), mat, N, self._p(frames), OH, OW, self._p(out), self._stream()))
        return out

    def screen_luminance(self, frames, layout, response, weights, B, T, radii=(), centres=None, sx=1.0, sy=1.0, centre_valid=None,
                         lengths=None, matrix='bt601'):
        """The mean relative luminance of B x T screen captures where they lie, over the whole visible region and over the discs of
        `radii` capture pixels around `centres`: frames uint8 [B * T, ...] with layout.frame_stride bytes per frame, layout a
        data.SurfaceLayout (checked as for screen_area_surface_to_nchw); response uint16-valued int16 / uint16 [3, 256] on the device
        (data.display_response); weights (kr, kg, kb) integers >= 0 that sum to 65536; radii up to four strictly increasing integers
        in 1 .. 16384; centres float32 [B * T, 2] in the units that sx, sy turn into capture pixels (needed iff there are radii);
        centre_valid uint8 [B * T] or None; lengths int32 [B] or None.  -> (sums int64 [B * T, 1 + R], counts int32 [B * T, 1 + R],
        mean float32 [B * T, 1 + R]); column 0 is the whole frame (include/eve_hip.h eve_screen_luminance)."""
        who = 'screen_luminance'
        N, mat = self._surface_args(who, frames, layout, matrix)
        ok = lambda t, dtype: torch.is_tensor(t) and t.dtype == dtype
        got = lambda t: (getattr(t, 'dtype', type(t)), tuple(getattr(t, 'shape', ())))
        B, T = int(B), int(T)
        if B < 1 or T < 1 or B * T != N:
            raise ValueError('%s: frames hold %d frames, B x T is %d x %d' % (who, N, B, T))
        if not torch.is_tensor(response) or response.dtype not in (torch.int16, torch.uint16) or tuple(response.shape) != (3, 256):
            raise TypeError('%s: response must be a 16-bit integer [3, 256] tensor (data.display_response), got %s %s' % ((who,) + got(response)))
        radii = [int(r) for r in radii]
        R = len(radii)
        checks = [('lengths', lengths, torch.int32, (B,), False), ('centres', centres, torch.float32, (N, 2), R > 0),
                  ('centre_valid', centre_valid, torch.uint8, (N,), False)]
        tensors = [response]
        for name, t, dtype, shape, needed in checks:
            if (t is not None or needed) and (not ok(t, dtype) or tuple(t.shape) != shape):
                raise TypeError('%s: %s must be %s %s, got %s %s' % ((who, name, str(dtype).replace('torch.', ''), list(shape)) + got(t)))
            if t is not None:
                tensors.append(t)
        if not all(t.is_contiguous() for t in tensors):
            raise RuntimeError('eve_amd: non-contiguous tensor handed to a kernel')
        if any(t.device != frames.device for t in tensors):
            raise RuntimeError('%s: the tensors are on different devices' % who)
        kr, kg, kb = (int(w) for w in weights)
        dev = frames.device
        sums = torch.empty((N, 1 + R), dtype=torch.int64, device=dev)
        counts = torch.empty((N, 1 + R), dtype=torch.int32, device=dev)
        mean = torch.empty((N, 1 + R), dtype=torch.float32, device=dev)
        surf = layout.as_ctypes()
        self._ck(self.lib.eve_screen_luminance(
            ctypes.byref(surf), mat, B, T, self._p(frames), self._p(response), kr, kg, kb, self._p(lengths), R,
            (ctypes.c_int * R)(*radii) if R else None, self._p(centres), float(sx), float(sy), self._p(centre_valid), self._p(sums),
            self._p(counts), self._p(mean), self._stream()))
        return sums, counts, mean

    def eye_pose_normalize(self, pose, out_hw):
        """Eye normalisation derived from the head pose, both eyes of N frames in one launch: pose float32 [N,18] =
        (fx, fy, cx, cy, rvec, tvec, left eye centre, right eye centre, focal_norm, distance_norm) per frame (data.eye_pose),
        out_hw = (OH, OW) of the patch -> (head_R [N,3,3], o [2,N,3], R [2,N,3,3], warp [2,N,3,3] = inv(W), h [2,N,2] float32,
        valid uint8 [2,N]), eye-major: index 0 the left eye, 1 the right one, each a contiguous [N, ...] tensor.  An invalid eye
        has warp = 0, R = I, o = 0, h = 0 (include/eve_hip.h eve_eye_pose_normalize)."""
        if not torch.is_tensor(pose) or pose.dtype != torch.float32 or pose.dim() != 2 or pose.shape[1] != 18:
            raise TypeError('eye_pose_normalize: pose must be float32 [N, 18], got %s %s' % (getattr(pose, 'dtype', type(pose)),
                                                                                          tuple(getattr(pose, 'shape', ()))))
        if not pose.is_contiguous():
            raise RuntimeError('eve_amd: non-contiguous tensor handed to a kernel')
        N, (OH, OW) = pose.shape[0], (int(out_hw[0]), int(out_hw[1]))
        new = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=pose.device)
        head_R, o, R, warp, h = new(N, 3, 3), new(2, N, 3), new(2, N, 3, 3), new(2, N, 3, 3), new(2, N, 2)
        valid = new(2, N, dtype=torch.uint8)
        self._ck(self.lib.eve_eye_pose_normalize(N, self._p(pose), OH, OW, self._p(head_R), self._p(o), self._p(R), self._p(warp), self._p(h),
                                                 self._p(valid), self._stream()))
        return head_R, o, R, warp, h, valid

    def eye_pose_normalize_rt(self, rows, head_R, head_t, valid_in, out_hw):
        """The same normalisation from a head_R and a translation that exist already: rows float32 [S, >= 12], one per sequence,
        whose first 12 entries are (fx, fy, cx, cy, left eye centre, right eye centre, focal_norm, distance_norm) -- a face rig
        as it is -- head_R float32 [S, T, 3, 3], head_t float32 [S, T, 3], valid_in uint8 [S, T] or None (ANDed into valid) ->
        (o [2,N,3], R [2,N,3,3], warp [2,N,3,3], h [2,N,2] float32, valid uint8 [2,N]) for the N = S * T frames, eye-major like
        eye_pose_normalize (include/eve_hip.h eve_eye_pose_normalize_rt)."""
        ok = lambda t, dtype: torch.is_tensor(t) and t.dtype == dtype
        if not ok(head_R, torch.float32) or head_R.dim() != 4 or tuple(head_R.shape[2:]) != (3, 3):
            raise TypeError('eye_pose_normalize_rt: head_R must be float32 [S, T, 3, 3], got %s %s' % (
                getattr(head_R, 'dtype', type(head_R)), tuple(getattr(head_R, 'shape', ()))))
        S, T = head_R.shape[:2]
        if not ok(rows, torch.float32) or rows.dim() != 2 or rows.shape[0] != S or rows.shape[1] < 12:
            raise TypeError('eye_pose_normalize_rt: rows must be float32 [%d, >= 12], got %s %s' % (
                S, getattr(rows, 'dtype', type(rows)), tuple(getattr(rows, 'shape', ()))))
        if not ok(head_t, torch.float32) or tuple(head_t.shape) != (S, T, 3):
            raise TypeError('eye_pose_normalize_rt: head_t must be float32 [%d, %d, 3], got %s %s' % (
                S, T, getattr(head_t, 'dtype', type(head_t)), tuple(getattr(head_t, 'shape', ()))))
        if valid_in is not None and (not ok(valid_in, torch.uint8) or tuple(valid_in.shape) != (S, T)):
            raise TypeError('eye_pose_normalize_rt: valid_in must be uint8 [%d, %d], got %s %s' % (
                S, T, getattr(valid_in, 'dtype', type(valid_in)), tuple(getattr(valid_in, 'shape', ()))))
        if not all(t.is_contiguous() for t in (rows, head_R, head_t) + (() if valid_in is None else (valid_in,))):
            raise RuntimeError('eve_amd: non-contiguous tensor handed to a kernel')
        N, (OH, OW) = S * T, (int(out_hw[0]), int(out_hw[1]))
        new = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=rows.device)
        o, R, warp, h, valid = new(2, N, 3), new(2, N, 3, 3), new(2, N, 3, 3), new(2, N, 2), new(2, N, dtype=torch.uint8)
        self._ck(self.lib.eve_eye_pose_normalize_rt(N, T, self._p(rows), rows.shape[1], self._p(head_R), self._p(head_t),
                                                    None if valid_in is None else self._p(valid_in), OH, OW, self._p(o), self._p(R),
                                                    self._p(warp), self._p(h), self._p(valid), self._stream()))
        return o, R, warp, h, valid

    def face_pose_solve(self, landmarks, rig, lengths=None, state=None, reset=None):
        """Head pose from face landmarks, one wavefront per sequence, every frame warm-started from the one before: landmarks
        float32 [S, T, L, 2 | 3] = pixel (u, v[, w]) of the undistorted image, 4 <= L <= 68; rig float32 [S, 12 + 3L] (data.face_rig);
        lengths None or int32 [S] (frames past it are not solved); state None or float64 [S, 13] = (R, t, has_pose), read and
        UPDATED IN PLACE; reset None or int32 [S] -> (head_R [S,T,3,3], head_t [S,T,3], reproj_rms [S,T] float32, valid uint8
        [S,T]).  An invalid frame has head_R = I, head_t = 0, reproj_rms = 0 (include/eve_hip.h eve_face_pose_solve)."""
        ok = lambda t, dtype: torch.is_tensor(t) and t.dtype == dtype
        if not ok(landmarks, torch.float32) or landmarks.dim() != 4 or landmarks.shape[3] not in (2, 3):
            raise TypeError('face_pose_solve: landmarks must be float32 [S, T, L, 2 | 3], got %s %s' % (
                getattr(landmarks, 'dtype', type(landmarks)), tuple(getattr(landmarks, 'shape', ()))))
        S, T, L, C = landmarks.shape
        if not ok(rig, torch.float32) or tuple(rig.shape) != (S, 12 + 3 * L):
            raise TypeError('face_pose_solve: rig must be float32 [%d, %d], got %s %s' % (
                S, 12 + 3 * L, getattr(rig, 'dtype', type(rig)), tuple(getattr(rig, 'shape', ()))))
        for name, t, dtype, shape in (('lengths', lengths, torch.int32, (S,)), ('state', state, torch.float64, (S, 13)),
                                      ('reset', reset, torch.int32, (S,))):
            if t is not None and (not ok(t, dtype) or tuple(t.shape) != shape):
                raise TypeError('face_pose_solve: %s must be %s %s, got %s %s' % (
                    name, str(dtype).replace('torch.', ''), list(shape), getattr(t, 'dtype', type(t)), tuple(getattr(t, 'shape', ()))))
        given = [t for t in (landmarks, rig, lengths, state, reset) if t is not None]
        if not all(t.is_contiguous() for t in given):
            raise RuntimeError('eve_amd: non-contiguous tensor handed to a kernel')
        new = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=landmarks.device)
        head_R, head_t, rms, valid = new(S, T, 3, 3), new(S, T, 3), new(S, T), new(S, T, dtype=torch.uint8)
        opt = lambda t: None if t is None else self._p(t)
        self._ck(self.lib.eve_face_pose_solve(S, T, L, C, self._p(landmarks), self._p(rig), opt(lengths), opt(state), opt(reset),
                                              self._p(head_R), self._p(head_t), self._p(rms), self._p(valid), self._stream()))
        return head_R, head_t, rms, valid

    def face_pose_solve_ex(self, landmarks, rig, lens=None, huber_px=None, lengths=None, state=None, reset=None):
        """face_pose_solve with landmarks of the RAW frame and / or a Huber loss: lens None, or float32 [S, T, 12] rows (data.camera_lens),
        one per frame -- every landmark is undistorted on the device first, an unusable point is dropped; huber_px None, or k > 0
        pixels.  -> (head_R, head_t, reproj_rms, valid as face_pose_solve, inliers uint8 [S,T]: the points within k pixels, the used
        points without the loss, 0 on an invalid frame).  Neither given: face_pose_solve's bits (include/eve_hip.h
        eve_face_pose_solve_ex)."""
        ok = lambda t, dtype: torch.is_tensor(t) and t.dtype == dtype
        if not ok(landmarks, torch.float32) or landmarks.dim() != 4 or landmarks.shape[3] not in (2, 3):
            raise TypeError('face_pose_solve_ex: landmarks must be float32 [S, T, L, 2 | 3], got %s %s' % (
                getattr(landmarks, 'dtype', type(landmarks)), tuple(getattr(landmarks, 'shape', ()))))
        S, T, L, C = landmarks.shape
        if not ok(rig, torch.float32) or tuple(rig.shape) != (S, 12 + 3 * L):
            raise TypeError('face_pose_solve_ex: rig must be float32 [%d, %d], got %s %s' % (
                S, 12 + 3 * L, getattr(rig, 'dtype', type(rig)), tuple(getattr(rig, 'shape', ()))))
        for name, t, dtype, shape in (('lens', lens, torch.float32, (S, T, 12)), ('lengths', lengths, torch.int32, (S,)),
                                      ('state', state, torch.float64, (S, 13)), ('reset', reset, torch.int32, (S,))):
            if t is not None and (not ok(t, dtype) or tuple(t.shape) != shape):
                raise TypeError('face_pose_solve_ex: %s must be %s %s, got %s %s' % (
                    name, str(dtype).replace('torch.', ''), list(shape), getattr(t, 'dtype', type(t)), tuple(getattr(t, 'shape', ()))))
        if huber_px is not None and not (isinstance(huber_px, (int, float)) and not isinstance(huber_px, bool) and 0 < huber_px < float('inf')):
            raise ValueError('face_pose_solve_ex: huber_px must be None or a finite number > 0, got %r' % (huber_px,))
        given = [t for t in (landmarks, rig, lens, lengths, state, reset) if t is not None]
        if not all(t.is_contiguous() for t in given):
            raise RuntimeError('eve_amd: non-contiguous tensor handed to a kernel')
        new = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=landmarks.device)
        head_R, head_t, rms, valid = new(S, T, 3, 3), new(S, T, 3), new(S, T), new(S, T, dtype=torch.uint8)
        inliers = new(S, T, dtype=torch.uint8)
        opt = lambda t: None if t is None else self._p(t)
        self._ck(self.lib.eve_face_pose_solve_ex(S, T, L, C, self._p(landmarks), self._p(rig), opt(lens), 0.0 if huber_px is None else float(huber_px),
                                                 opt(lengths), opt(state), opt(reset), self._p(head_R), self._p(head_t), self._p(rms),
                                                 self._p(valid), self._p(inliers), self._stream()))
        return head_R, head_t, rms, valid, inliers

    def undistort_points(self, points, lens):
        """Raw pixels -> normalised points of the undistorted image: points float32 [N, 2], lens float32 [N, 12] (one row per
        point) or [1, 12] (one for all) -> (xy float64 [N, 2], ok uint8 [N]); ok = 0 and xy = 0 for a point the iteration cannot
        invert, a point or a lens row that is not finite (include/eve_hip.h eve_undistort_points)."""
        ok = lambda t: torch.is_tensor(t) and t.dtype == torch.float32
        if not ok(points) or points.dim() != 2 or points.shape[1] != 2 or points.shape[0] < 1:
            raise TypeError('undistort_points: points must be float32 [N, 2] with N >= 1, got %s %s' % (
                getattr(points, 'dtype', type(points)), tuple(getattr(points, 'shape', ()))))
        N = points.shape[0]
        if not ok(lens) or tuple(lens.shape) not in ((N, 12), (1, 12)):
            raise TypeError('undistort_points: lens must be float32 [%d, 12] or [1, 12], got %s %s' % (
                N, getattr(lens, 'dtype', type(lens)), tuple(getattr(lens, 'shape', ()))))
        if not (points.is_contiguous() and lens.is_contiguous()):
            raise RuntimeError('eve_amd: non-contiguous tensor handed to a kernel')
        xy = torch.empty((N, 2), dtype=torch.float64, device=points.device)
        good = torch.empty((N,), dtype=torch.uint8, device=points.device)
        stride = 12 if lens.shape[0] == N and N > 1 else 0
        self._ck(self.lib.eve_undistort_points(N, self._p(points), self._p(lens), stride, self._p(xy), self._p(good), self._stream()))
        return xy, good

    # ------------------------------------------------------------------ per-person gaze calibration
    def calib_append(self, g, head_R, origin, R, inv_cam, ppm, target, samples, count, dropped, valid=None, lengths=None, eye_valid=None):
        """Reduce the usable frames of B streams x T frames x E eyes to the offset fit's 16 doubles and append them, in frame order,
        to the stores: g [E, B, T, 2], origin [E, B, T, 3], R [E, B, T, 3, 3] (eye-major), head_R [B, T, 3, 3], inv_cam [B, T, 4, 4],
        ppm [B, T, 2], target [B, T, 2] float32; samples float64 [B, E, C, 16], count and dropped int32 [B, E], UPDATED IN PLACE;
        valid uint8 [B, T], lengths int32 [B], eye_valid uint8 [B, T, E] or None (include/eve_hip.h eve_calib_append)."""
        ok = lambda t, dtype: torch.is_tensor(t) and t.dtype == dtype
        if not ok(g, torch.float32) or g.dim() != 4 or g.shape[0] not in (1, 2) or g.shape[3] != 2:
            raise TypeError('calib_append: g must be float32 [E, B, T, 2] with E = 1 or 2, got %s %s' % (
                getattr(g, 'dtype', type(g)), tuple(getattr(g, 'shape', ()))))
        E, B, T = g.shape[:3]
        if not ok(samples, torch.float64) or samples.dim() != 4 or tuple(samples.shape[:2]) != (B, E) or samples.shape[3] != 16:
            raise TypeError('calib_append: samples must be float64 [%d, %d, C, 16], got %s %s' % (
                B, E, getattr(samples, 'dtype', type(samples)), tuple(getattr(samples, 'shape', ()))))
        C = samples.shape[2]
        for name, t, dtype, shape in (('head_R', head_R, torch.float32, (B, T, 3, 3)), ('origin', origin, torch.float32, (E, B, T, 3)),
                                      ('R', R, torch.float32, (E, B, T, 3, 3)), ('inv_cam', inv_cam, torch.float32, (B, T, 4, 4)),
                                      ('ppm', ppm, torch.float32, (B, T, 2)), ('target', target, torch.float32, (B, T, 2)),
                                      ('count', count, torch.int32, (B, E)), ('dropped', dropped, torch.int32, (B, E)),
                                      ('valid', valid, torch.uint8, (B, T)), ('lengths', lengths, torch.int32, (B,)),
                                      ('eye_valid', eye_valid, torch.uint8, (B, T, E))):
            if (t is not None or name not in ('valid', 'lengths', 'eye_valid')) and (not ok(t, dtype) or tuple(t.shape) != shape):
                raise TypeError('calib_append: %s must be %s %s, got %s %s' % (
                    name, str(dtype).replace('torch.', ''), list(shape), getattr(t, 'dtype', type(t)), tuple(getattr(t, 'shape', ()))))
        self._ck(self.lib.eve_calib_append(B, T, E, self._p(g), self._p(head_R), self._p(origin), self._p(R), self._p(inv_cam), self._p(ppm),
                                           self._p(target), self._p(valid), self._p(lengths), self._p(eye_valid), C, self._p(samples),
                                           self._p(count), self._p(dropped), self._stream()))

    def calib_fit(self, samples, count=None, select=None, huber_mm=None, min_samples=5, kappa_store=None, ok_store=None):
        """The offset fit, one wavefront per sequence: samples float64 [S, C, 16]; count int32 [S] or None (all C rows); select uint8
        [S] or None (0: the sequence is not fitted); huber_mm None or millimetres > 0; kappa_store float32 [S, 2] and ok_store uint8
        [S] (both or neither), written where the fit is ok and only there.  -> (kappa float64 [S, 2], rms_mm float64 [S], used int32
        [S], inliers int32 [S], ok uint8 [S]) (include/eve_hip.h eve_calib_fit)."""
        ok = lambda t, dtype: torch.is_tensor(t) and t.dtype == dtype
        if not ok(samples, torch.float64) or samples.dim() != 3 or samples.shape[2] != 16 or samples.shape[0] < 1 or samples.shape[1] < 1:
            raise TypeError('calib_fit: samples must be float64 [S, C, 16], got %s %s' % (
                getattr(samples, 'dtype', type(samples)), tuple(getattr(samples, 'shape', ()))))
        S, C = samples.shape[:2]
        for name, t, dtype, shape in (('count', count, torch.int32, (S,)), ('select', select, torch.uint8, (S,)),
                                      ('kappa_store', kappa_store, torch.float32, (S, 2)), ('ok_store', ok_store, torch.uint8, (S,))):
            if t is not None and (not ok(t, dtype) or tuple(t.shape) != shape):
                raise TypeError('calib_fit: %s must be %s %s, got %s %s' % (
                    name, str(dtype).replace('torch.', ''), list(shape), getattr(t, 'dtype', type(t)), tuple(getattr(t, 'shape', ()))))
        if (kappa_store is None) != (ok_store is None):
            raise TypeError('calib_fit: kappa_store and ok_store come together')
        if huber_mm is not None and not (isinstance(huber_mm, (int, float)) and not isinstance(huber_mm, bool) and 0 < huber_mm < float('inf')):
            raise ValueError('calib_fit: huber_mm must be None or a finite number > 0, got %r' % (huber_mm,))
        if isinstance(min_samples, bool) or not isinstance(min_samples, int) or min_samples < 1:
            raise ValueError('calib_fit: min_samples must be an integer >= 1, got %r' % (min_samples,))
        new = lambda *shape, dtype=torch.float64: torch.empty(shape, dtype=dtype, device=samples.device)
        kappa, rms, used, inliers, good = new(S, 2), new(S), new(S, dtype=torch.int32), new(S, dtype=torch.int32), new(S, dtype=torch.uint8)
        self._ck(self.lib.eve_calib_fit(S, C, self._p(samples), self._p(count), self._p(select), 0.0 if huber_mm is None else float(huber_mm),
                                        int(min_samples), self._p(kappa), self._p(rms), self._p(used), self._p(inliers), self._p(good),
                                        self._p(kappa_store), self._p(ok_store), self._stream()))
        return kappa, rms, used, inliers, good

    # ------------------------------------------------------------------ screen-space gaze calibration
    def screen_calib_append(self, pog, origin, inv_cam, ppm, target, screen_size, samples, count, dropped, valid=None, lengths=None,
                            frame_valid=None):
        """Reduce the usable frames of B streams x T frames to the screen map fit's 12 doubles and append them, in frame order, to
        the stores: pog [B, T, 2] (the output point before the map), origin [B, T, 3], inv_cam [B, T, 4, 4], ppm [B, T, 2], target
        [B, T, 2] float32; screen_size (W, H); samples float64 [B, C, 12], count and dropped int32 [B], UPDATED IN PLACE; valid uint8
        [B, T], lengths int32 [B], frame_valid uint8 [B, T] or None (include/eve_hip.h eve_screen_calib_append)."""
        ok = lambda t, dtype: torch.is_tensor(t) and t.dtype == dtype
        if not ok(pog, torch.float32) or pog.dim() != 3 or pog.shape[2] != 2:
            raise TypeError('screen_calib_append: pog must be float32 [B, T, 2], got %s %s' % (
                getattr(pog, 'dtype', type(pog)), tuple(getattr(pog, 'shape', ()))))
        B, T = pog.shape[:2]
        if not ok(samples, torch.float64) or samples.dim() != 3 or samples.shape[0] != B or samples.shape[2] != 12:
            raise TypeError('screen_calib_append: samples must be float64 [%d, C, 12], got %s %s' % (
                B, getattr(samples, 'dtype', type(samples)), tuple(getattr(samples, 'shape', ()))))
        C = samples.shape[1]
        for name, t, dtype, shape in (('origin', origin, torch.float32, (B, T, 3)), ('inv_cam', inv_cam, torch.float32, (B, T, 4, 4)),
                                      ('ppm', ppm, torch.float32, (B, T, 2)), ('target', target, torch.float32, (B, T, 2)),
                                      ('count', count, torch.int32, (B,)), ('dropped', dropped, torch.int32, (B,)),
                                      ('valid', valid, torch.uint8, (B, T)), ('lengths', lengths, torch.int32, (B,)),
                                      ('frame_valid', frame_valid, torch.uint8, (B, T))):
            if (t is not None or name not in ('valid', 'lengths', 'frame_valid')) and (not ok(t, dtype) or tuple(t.shape) != shape):
                raise TypeError('screen_calib_append: %s must be %s %s, got %s %s' % (
                    name, str(dtype).replace('torch.', ''), list(shape), getattr(t, 'dtype', type(t)), tuple(getattr(t, 'shape', ()))))
        for t in (pog, origin, inv_cam, ppm, target, samples, count, dropped, valid, lengths, frame_valid):
            if t is not None and not t.is_contiguous():
                raise RuntimeError('eve_amd: non-contiguous tensor handed to a kernel')
        self._ck(self.lib.eve_screen_calib_append(B, T, self._p(pog), self._p(origin), self._p(inv_cam), self._p(ppm), self._p(target),
                                                  self._p(valid), self._p(lengths), self._p(frame_valid), float(screen_size[0]),
                                                  float(screen_size[1]), C, self._p(samples), self._p(count), self._p(dropped), self._stream()))

    def screen_calib_fit(self, samples, count=None, select=None, mode=0, kind=2, huber_mm=None, min_samples=1, max_shift_mm=100.0,
                         coef_store=None, kind_store=None):
        """The screen map fit (mode 0) or the evaluation of the stored map (mode 1), one wavefront per stream: samples float64
        [S, C, 12]; count int32 [S] or None (all C rows); select uint8 [S] or None (0: the stream is not touched); kind 1 offset, 2
        affine, 3 quadratic; huber_mm None or millimetres > 0; coef_store float64 [S, 2, 6] and kind_store uint8 [S] (both or
        neither; mode 1 reads them), written in mode 0 where the fit is ok and only there.  -> (coef float64 [S, 2, 6], report
        float64 [S, 8] in the order of data.SCREEN_CALIB_REPORT, used, inliers, solves int32 [S], ok uint8 [S]) (include/eve_hip.h
        eve_screen_calib_fit)."""
        ok = lambda t, dtype: torch.is_tensor(t) and t.dtype == dtype
        if not ok(samples, torch.float64) or samples.dim() != 3 or samples.shape[2] != 12 or samples.shape[0] < 1 or samples.shape[1] < 1:
            raise TypeError('screen_calib_fit: samples must be float64 [S, C, 12], got %s %s' % (
                getattr(samples, 'dtype', type(samples)), tuple(getattr(samples, 'shape', ()))))
        S, C = samples.shape[:2]
        for name, t, dtype, shape in (('count', count, torch.int32, (S,)), ('select', select, torch.uint8, (S,)),
                                      ('coef_store', coef_store, torch.float64, (S, 2, 6)), ('kind_store', kind_store, torch.uint8, (S,))):
            if t is not None and (not ok(t, dtype) or tuple(t.shape) != shape):
                raise TypeError('screen_calib_fit: %s must be %s %s, got %s %s' % (
                    name, str(dtype).replace('torch.', ''), list(shape), getattr(t, 'dtype', type(t)), tuple(getattr(t, 'shape', ()))))
        if (coef_store is None) != (kind_store is None):
            raise TypeError('screen_calib_fit: coef_store and kind_store come together')
        if mode not in (0, 1) or (mode == 1 and coef_store is None):
            raise ValueError('screen_calib_fit: mode is 0 (fit) or 1 (evaluate coef_store / kind_store), got %r' % (mode,))
        if mode == 0 and kind not in (1, 2, 3):
            raise ValueError('screen_calib_fit: kind is 1 (offset), 2 (affine) or 3 (quadratic), got %r' % (kind,))
        if huber_mm is not None and not (isinstance(huber_mm, (int, float)) and not isinstance(huber_mm, bool) and 0 < huber_mm < float('inf')):
            raise ValueError('screen_calib_fit: huber_mm must be None or a finite number > 0, got %r' % (huber_mm,))
        if isinstance(min_samples, bool) or not isinstance(min_samples, int) or min_samples < 1:
            raise ValueError('screen_calib_fit: min_samples must be an integer >= 1, got %r' % (min_samples,))
        if isinstance(max_shift_mm, bool) or not isinstance(max_shift_mm, (int, float)) or not max_shift_mm > 0:
            raise ValueError('screen_calib_fit: max_shift_mm must be a number > 0, got %r' % (max_shift_mm,))
        for t in (samples, count, select, coef_store, kind_store):
            if t is not None and not t.is_contiguous():
                raise RuntimeError('eve_amd: non-contiguous tensor handed to a kernel')
        new = lambda *shape, dtype=torch.float64: torch.empty(shape, dtype=dtype, device=samples.device)
        coef, report = new(S, 2, 6), new(S, 8)
        used, inliers, solves, good = (new(S, dtype=torch.int32), new(S, dtype=torch.int32), new(S, dtype=torch.int32),
                                       new(S, dtype=torch.uint8))
        self._ck(self.lib.eve_screen_calib_fit(S, C, self._p(samples), self._p(count), self._p(select), int(mode), int(kind),
                                               0.0 if huber_mm is None else float(huber_mm), int(min_samples), float(max_shift_mm),
                                               self._p(coef), self._p(report), self._p(used), self._p(inliers), self._p(solves), self._p(good),
                                               self._p(coef_store), self._p(kind_store), self._stream()))
        return coef, report, used, inliers, solves, good

    def screen_calib_apply(self, px, ppm, coef, kind, screen_size):
        """The screen map applied: px float32 [B, T, 2], ppm float32 [B, T, 2], coef float64 [B, 2, 6], kind uint8 [B], screen_size
        (W, H) -> float32 [B, T, 2]; a stream of kind 0 gets its input bits (include/eve_hip.h eve_screen_calib_apply)."""
        ok = lambda t, dtype: torch.is_tensor(t) and t.dtype == dtype
        if not ok(px, torch.float32) or px.dim() != 3 or px.shape[2] != 2 or px.shape[0] < 1 or px.shape[1] < 1:
            raise TypeError('screen_calib_apply: px must be float32 [B, T, 2], got %s %s' % (
                getattr(px, 'dtype', type(px)), tuple(getattr(px, 'shape', ()))))
        B, T = px.shape[:2]
        for name, t, dtype, shape in (('ppm', ppm, torch.float32, (B, T, 2)), ('coef', coef, torch.float64, (B, 2, 6)),
                                      ('kind', kind, torch.uint8, (B,))):
            if not ok(t, dtype) or tuple(t.shape) != shape:
                raise TypeError('screen_calib_apply: %s must be %s %s, got %s %s' % (
                    name, str(dtype).replace('torch.', ''), list(shape), getattr(t, 'dtype', type(t)), tuple(getattr(t, 'shape', ()))))
        if not (px.is_contiguous() and ppm.is_contiguous() and coef.is_contiguous() and kind.is_contiguous()):
            raise RuntimeError('eve_amd: non-contiguous tensor handed to a kernel')
        out = torch.empty_like(px)
        self._ck(self.lib.eve_screen_calib_apply(B, T, self._p(px), self._p(ppm), self._p(coef), self._p(kind), float(screen_size[0]),
                                                 float(screen_size[1]), self._p(out), self._stream()))
        return out

    # ------------------------------------------------------------------ gaze filtering, fixation / saccade events
    GAZE_EVENT_KEYS = ('PoG_px_filtered', 'gaze_velocity', 'gaze_event', 'fixation_id', 'fixation_px', 'fixation_ms', 'fixating')

    def gaze_events(self, pog, origin, inv_cam, ppm, spec, state, store, count, dropped, frame_time=None, valid=None, lengths=None,
                    reset=None, flush=None):
        """The one-euro filter, the angular gaze velocity, the I-VT labels and the running fixation of B streams x T frames: pog
        [B, T, 2], origin [B, T, 3], inv_cam [B, T, 4, 4], ppm [B, T, 2] float32; spec an eve_amd.GazeEventSpec (its numbers are the
        launch's scalars); state float64 [B, 32], store float64 [B, F, 8], count and dropped int32 [B], UPDATED IN PLACE; frame_time
        float64 [B, T], valid uint8 [B, T], lengths, reset and flush int32 [B], or None.  -> a dict of GAZE_EVENT_KEYS.  pog None
        (then origin, inv_cam, ppm, frame_time and valid are None too): T = 0, a launch that only resets and flushes, -> {}
        (include/eve_hip.h eve_gaze_events)."""
        ok = lambda t, dtype: torch.is_tensor(t) and t.dtype == dtype
        if not ok(state, torch.float64) or state.dim() != 2 or state.shape[1] != 32 or state.shape[0] < 1:
            raise TypeError('gaze_events: state must be float64 [B, 32], got %s %s' % (getattr(state, 'dtype', type(state)),
                                                                                      tuple(getattr(state, 'shape', ()))))
        B = state.shape[0]
        if not ok(store, torch.float64) or store.dim() != 3 or store.shape[0] != B or store.shape[1] < 1 or store.shape[2] != 8:
            raise TypeError('gaze_events: store must be float64 [%d, F, 8], got %s %s' % (B, getattr(store, 'dtype', type(store)),
                                                                                         tuple(getattr(store, 'shape', ()))))
        F = store.shape[1]
        T = 0
        if pog is not None:
            if not ok(pog, torch.float32) or pog.dim() != 3 or pog.shape[0] != B or pog.shape[1] < 1 or pog.shape[2] != 2:
                raise TypeError('gaze_events: pog must be float32 [%d, T, 2], got %s %s' % (B, getattr(pog, 'dtype', type(pog)),
                                                                                           tuple(getattr(pog, 'shape', ()))))
            T = pog.shape[1]
        checks = [('count', count, torch.int32, (B,), True), ('dropped', dropped, torch.int32, (B,), True),
                  ('lengths', lengths, torch.int32, (B,), False), ('reset', reset, torch.int32, (B,), False),
                  ('flush', flush, torch.int32, (B,), False)]
        if T:
            checks += [('origin', origin, torch.float32, (B, T, 3), True), ('inv_cam', inv_cam, torch.float32, (B, T, 4, 4), True),
                       ('ppm', ppm, torch.float32, (B, T, 2), True), ('frame_time', frame_time, torch.float64, (B, T), False),
                       ('valid', valid, torch.uint8, (B, T), False)]
        elif any(t is not None for t in (origin, inv_cam, ppm, frame_time, valid)):
            raise TypeError('gaze_events: without pog (T = 0) there are no frame inputs')
        tensors = [state, store] + ([pog] if T else [])
        for name, t, dtype, shape, needed in checks:
            if (t is not None or needed) and (not ok(t, dtype) or tuple(t.shape) != shape):
                raise TypeError('gaze_events: %s must be %s %s, got %s %s' % (
                    name, str(dtype).replace('torch.', ''), list(shape), getattr(t, 'dtype', type(t)), tuple(getattr(t, 'shape', ()))))
            if t is not None:
                tensors.append(t)
        if not all(t.is_contiguous() for t in tensors):
            raise RuntimeError('eve_amd: non-contiguous tensor handed to a kernel')
        if T and frame_time is None and spec.fps is None:
            raise ValueError('gaze_events: without frame_time the spec needs fps')
        dev = state.device
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
        out = {}
        if T:
            out = {'PoG_px_filtered': new((B, T, 2), torch.float32), 'gaze_velocity': new((B, T), torch.float32),
                   'gaze_event': new((B, T), torch.uint8), 'fixation_id': new((B, T), torch.int32),
                   'fixation_px': new((B, T, 2), torch.float32), 'fixation_ms': new((B, T), torch.float32),
                   'fixating': new((B, T), torch.uint8)}
        self._ck(self.lib.eve_gaze_events(
            B, T, self._p(pog), self._p(origin), self._p(inv_cam), self._p(ppm), self._p(frame_time), self._p(valid), self._p(lengths),
            self._p(reset), self._p(flush), 0.0 if spec.fps is None else float(spec.fps), float(spec.min_cutoff_hz), float(spec.beta),
            float(spec.d_cutoff_hz), 1 if spec.velocity_from == 'raw' else 0, float(spec.saccade_deg_s), float(spec.min_fixation_s),
            float(spec.max_gap_s), self._p(state), F, self._p(store), self._p(count), self._p(dropped),
            *([self._p(out[k_]) for k_ in self.GAZE_EVENT_KEYS] if T else [None] * 7), self._stream()))
        return out

    GAZE_EVENT_EX_KEYS = ('sample', 'sample_time', 'gaze_vector')

    def gaze_events_ex(self, pog, origin, inv_cam, ppm, spec, state, store, count, dropped, frame_time=None, valid=None, lengths=None,
                       reset=None, flush=None):
        """gaze_events -- its arguments, its checks, its bits -- which also hands out what the launch computes on the way: -> a dict of
        GAZE_EVENT_KEYS plus sample uint8 [B, T] (0 no sample, 1 a sample that restarts the chain, 2 a chained one), sample_time float64
        [B, T] and gaze_vector float64 [B, T, 3] (zeros where sample is 0): what gaze_saccades consumes.  pog is not None: T >= 1
        (include/eve_hip.h eve_gaze_events_ex)."""
        ok = lambda t, dtype: torch.is_tensor(t) and t.dtype == dtype
        got = lambda t: (getattr(t, 'dtype', type(t)), tuple(getattr(t, 'shape', ())))
        if not ok(state, torch.float64) or state.dim() != 2 or state.shape[1] != 32 or state.shape[0] < 1:
            raise TypeError('gaze_events_ex: state must be float64 [B, 32], got %s %s' % got(state))
        B = state.shape[0]
        if not ok(store, torch.float64) or store.dim() != 3 or store.shape[0] != B or store.shape[1] < 1 or store.shape[2] != 8:
            raise TypeError('gaze_events_ex: store must be float64 [%d, F, 8], got %s %s' % ((B,) + got(store)))
        F = store.shape[1]
        if not ok(pog, torch.float32) or pog.dim() != 3 or pog.shape[0] != B or pog.shape[1] < 1 or pog.shape[2] != 2:
            raise TypeError('gaze_events_ex: pog must be float32 [%d, T, 2], got %s %s' % ((B,) + got(pog)))
        T = pog.shape[1]
        tensors = [state, store, pog]
        for name, t, dtype, shape, needed in (
                ('count', count, torch.int32, (B,), True), ('dropped', dropped, torch.int32, (B,), True),
                ('lengths', lengths, torch.int32, (B,), False), ('reset', reset, torch.int32, (B,), False),
                ('flush', flush, torch.int32, (B,), False), ('origin', origin, torch.float32, (B, T, 3), True),
                ('inv_cam', inv_cam, torch.float32, (B, T, 4, 4), True), ('ppm', ppm, torch.float32, (B, T, 2), True),
                ('frame_time', frame_time, torch.float64, (B, T), False), ('valid', valid, torch.uint8, (B, T), False)):
            if (t is not None or needed) and (not ok(t, dtype) or tuple(t.shape) != shape):
                raise TypeError('gaze_events_ex: %s must be %s %s, got %s %s' % ((name, str(dtype).replace('torch.', ''), list(shape)) + got(t)))
            if t is not None:
                tensors.append(t)
        if not all(t.is_contiguous() for t in tensors):
            raise RuntimeError('eve_amd: non-contiguous tensor handed to a kernel')
        if frame_time is None and spec.fps is None:
            raise ValueError('gaze_events_ex: without frame_time the spec needs fps')
        dev = state.device
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
        out = {'PoG_px_filtered': new((B, T, 2), torch.float32), 'gaze_velocity': new((B, T), torch.float32),
               'gaze_event': new((B, T), torch.uint8), 'fixation_id': new((B, T), torch.int32),
               'fixation_px': new((B, T, 2), torch.float32), 'fixation_ms': new((B, T), torch.float32),
               'fixating': new((B, T), torch.uint8), 'sample': new((B, T), torch.uint8), 'sample_time': new((B, T), torch.float64),
               'gaze_vector': new((B, T, 3), torch.float64)}
        self._ck(self.lib.eve_gaze_events_ex(
            B, T, self._p(pog), self._p(origin), self._p(inv_cam), self._p(ppm), self._p(frame_time), self._p(valid), self._p(lengths),
            self._p(reset), self._p(flush), 0.0 if spec.fps is None else float(spec.fps), float(spec.min_cutoff_hz), float(spec.beta),
            float(spec.d_cutoff_hz), 1 if spec.velocity_from == 'raw' else 0, float(spec.saccade_deg_s), float(spec.min_fixation_s),
            float(spec.max_gap_s), self._p(state), F, self._p(store), self._p(count), self._p(dropped),
            *[self._p(out[k_]) for k_ in self.GAZE_EVENT_KEYS + self.GAZE_EVENT_EX_KEYS], self._stream()))
        return out

    # ------------------------------------------------------------------ saccades as events
    GAZE_SACCADE_KEYS = ('saccade_id', 'saccade_ms')

    def gaze_saccades(self, sample, sample_time, gaze_vector, point, event, velocity, fixation_id, spec, state, table, store, count, dropped,
                      lengths=None, reset=None):
        """The saccades of B streams x T frames, cut from the events launch's labels: sample uint8 [B, T], sample_time float64 [B, T],
        gaze_vector float64 [B, T, 3] (gaze_events_ex's), point float32 [B, T, 2] (the point the velocity is from), event uint8 [B, T],
        velocity float32 [B, T], fixation_id int32 [B, T]; spec an eve_amd.SaccadeSpec (its numbers are the launch's scalars); state
        float64 [B, 32], table float64 [B, 16], store float64 [B, S, 16], count and dropped int32 [B], UPDATED IN PLACE; lengths and reset
        int32 [B], or None.  -> a dict of GAZE_SACCADE_KEYS: saccade_id int32 [B, T] (-1 outside a saccade), saccade_ms float32 [B, T].
        sample None (then every frame input is None too): T = 0, a launch that only resets, -> {} (include/eve_hip.h
        eve_gaze_saccades)."""
        ok = lambda t, dtype: torch.is_tensor(t) and t.dtype == dtype
        got = lambda t: (getattr(t, 'dtype', type(t)), tuple(getattr(t, 'shape', ())))
        if not ok(state, torch.float64) or state.dim() != 2 or state.shape[1] != 32 or state.shape[0] < 1:
            raise TypeError('gaze_saccades: state must be float64 [B, 32], got %s %s' % got(state))
        B = state.shape[0]
        if not ok(store, torch.float64) or store.dim() != 3 or store.shape[0] != B or store.shape[1] < 1 or store.shape[2] != 16:
            raise TypeError('gaze_saccades: store must be float64 [%d, S, 16], got %s %s' % ((B,) + got(store)))
        S = store.shape[1]
        T = 0
        if sample is not None:
            if not ok(sample, torch.uint8) or sample.dim() != 2 or sample.shape[0] != B or sample.shape[1] < 1:
                raise TypeError('gaze_saccades: sample must be uint8 [%d, T], got %s %s' % ((B,) + got(sample)))
            T = sample.shape[1]
        checks = [('table', table, torch.float64, (B, 16), True), ('count', count, torch.int32, (B,), True),
                  ('dropped', dropped, torch.int32, (B,), True), ('lengths', lengths, torch.int32, (B,), False),
                  ('reset', reset, torch.int32, (B,), False)]
        if T:
            checks += [('sample_time', sample_time, torch.float64, (B, T), True), ('gaze_vector', gaze_vector, torch.float64, (B, T, 3), True),
                       ('point', point, torch.float32, (B, T, 2), True), ('event', event, torch.uint8, (B, T), True),
                       ('velocity', velocity, torch.float32, (B, T), True), ('fixation_id', fixation_id, torch.int32, (B, T), True)]
        elif any(t is not None for t in (sample_time, gaze_vector, point, event, velocity, fixation_id)):
            raise TypeError('gaze_saccades: without sample (T = 0) there are no frame inputs')
        tensors = [state, store] + ([sample] if T else [])
        for name, t, dtype, shape, needed in checks:
            if (t is not None or needed) and (not ok(t, dtype) or tuple(t.shape) != shape):
                raise TypeError('gaze_saccades: %s must be %s %s, got %s %s' % ((name, str(dtype).replace('torch.', ''), list(shape)) + got(t)))
            if t is not None:
                tensors.append(t)
        if not all(t.is_contiguous() for t in tensors):
            raise RuntimeError('eve_amd: non-contiguous tensor handed to a kernel')
        dev = state.device
        out = {}
        if T:
            out = {'saccade_id': torch.empty((B, T), dtype=torch.int32, device=dev), 'saccade_ms': torch.empty((B, T), dtype=torch.float32, device=dev)}
        self._ck(self.lib.eve_gaze_saccades(
            B, T, self._p(sample), self._p(sample_time), self._p(gaze_vector), self._p(point), self._p(event), self._p(velocity),
            self._p(fixation_id), self._p(lengths), self._p(reset), float(spec.min_amplitude_deg), float(spec.min_duration_s),
            float(spec.max_duration_s), int(spec.max_missing), self._p(state), self._p(table), S, self._p(store), self._p(count),
            self._p(dropped), *([self._p(out[k_]) for k_ in self.GAZE_SACCADE_KEYS] if T else [None] * 2), self._stream()))
        return out

    # ------------------------------------------------------------------ smooth pursuit
    GAZE_PURSUIT_KEYS = ('gaze_class', 'pursuit_id', 'pursuit_ms', 'gaze_velocity_windowed', 'gaze_straightness', 'pursuit_gain')

    def gaze_pursuits(self, sample, sample_time, gaze_vector, point, event, velocity, fixation_id, spec, state, table, store, count, dropped,
                      target=None, lengths=None, reset=None):
        """The smooth pursuit of B streams x T frames, found among the events launch's fixation frames: gaze_saccades' frame inputs
        (sample uint8 [B, T], sample_time float64 [B, T], gaze_vector float64 [B, T, 3], point float32 [B, T, 2], event uint8 [B, T],
        velocity float32 [B, T], fixation_id int32 [B, T]) plus target float32 [B, T, 2] or None (the pursued object's screen position,
        NaN where there is none); spec an eve_amd.PursuitSpec (its numbers are the launch's scalars); state float64 [B, 320], table
        float64 [B, 16], store float64 [B, S, 20], count and dropped int32 [B], UPDATED IN PLACE; lengths and reset int32 [B], or None.
        -> a dict of GAZE_PURSUIT_KEYS: gaze_class uint8 [B, T] (0 none, 1 fixation, 2 saccade, 3 pursuit), pursuit_id int32 [B, T]
        (-1 outside an episode), pursuit_ms, gaze_velocity_windowed, gaze_straightness and pursuit_gain float32 [B, T] (the last three
        NaN where undefined).  sample None (then every frame input is None too): T = 0, a launch that only resets, -> {}
        (include/eve_hip.h eve_gaze_pursuits)."""
        ok = lambda t, dtype: torch.is_tensor(t) and t.dtype == dtype
        got = lambda t: (getattr(t, 'dtype', type(t)), tuple(getattr(t, 'shape', ())))
        if not ok(state, torch.float64) or state.dim() != 2 or state.shape[1] != 320 or state.shape[0] < 1:
            raise TypeError('gaze_pursuits: state must be float64 [B, 320], got %s %s' % got(state))
        B = state.shape[0]
        if not ok(store, torch.float64) or store.dim() != 3 or store.shape[0] != B or store.shape[1] < 1 or store.shape[2] != 20:
            raise TypeError('gaze_pursuits: store must be float64 [%d, S, 20], got %s %s' % ((B,) + got(store)))
        S = store.shape[1]
        T = 0
        if sample is not None:
            if not ok(sample, torch.uint8) or sample.dim() != 2 or sample.shape[0] != B or sample.shape[1] < 1:
                raise TypeError('gaze_pursuits: sample must be uint8 [%d, T], got %s %s' % ((B,) + got(sample)))
            T = sample.shape[1]
        checks = [('table', table, torch.float64, (B, 16), True), ('count', count, torch.int32, (B,), True),
                  ('dropped', dropped, torch.int32, (B,), True), ('lengths', lengths, torch.int32, (B,), False),
                  ('reset', reset, torch.int32, (B,), False)]
        if T:
            checks += [('sample_time', sample_time, torch.float64, (B, T), True), ('gaze_vector', gaze_vector, torch.float64, (B, T, 3), True),
                       ('point', point, torch.float32, (B, T, 2), True), ('event', event, torch.uint8, (B, T), True),
                       ('velocity', velocity, torch.float32, (B, T), True), ('fixation_id', fixation_id, torch.int32, (B, T), True),
                       ('target', target, torch.float32, (B, T, 2), False)]
        elif any(t is not None for t in (sample_time, gaze_vector, point, event, velocity, fixation_id, target)):
            raise TypeError('gaze_pursuits: without sample (T = 0) there are no frame inputs')
        tensors = [state, store] + ([sample] if T else [])
        for name, t, dtype, shape, needed in checks:
            if (t is not None or needed) and (not ok(t, dtype) or tuple(t.shape) != shape):
                raise TypeError('gaze_pursuits: %s must be %s %s, got %s %s' % ((name, str(dtype).replace('torch.', ''), list(shape)) + got(t)))
            if t is not None:
                tensors.append(t)
        if not all(t.is_contiguous() for t in tensors):
            raise RuntimeError('eve_amd: non-contiguous tensor handed to a kernel')
        dev = state.device
        out = {}
        if T:
            dtypes = (torch.uint8, torch.int32, torch.float32, torch.float32, torch.float32, torch.float32)
            out = {k_: torch.empty((B, T), dtype=dt, device=dev) for k_, dt in zip(self.GAZE_PURSUIT_KEYS, dtypes)}
        self._ck(self.lib.eve_gaze_pursuits(
            B, T, self._p(sample), self._p(sample_time), self._p(gaze_vector), self._p(point), self._p(event), self._p(velocity),
            self._p(fixation_id), self._p(target), self._p(lengths), self._p(reset), float(spec.window_s), float(spec.min_window_s),
            float(spec.pursuit_deg_s), float(spec.min_straightness), float(spec.settle_s), float(spec.min_duration_s),
            float(spec.min_amplitude_deg), int(spec.max_missing), self._p(state), self._p(table), S, self._p(store), self._p(count),
            self._p(dropped), *([self._p(out[k_]) for k_ in self.GAZE_PURSUIT_KEYS] if T else [None] * 6), self._stream()))
        return out

    # ------------------------------------------------------------------ the time-decayed gaze history
    def gaze_history_plan(self, P, screen_size, state, T, pog=None, frame_time=None, valid=None, valid_key=None, lengths=None, reset=None):
        """The time chain of the gaze history for B streams x T frames: P the launch's scalars (data.GazeHistorySpec.launch_params:
        size (MW, MH), ln_decay, seconds, max_gap_s, fps or None, gain, ...), screen_size (W, H); state float64 [B, 8], UPDATED IN PLACE;
        pog float32 [B, T, 2] or None (the heat source), frame_time float64 [B, T], valid and valid_key uint8 [B, T], lengths and reset
        int32 [B], or None.  -> (coef float64 [B, T, 4], clear int32 [B]) for gaze_history_update (include/eve_hip.h
        eve_gaze_history_plan)."""
        ok = lambda t, dtype: torch.is_tensor(t) and t.dtype == dtype
        if not ok(state, torch.float64) or state.dim() != 2 or state.shape[1] != 8 or state.shape[0] < 1:
            raise TypeError('gaze_history_plan: state must be float64 [B, 8], got %s %s' % (getattr(state, 'dtype', type(state)),
                                                                                          tuple(getattr(state, 'shape', ()))))
        B, T = state.shape[0], int(T)
        tensors = [state]
        for name, t, dtype, shape in (('pog', pog, torch.float32, (B, T, 2)), ('frame_time', frame_time, torch.float64, (B, T)),
                                      ('valid', valid, torch.uint8, (B, T)), ('valid_key', valid_key, torch.uint8, (B, T)),
                                      ('lengths', lengths, torch.int32, (B,)), ('reset', reset, torch.int32, (B,))):
            if t is not None:
                if not ok(t, dtype) or tuple(t.shape) != shape:
                    raise TypeError('gaze_history_plan: %s must be %s %s, got %s %s' % (
                        name, str(dtype).replace('torch.', ''), list(shape), getattr(t, 'dtype', type(t)), tuple(getattr(t, 'shape', ()))))
                tensors.append(t)
        if not all(t.is_contiguous() for t in tensors):
            raise RuntimeError('eve_amd: non-contiguous tensor handed to a kernel')
        if T and frame_time is None and P['fps'] is None:
            raise ValueError('gaze_history_plan: without frame_time the spec needs fps')
        coef = torch.empty((B, T, 4), dtype=torch.float64, device=state.device)
        clear = torch.empty((B,), dtype=torch.int32, device=state.device)
        self._ck(self.lib.eve_gaze_history_plan(
            B, T, self._p(pog), self._p(frame_time), self._p(valid), self._p(valid_key), self._p(lengths), self._p(reset),
            0.0 if P['fps'] is None else float(P['fps']), float(P['ln_decay']), 1 if P['seconds'] else 0, float(P['max_gap_s']), float(P['gain']),
            int(P['size'][0]), int(P['size'][1]), float(screen_size[0]), float(screen_size[1]), self._p(state), self._p(coef) if T else None,
            self._p(clear), self._stream()))
        return coef, clear

    def gaze_history_update(self, P, coef, clear, maps, heat=None, per_frame=False):
        """The plan's rows applied to the maps: coef float64 [B, T, 4] and clear int32 [B] from gaze_history_plan, maps float32
        [B, MH, MW], UPDATED IN PLACE, heat None or float32 [B, T, MH, MW].  -> the map after every frame, float32 [B, T, MH, MW], where
        per_frame, else None (include/eve_hip.h eve_gaze_history_update)."""
        ok = lambda t, dtype: torch.is_tensor(t) and t.dtype == dtype
        MW, MH = int(P['size'][0]), int(P['size'][1])
        if not ok(maps, torch.float32) or maps.dim() != 3 or tuple(maps.shape[1:]) != (MH, MW) or maps.shape[0] < 1:
            raise TypeError('gaze_history_update: maps must be float32 [B, %d, %d], got %s %s' % (MH, MW, getattr(maps, 'dtype', type(maps)),
                                                                                                tuple(getattr(maps, 'shape', ()))))
        B = maps.shape[0]
        if not ok(coef, torch.float64) or coef.dim() != 3 or coef.shape[0] != B or coef.shape[2] != 4:
            raise TypeError('gaze_history_update: coef must be float64 [%d, T, 4], got %s %s' % (B, getattr(coef, 'dtype', type(coef)),
                                                                                               tuple(getattr(coef, 'shape', ()))))
        T = coef.shape[1]
        if not ok(clear, torch.int32) or tuple(clear.shape) != (B,):
            raise TypeError('gaze_history_update: clear must be int32 [%d]' % B)
        if heat is not None and (not ok(heat, torch.float32) or tuple(heat.shape) != (B, T, MH, MW)):
            raise TypeError('gaze_history_update: heat must be float32 [%d, %d, %d, %d], got %s %s' % (
                B, T, MH, MW, getattr(heat, 'dtype', type(heat)), tuple(getattr(heat, 'shape', ()))))
        if not all(t.is_contiguous() for t in (maps, coef, clear) + (() if heat is None else (heat,))):
            raise RuntimeError('eve_amd: non-contiguous tensor handed to a kernel')
        frames = torch.empty((B, T, MH, MW), dtype=torch.float32, device=maps.device) if per_frame else None
        self._ck(self.lib.eve_gaze_history_update(B, T, MH, MW, self._p(coef) if T else None, self._p(clear), self._p(heat), float(P['alpha']),
                                                  float(P['floor']), self._p(maps), self._p(frames), self._stream()))
        return frames

    # ------------------------------------------------------------------ areas of interest
    GAZE_AOI_KEYS = ('id', 'mask', 'visit_ms')

    def gaze_aoi(self, pog, shapes, spec, state, table, trans, visits, count, dropped, frame_time=None, valid=None, valid_key=None,
                 fixation_id=None, fixating=None, lengths=None, reset=None, flush=None):
        """The hit tests, visits, dwell table and transitions of B streams x T frames against A areas of interest: pog float32
        [B, T, 2]; shapes float32 [B, A, 36], or [B, T, A, 36] with one table per frame (data.aoi_shapes has the rows); spec an
        eve_amd.AoiSpec (fps and max_gap_s are the launch's scalars); state float64 [B, 16], table float64 [B, A + 1, 8], trans int32
        [B, A + 1, A], visits float64 [B, V, 8], count and dropped int32 [B], UPDATED IN PLACE; frame_time float64 [B, T], valid and
        valid_key uint8 [B, T], fixation_id int32 [B, T] with fixating uint8 [B, T], lengths, reset and flush int32 [B], or None.  -> a
        dict of GAZE_AOI_KEYS: id int32 [B, T], mask int64 [B, T], visit_ms float32 [B, T].  pog None (then every frame input is None
        too): T = 0, a launch that only resets and flushes, -> {} (include/eve_hip.h eve_gaze_aoi)."""
        ok = lambda t, dtype: torch.is_tensor(t) and t.dtype == dtype
        got = lambda t: (getattr(t, 'dtype', type(t)), tuple(getattr(t, 'shape', ())))
        if not ok(state, torch.float64) or state.dim() != 2 or state.shape[1] != 16 or state.shape[0] < 1:
            raise TypeError('gaze_aoi: state must be float64 [B, 16], got %s %s' % got(state))
        B = state.shape[0]
        if not ok(table, torch.float64) or table.dim() != 3 or table.shape[0] != B or not 2 <= table.shape[1] <= 65 or table.shape[2] != 8:
            raise TypeError('gaze_aoi: table must be float64 [%d, A + 1, 8] with A in 1 .. 64, got %s %s' % ((B,) + got(table)))
        A = table.shape[1] - 1
        if not ok(visits, torch.float64) or visits.dim() != 3 or visits.shape[0] != B or visits.shape[1] < 1 or visits.shape[2] != 8:
            raise TypeError('gaze_aoi: visits must be float64 [%d, V, 8], got %s %s' % ((B,) + got(visits)))
        V = visits.shape[1]
        T = 0
        if pog is not None:
            if not ok(pog, torch.float32) or pog.dim() != 3 or pog.shape[0] != B or pog.shape[1] < 1 or pog.shape[2] != 2:
                raise TypeError('gaze_aoi: pog must be float32 [%d, T, 2], got %s %s' % ((B,) + got(pog)))
            T = pog.shape[1]
        checks = [('trans', trans, torch.int32, (B, A + 1, A), True), ('count', count, torch.int32, (B,), True),
                  ('dropped', dropped, torch.int32, (B,), True), ('lengths', lengths, torch.int32, (B,), False),
                  ('reset', reset, torch.int32, (B,), False), ('flush', flush, torch.int32, (B,), False)]
        per_frame = False
        if T:
            per_frame = torch.is_tensor(shapes) and shapes.dim() == 4
            checks += [('shapes', shapes, torch.float32, (B, T, A, 36) if per_frame else (B, A, 36), True),
                       ('frame_time', frame_time, torch.float64, (B, T), False), ('valid', valid, torch.uint8, (B, T), False),
                       ('valid_key', valid_key, torch.uint8, (B, T), False), ('fixation_id', fixation_id, torch.int32, (B, T), False),
                       ('fixating', fixating, torch.uint8, (B, T), False)]
            if (fixation_id is None) != (fixating is None):
                raise TypeError('gaze_aoi: fixation_id and fixating come together')
        elif any(t is not None for t in (shapes, frame_time, valid, valid_key, fixation_id, fixating)):
            raise TypeError('gaze_aoi: without pog (T = 0) there are no frame inputs')
        tensors = [state, table, visits] + ([pog] if T else [])
        for name, t, dtype, shape, needed in checks:
            if (t is not None or needed) and (not ok(t, dtype) or tuple(t.shape) != shape):
                raise TypeError('gaze_aoi: %s must be %s %s, got %s %s' % ((name, str(dtype).replace('torch.', ''), list(shape)) + got(t)))
            if t is not None:
                tensors.append(t)
        if not all(t.is_contiguous() for t in tensors):
            raise RuntimeError('eve_amd: non-contiguous tensor handed to a kernel')
        if T and frame_time is None and spec.fps is None:
            raise ValueError('gaze_aoi: without frame_time the spec needs fps')
        dev = state.device
        out = {}
        if T:
            out = {'id': torch.empty((B, T), dtype=torch.int32, device=dev), 'mask': torch.empty((B, T), dtype=torch.int64, device=dev),
                   'visit_ms': torch.empty((B, T), dtype=torch.float32, device=dev)}
        self._ck(self.lib.eve_gaze_aoi(
            B, T, A, self._p(pog), self._p(shapes), 1 if per_frame else 0, self._p(frame_time), self._p(valid), self._p(valid_key),
            self._p(fixation_id), self._p(fixating), self._p(lengths), self._p(reset), self._p(flush),
            0.0 if spec.fps is None else float(spec.fps), float(spec.max_gap_s), self._p(state), self._p(table), self._p(trans), V,
            self._p(visits), self._p(count), self._p(dropped), *([self._p(out[k_]) for k_ in self.GAZE_AOI_KEYS] if T else [None] * 3),
            self._stream()))
        return out

    # ------------------------------------------------------------------ pupillometry
    PUPIL_KEYS = ('mm', 'raw_mm', 'velocity', 'change_mm', 'change_pct', 'valid', 'eye_used', 'eye_reason', 'event')

    def pupil_track(self, size, spec, state, table, light, store, count, dropped, eye_valid=None, frame_time=None, lengths=None, reset=None,
                    flush=None, luminance=None, baseline_mark=None):
        """The validated, fused, filtered and baseline-corrected pupil trace, its tallies and its dilation / constriction episodes for B
        streams x T frames: size float32 [2, B, T] (left, right; mm); spec an eve_amd.PupilSpec (its numbers are the launch's scalars);
        state float64 [B, 32], table float64 [B, 24], store float64 [B, capacity, 8], count and dropped int32 [B], UPDATED IN PLACE;
        light float64 [B, 4] (has_gain, gain, ref, 0), read; eye_valid uint8 [B, T, 2], frame_time float64 [B, T], luminance float32
        [B, T], baseline_mark uint8 [B, T], lengths, reset and flush int32 [B], or None.  -> a dict of PUPIL_KEYS: mm, raw_mm, velocity,
        change_mm, change_pct float32 [B, T], valid and event uint8 [B, T], eye_used and eye_reason uint8 [B, T, 2].  size None (then
        every frame input is None too): T = 0, a launch that only resets and flushes, -> {} (include/eve_hip.h eve_pupil_track)."""
        ok = lambda t, dtype: torch.is_tensor(t) and t.dtype == dtype
        got = lambda t: (getattr(t, 'dtype', type(t)), tuple(getattr(t, 'shape', ())))
        if not ok(state, torch.float64) or state.dim() != 2 or state.shape[1] != 32 or state.shape[0] < 1:
            raise TypeError('pupil_track: state must be float64 [B, 32], got %s %s' % got(state))
        B = state.shape[0]
        if not ok(store, torch.float64) or store.dim() != 3 or store.shape[0] != B or store.shape[1] < 1 or store.shape[2] != 8:
            raise TypeError('pupil_track: store must be float64 [%d, capacity, 8], got %s %s' % ((B,) + got(store)))
        V = store.shape[1]
        T = 0
        if size is not None:
            if not ok(size, torch.float32) or size.dim() != 3 or size.shape[0] != 2 or size.shape[1] != B or size.shape[2] < 1:
                raise TypeError('pupil_track: size must be float32 [2, %d, T], got %s %s' % ((B,) + got(size)))
            T = size.shape[2]
        checks = [('table', table, torch.float64, (B, 24), True), ('light', light, torch.float64, (B, 4), True),
                  ('count', count, torch.int32, (B,), True), ('dropped', dropped, torch.int32, (B,), True),
                  ('lengths', lengths, torch.int32, (B,), False), ('reset', reset, torch.int32, (B,), False),
                  ('flush', flush, torch.int32, (B,), False)]
        if T:
            checks += [('eye_valid', eye_valid, torch.uint8, (B, T, 2), False), ('frame_time', frame_time, torch.float64, (B, T), False),
                       ('luminance', luminance, torch.float32, (B, T), False), ('baseline_mark', baseline_mark, torch.uint8, (B, T), False)]
        elif any(t is not None for t in (eye_valid, frame_time, luminance, baseline_mark)):
            raise TypeError('pupil_track: without size (T = 0) there are no frame inputs')
        tensors = [state, store] + ([size] if T else [])
        for name, t, dtype, shape, needed in checks:
            if (t is not None or needed) and (not ok(t, dtype) or tuple(t.shape) != shape):
                raise TypeError('pupil_track: %s must be %s %s, got %s %s' % ((name, str(dtype).replace('torch.', ''), list(shape)) + got(t)))
            if t is not None:
                tensors.append(t)
        if not all(t.is_contiguous() for t in tensors):
            raise RuntimeError('eve_amd: non-contiguous tensor handed to a kernel')
        if T and frame_time is None and spec.fps is None:
            raise ValueError('pupil_track: without frame_time the spec needs fps')
        dev = state.device
        out = {}
        if T:
            out = {k_: torch.empty((B, T), dtype=torch.float32, device=dev) for k_ in self.PUPIL_KEYS[:5]}
            out.update(valid=torch.empty((B, T), dtype=torch.uint8, device=dev), eye_used=torch.empty((B, T, 2), dtype=torch.uint8, device=dev),
                       eye_reason=torch.empty((B, T, 2), dtype=torch.uint8, device=dev), event=torch.empty((B, T), dtype=torch.uint8, device=dev))
        self._ck(self.lib.eve_pupil_track(
            B, T, self._p(size), self._p(eye_valid), self._p(frame_time), self._p(lengths), self._p(reset), self._p(flush), self._p(luminance),
            self._p(baseline_mark), 0.0 if spec.fps is None else float(spec.fps), float(spec.min_mm), float(spec.max_mm),
            float(spec.max_speed_mm_s), float(spec.max_gap_s), float(spec.offset_rate), float(spec.cutoff_hz), float(spec.light_tau_s),
            0.0 if spec.baseline_tau_s is None else float(spec.baseline_tau_s), float(spec.dilate_mm_s), float(spec.constrict_mm_s),
            float(spec.min_amplitude_mm), self._p(state), self._p(table), self._p(light), V, self._p(store), self._p(count), self._p(dropped),
            *([self._p(out[k_]) for k_ in self.PUPIL_KEYS] if T else [None] * 9), self._stream()))
        return out

    # ------------------------------------------------------------------ the eye gate
    def eye_gate(self, spec, B, T, state, store, count, dropped, pose_valid=None, reproj_rms=None, inliers=None, warp=None, h=None,
                 contours=None, lengths=None, reset=None, frame_size=None, patch_size=None):
        """Per frame and eye: is the eye usable, and is it blinking?  spec an eve_amd.EyeGateSpec (its numbers are the launch's
        parameter block); state float64 [B, 2, 8], store float64 [B, capacity, 4], count and dropped int32 [B], UPDATED IN PLACE;
        pose_valid uint8 [B, T, 2], reproj_rms float32 [B, T], inliers uint8 [B, T], warp float32 [2, B*T, 9] with frame_size (IW, IH)
        and patch_size (OW, OH), h float32 [2, B*T, 2], contours float32 [B, T, 2, 6, 2 | 3], lengths and reset int32 [B], or None: an
        input that is None turns its criterion off, and an input whose criterion the spec leaves off must be None.  -> {'usable',
        'reason', 'blink': uint8 [B, T, 2], 'openness': float32 [B, T, 2]} (include/eve_hip.h eve_eye_gate)."""
        from ._lib import EyeGateParams
        ok = lambda t, dtype: torch.is_tensor(t) and t.dtype == dtype
        B, T = int(B), int(T)
        if B < 1 or T < 1:
            raise ValueError('eye_gate: B and T must be >= 1, got %d and %d' % (B, T))
        if not ok(state, torch.float64) or tuple(state.shape) != (B, 2, 8):
            raise TypeError('eye_gate: state must be float64 [%d, 2, 8], got %s %s' % (B, getattr(state, 'dtype', type(state)),
                                                                                        tuple(getattr(state, 'shape', ()))))
        if not ok(store, torch.float64) or store.dim() != 3 or store.shape[0] != B or store.shape[1] < 1 or store.shape[2] != 4:
            raise TypeError('eye_gate: store must be float64 [%d, capacity, 4], got %s %s' % (B, getattr(store, 'dtype', type(store)),
                                                                                               tuple(getattr(store, 'shape', ()))))
        C = 0
        if contours is not None:
            if not ok(contours, torch.float32) or contours.dim() != 5 or tuple(contours.shape[:4]) != (B, T, 2, 6) or contours.shape[4] not in (2, 3):
                raise TypeError('eye_gate: contours must be float32 [%d, %d, 2, 6, 2 | 3], got %s %s' % (
                    B, T, getattr(contours, 'dtype', type(contours)), tuple(getattr(contours, 'shape', ()))))
            C = contours.shape[4]
        checks = [('count', count, torch.int32, (B,), True), ('dropped', dropped, torch.int32, (B,), True),
                  ('pose_valid', pose_valid, torch.uint8, (B, T, 2), False), ('reproj_rms', reproj_rms, torch.float32, (B, T), False),
                  ('inliers', inliers, torch.uint8, (B, T), False), ('warp', warp, torch.float32, (2, B * T, 9), False),
                  ('h', h, torch.float32, (2, B * T, 2), False), ('lengths', lengths, torch.int32, (B,), False),
                  ('reset', reset, torch.int32, (B,), False)]
        tensors = [state, store] + ([contours] if contours is not None else [])
        for name, t, dtype, shape, needed in checks:
            if (t is not None or needed) and (not ok(t, dtype) or tuple(t.shape) != shape):
                raise TypeError('eye_gate: %s must be %s %s, got %s %s' % (
                    name, str(dtype).replace('torch.', ''), list(shape), getattr(t, 'dtype', type(t)), tuple(getattr(t, 'shape', ()))))
            if t is not None:
                tensors.append(t)
        if not all(t.is_contiguous() for t in tensors):
            raise RuntimeError('eve_amd: non-contiguous tensor handed to a kernel')
        for name, t, on in (('reproj_rms', reproj_rms, spec.max_reproj_px is not None), ('inliers', inliers, spec.min_inliers is not None),
                            ('warp', warp, spec.min_coverage is not None), ('h', h, spec.head_angles), ('contours', contours, spec.blink is not None)):
            if (t is not None) != bool(on):
                raise ValueError('eye_gate: %s goes with its criterion in the spec, and only with it' % name)
        IW = IH = OW = OH = 0
        if warp is not None:
            if frame_size is None or patch_size is None:
                raise ValueError('eye_gate: warp needs frame_size (IW, IH) and patch_size (OW, OH)')
            (IW, IH), (OW, OH) = (int(v) for v in frame_size), (int(v) for v in patch_size)
        inf = float('inf')
        rng = lambda r: (-inf, inf) if r is None else r
        P = EyeGateParams()
        P.max_reproj_px = inf if spec.max_reproj_px is None else spec.max_reproj_px
        P.pitch_lo, P.pitch_hi = rng(spec.head_pitch)
        for e, r in enumerate((spec.head_yaw_left, spec.head_yaw_right)):
            P.yaw_lo[e], P.yaw_hi[e] = rng(r)
        P.min_inliers = 0 if spec.min_inliers is None else spec.min_inliers
        P.min_inside = 1 if spec.min_coverage is None else spec.min_inside
        bl = spec.blink
        P.close_ratio, P.open_ratio = (0.0, 1.0) if bl is None else (bl.close_ratio, bl.open_ratio)
        P.baseline_rate, P.baseline_rise = (0.0, 0.0) if bl is None else (bl.baseline_rate, bl.baseline_rise)
        P.hold_frames, P.max_closed_frames = (0, 1) if bl is None else (bl.hold_frames, bl.max_closed_frames)
        dev = state.device
        out = {'usable': torch.empty((B, T, 2), dtype=torch.uint8, device=dev), 'reason': torch.empty((B, T, 2), dtype=torch.uint8, device=dev),
               'openness': torch.empty((B, T, 2), dtype=torch.float32, device=dev), 'blink': torch.empty((B, T, 2), dtype=torch.uint8, device=dev)}
        self._ck(self.lib.eve_eye_gate(
            B, T, self._p(pose_valid), self._p(reproj_rms), self._p(inliers), self._p(warp), self._p(h), self._p(contours), C, self._p(lengths),
            self._p(reset), IW, IH, OW, OH, ctypes.byref(P), self._p(state), store.shape[1], self._p(store), self._p(count), self._p(dropped),
            self._p(out['usable']), self._p(out['reason']), self._p(out['openness']), self._p(out['blink']), self._stream()))
        return out

    # ------------------------------------------------------------------ gaze geometry / heat-maps / soft-argmax
    def _flat32(self, t, shape, what):
        t = t.contiguous()
        assert t.dtype == torch.float32 and tuple(t.shape) == tuple(shape), (what, t.dtype, tuple(t.shape), tuple(shape))
        self._p(t)                                   # device check
        return t

    def gaze_to_pog(self, g, origin, R, inv_cam, ppm, screen, head_R=None, kappa=None):
        """Flat N frames.  Returns (g_out [N,2], pog_mm [N,2], pog_px [N,2], jac [N,6,2])."""
        N = g.shape[0]
        g = self._flat32(g, (N, 2), 'g'); origin = self._flat32(origin, (N, 3), 'origin')
        R = self._flat32(R, (N, 3, 3), 'R'); inv_cam = self._flat32(inv_cam, (N, 4, 4), 'inv_cam')
        ppm = self._flat32(ppm, (N, 2), 'ppm')
        if kappa is not None:
            head_R = self._flat32(head_R, (N, 3, 3), 'head_R'); kappa = self._flat32(kappa, (N, 2), 'kappa')
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=g.device)
        g_out, mm, px, jac = new(N, 2), new(N, 2), new(N, 2), new(N, 6, 2)
        self._ck(self.lib.eve_gaze_to_pog(N, self._p(g), self._p(origin), self._p(R), self._p(inv_cam), self._p(ppm),
                                          self._p(head_R if kappa is not None else None), self._p(kappa), float(screen[0]),
                                          float(screen[1]), self._p(g_out), self._p(mm), self._p(px), self._p(jac), self._stream()))
        return g_out, mm, px, jac

    def gaze_to_pog_bwd(self, jac, dg_out, dmm, dpx):
        N = jac.shape[0]
        f = lambda t: None if t is None else self._flat32(t, (N, 2), 'grad')
        dg_out, dmm, dpx = f(dg_out), f(dmm), f(dpx)
        dg = torch.empty((N, 2), dtype=torch.float32, device=jac.device)
        self._ck(self.lib.eve_gaze_to_pog_bwd(N, self._p(jac), self._p(dg_out), self._p(dmm), self._p(dpx), self._p(dg), self._stream()))
        return dg

    def combined_gaze(self, origin, pog_mm, R, cam):
        N = origin.shape[0]
        origin = self._flat32(origin, (N, 3), 'origin'); pog_mm = self._flat32(pog_mm, (N, 2), 'pog_mm')
        R = self._flat32(R, (N, 3, 3), 'R'); cam = self._flat32(cam, (N, 4, 4), 'cam')
        g = torch.empty((N, 2), dtype=torch.float32, device=origin.device)
        self._ck(self.lib.eve_combined_gaze(N, self._p(origin), self._p(pog_mm), self._p(R), self._p(cam), self._p(g), self._stream()))
        return g

    def make_heatmaps(self, centres_px, sigma, hw, screen, validity=None):
        """centres [N,2] px -> [N,1,H,W] float32 (x validity[n] when given)."""
        N = centres_px.shape[0]
        c = self._flat32(centres_px, (N, 2), 'centres')
        v = None
        if validity is not None:
            v = validity.contiguous()
            v = v.view(torch.uint8) if v.dtype == torch.bool else v.to(torch.uint8)
            assert tuple(v.shape) == (N,)
        out = torch.empty((N, 1, hw[0], hw[1]), dtype=torch.float32, device=c.device)
        for i in range(0, N, 65535):
            n = min(65535, N - i)
            self._ck(self.lib.eve_make_heatmaps(n, hw[0], hw[1], self._p(c[i:i + n]), self._p(None if v is None else v[i:i + n]),
                                                float(sigma), float(screen[0]), float(screen[1]), self._p(out[i:i + n]), self._stream()))
        return out

    def make_heatmaps_bwd(self, centres_px, sigma, screen, dout):
        N, _, H, W = dout.shape
        c = self._flat32(centres_px, (N, 2), 'centres')
        dout = self._flat32(dout, (N, 1, H, W), 'dout')
        dc = torch.empty((N, 2), dtype=torch.float32, device=c.device)
        self._ck(self.lib.eve_make_heatmaps_bwd(N, H, W, self._p(c), float(sigma), float(screen[0]), float(screen[1]), self._p(dout),
                                                self._p(dc), self._stream()))
        return dc

    def soft_argmax_fwd(self, heat, screen):
        """heat [N,1,H,W] float32 -> (pog_px [N,2], stats [N,4])."""
        N, _, H, W = heat.shape
        heat = self._flat32(heat, (N, 1, H, W), 'heat')
        px = torch.empty((N, 2), dtype=torch.float32, device=heat.device)
        stats = torch.empty((N, 4), dtype=torch.float32, device=heat.device)
        self._ck(self.lib.eve_soft_argmax_fwd(N, H, W, self._p(heat), float(screen[0]), float(screen[1]), self._p(px), self._p(stats),
                                              self._stream()))
        return px, stats

    def soft_argmax_bwd(self, heat, stats, dpog, screen):
        N, _, H, W = heat.shape
        dpog = self._flat32(dpog, (N, 2), 'dpog')
        dh = torch.empty_like(heat)
        for i in range(0, N, 65535):
            n = min(65535, N - i)
            self._ck(self.lib.eve_soft_argmax_bwd(n, H, W, self._p(heat[i:i + n]), self._p(stats[i:i + n]), self._p(dpog[i:i + n]),
                                                  float(screen[0]), float(screen[1]), self._p(dh[i:i + n]), self._stream()))
        return dh

    # ------------------------------------------------------------------ RefineNet head + heat-map losses
    def heatmap_head_fwd(self, logits):
        """logits NHWC [N, H, W, Cpad] (channel 0 is the map) -> float [N, 1, H, W] = sigmoid, evaluated in float."""
        N, H, W, Cp = logits.shape
        out = torch.empty((N, 1, H, W), dtype=torch.float32, device=logits.device)
        self._ck(self.lib.eve_heatmap_head_fwd(dt_code(logits.dtype), N * H * W, Cp, self._p(logits), self._p(out),
                                               self._stream()))
        return out

    def heatmap_head_bwd(self, dy, y, dtype, cpad):
        N, _, H, W = y.shape
        dy = dy.contiguous().float()
        dl = torch.empty((N, H, W, cpad), dtype=dtype, device=y.device)
        self._ck(self.lib.eve_heatmap_head_bwd(dt_code(dtype), N * H * W, cpad, self._p(dy), self._p(y), self._p(dl),
                                               self._stream()))
        return dl

    def heatmap_loss_fwd(self, kind, pred, gt, validity):
        """kind 0 = BCE, 1 = MSE; pred, gt float [B, T, ...map...]; validity bool/uint8 [B, T].
        Returns (loss 0-dim, w [B*T] = d loss / d per-frame mean)."""
        B, T = pred.shape[:2]
        HW = pred[0, 0].numel()
        pred, gt = pred.contiguous(), gt.contiguous()
        assert pred.dtype == torch.float32 and gt.dtype == torch.float32 and gt.shape == pred.shape
        v = validity.contiguous()
        v = v.view(torch.uint8) if v.dtype == torch.bool else v.to(torch.uint8)
        assert tuple(v.shape) == (B, T)
        per_map = torch.empty((B * T,), dtype=torch.float32, device=pred.device)
        w = torch.empty((B * T,), dtype=torch.float32, device=pred.device)
        loss = torch.empty((1,), dtype=torch.float32, device=pred.device)
        self._ck(self.lib.eve_heatmap_loss_fwd(kind, B, T, HW, self._p(pred), self._p(gt), self._p(v), self._p(per_map),
                                               self._p(loss), self._p(w), self._stream()))
        return loss.view(()), w

    def heatmap_loss_bwd(self, kind, pred, gt, w, upstream):
        B, T = pred.shape[:2]
        HW = pred[0, 0].numel()
        pred, gt = pred.contiguous(), gt.contiguous()
        up = upstream.detach().float().reshape(1).contiguous()
        dp = torch.empty_like(pred)
        self._ck(self.lib.eve_heatmap_loss_bwd(kind, B * T, HW, self._p(pred), self._p(gt), self._p(w), self._p(up),
                                               self._p(dp), self._stream()))
        return dp

    # ------------------------------------------------------------------ fused train-step losses
    def eye_losses(self, g_pred, g_tgt, g_val, p_pred, p_tgt, p_val, coeff_ang, coeff_l1):
        """Each argument is a (left, right) pair.  Returns terms[5], (dg_l, dg_r), (dp_l, dp_r)."""
        B, T = p_pred[0].shape
        dev = p_pred[0].device

        def pair(ts, dtype, shape):
            out = []
            for t in ts:
                t = t.contiguous()
                if dtype == torch.uint8:
                    t = t.view(torch.uint8) if t.dtype == torch.bool else t.to(torch.uint8)
                assert t.dtype == dtype and tuple(t.shape) == shape and t.is_cuda, (t.dtype, t.shape)
                out.append(t)
            return out, (ctypes.c_void_p * 2)(*[t.data_ptr() for t in out])

        keep = []
        ptrs = []
        for ts, dt, shp in ((g_pred, torch.float32, (B, T, 2)), (g_tgt, torch.float32, (B, T, 2)), (g_val, torch.uint8, (B, T)),
                            (p_pred, torch.float32, (B, T)), (p_tgt, torch.float32, (B, T)), (p_val, torch.uint8, (B, T))):
            k_, a = pair(ts, dt, shp)
            keep.append(k_)
            ptrs.append(a)
        terms = torch.zeros((5,), dtype=torch.float32, device=dev)
        dg = [torch.empty((B, T, 2), dtype=torch.float32, device=dev) for _ in range(2)]
        dp = [torch.empty((B, T), dtype=torch.float32, device=dev) for _ in range(2)]
        dg_a = (ctypes.c_void_p * 2)(*[t.data_ptr() for t in dg])
        dp_a = (ctypes.c_void_p * 2)(*[t.data_ptr() for t in dp])
        self._ck(self.lib.eve_eye_losses(B, T, ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[5], float(coeff_ang),
                                         float(coeff_l1), self._p(terms), dg_a, dp_a, self._stream()))
        return terms, dg, dp

    # ------------------------------------------------------------------ small float32 linear layers
    def linear_fwd(self, x, w_in_out, bias, act):
        M, K = x.shape
        N = w_in_out.shape[1]
        assert x.dtype == torch.float32 and w_in_out.dtype == torch.float32 and w_in_out.shape[0] == K
        assert x.is_contiguous() and w_in_out.is_contiguous()
        y = torch.empty((M, N), dtype=torch.float32, device=x.device)
        self._ck(self.lib.eve_linear_fwd(M, K, N, self._p(x), self._p(w_in_out), self._p(self._f32(bias, 'bias')), act,
                                         self._p(y), self._stream()))
        return y

    def linear_fwd_ex(self, x, k_cols, w_in_out, bias, act, y, n_cols=None):
        """y[:, :N] = act(x[:, :K] @ w_in_out + bias): K leading columns of x, N leading columns of y (both may be wider), a bias
        with fewer than N entries covers the leading columns (the zero-padded heads)."""
        M = x.shape[0]
        K, N = w_in_out.shape
        assert k_cols == K and (n_cols is None or n_cols == N)
        for t in (x, w_in_out, y, bias):
            assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda)
        assert x.shape[1] >= K and y.shape[1] >= N and y.shape[0] == M
        self._ck(self.lib.eve_linear_fwd_ex(M, K, N, self._p(x), x.shape[1], self._p(w_in_out), self._p(bias),
                                            bias.numel() if bias is not None else 0, act, self._p(y), y.shape[1], self._stream()))
        return y

    def linear_dgrad_ex(self, dy, n_cols, y, act, w_out_in, dx, accumulate=False):
        """dx (+)= (dy[:, :N] * act'(y[:, :N])) @ w_out_in  -- dy / y may be wider than N, dx exactly K wide."""
        M = dy.shape[0]
        N, K = w_out_in.shape
        assert n_cols == N and dy.shape[1] >= N and tuple(dx.shape) == (M, K) and (y is None or y.shape == dy.shape)
        for t in (dy, y, w_out_in, dx):
            assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda)
        self._ck(self.lib.eve_linear_dgrad_ex(M, K, N, self._p(dy), dy.shape[1], self._p(y), act, self._p(w_out_in), self._p(dx), K,
                                              int(bool(accumulate)), self._stream()))
        return dx

    def tail_head_pose(self, h_left, h_right, cat, col):
        BT = h_left.numel() // 2
        for t in (h_left, h_right, cat):
            assert t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda
        assert h_right.numel() == 2 * BT and cat.shape[0] == 2 * BT and cat.shape[1] >= col + 4
        self._ck(self.lib.eve_tail_head_pose(BT, self._p(h_left), self._p(h_right), self._p(cat), cat.shape[1], col, self._stream()))

    def tail_outputs_fwd(self, g2, p2):
        M = g2.shape[0]
        assert tuple(g2.shape) == (M, 4) and tuple(p2.shape) == (M, 4) and g2.is_contiguous() and p2.is_contiguous()
        gaze = torch.empty((M, 2), dtype=torch.float32, device=g2.device)
        pupil = torch.empty((M,), dtype=torch.float32, device=g2.device)
        self._ck(self.lib.eve_tail_outputs_fwd(M, self._p(g2), self._p(p2), self._p(gaze), self._p(pupil), self._stream()))
        return gaze, pupil

    def tail_outputs_bwd(self, dg, dp, g_full, coeff_ang, coeff_l1):
        """dg / dp: the (left, right) unit gradients of eye_losses; g_full: device scalar or None -> d_g2, d_p2 [2*B*T, 4]."""
        BT = dp[0].numel()
        for t in (dg[0], dg[1], dp[0], dp[1]):
            assert t.dtype == torch.float32 and t.is_contiguous()
        assert g_full is None or (g_full.dtype == torch.float32 and g_full.numel() == 1 and g_full.is_cuda)
        d_g2 = torch.empty((2 * BT, 4), dtype=torch.float32, device=dp[0].device)
        d_p2 = torch.empty((2 * BT, 4), dtype=torch.float32, device=dp[0].device)
        self._ck(self.lib.eve_tail_outputs_bwd(BT, self._p(dg[0]), self._p(dg[1]), self._p(dp[0]), self._p(dp[1]), self._p(g_full),
                                               float(coeff_ang), float(coeff_l1), self._p(d_g2), self._p(d_p2), self._stream()))
        return d_g2, d_p2

    def linear_dgrad(self, dy, y, act, w_out_in):
        M, N = dy.shape
        K = w_out_in.shape[1]
        assert dy.dtype == torch.float32 and dy.is_contiguous() and tuple(w_out_in.shape) == (N, K)
        dx = torch.empty((M, K), dtype=torch.float32, device=dy.device)
        self._ck(self.lib.eve_linear_dgrad(M, K, N, self._p(dy), self._p(y), act, self._p(w_out_in), self._p(dx),
                                           self._stream()))
        return dx

    def linear_wgrad(self, dy, y, act, x, dw_out_in, db):
        """Accumulates into dw_out_in [N, K] (and db [N] when given)."""
        M, N = dy.shape
        K = x.shape[1]
        assert tuple(dw_out_in.shape) == (N, K) and dw_out_in.dtype == torch.float32 and dw_out_in.is_contiguous()
        assert x.is_contiguous() and dy.is_contiguous() and (db is None or (db.numel() == N and db.is_contiguous()))
        self._ck(self.lib.eve_linear_wgrad(M, K, N, self._p(dy), self._p(y), act, self._p(x), self._p(dw_out_in),
                                           self._p(db), self._stream()))

    def bias_grad(self, dy, db):
        C = dy.shape[-1]
        M = dy.numel() // C
        assert db.dtype == torch.float32 and db.numel() == C
        self._ck(self.lib.eve_bias_grad(dt_code(dy.dtype), M, C, self._p(dy), self._p(db), self._stream()))
        return db

    # ------------------------------------------------------------------ instance norm
    def instnorm_stats(self, x, eps=1e-5):
        N, H, W, C = x.shape
        mr = torch.empty((N, C, 2), dtype=torch.float32, device=x.device)
        self._timed('in_stats', 0.0, lambda: self._ck(self.lib.eve_instnorm_stats(
            dt_code(x.dtype), N, H * W, C, self._p(x), eps, self._p(mr), self._stream())), (x,))
        return mr

    def instnorm_act_fwd(self, x, mr, gamma, beta, res, act):
        N, H, W, C = x.shape
        y = torch.empty_like(x)
        self._timed('in_fwd', 0.0, lambda: self._ck(self.lib.eve_instnorm_act_fwd(
            dt_code(x.dtype), N, H * W, C, self._p(x), self._p(mr), self._p(self._f32(gamma, 'gamma')),
            self._p(self._f32(beta, 'beta')), self._p(res), act, self._p(y), self._stream())), (x, res, y))
        return y

    def instnorm_act_bwd(self, dy, y, x, mr, gamma, act, want_dres, beta=None, dx_add=None):
        """y may be None when the forward had no residual (beta is then needed next to gamma)."""
        N, H, W, C = x.shape
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if want_dres else None
        sums = torch.empty((N, C, 2), dtype=torch.float32, device=x.device)
        # two passes over (dy, x[, y]) -- the reductions, then the gradient -- are this kernel's algorithmic traffic
        self._timed('in_bwd', 0.0, lambda: self._ck(self.lib.eve_instnorm_act_bwd(
            dt_code(x.dtype), N, H * W, C, self._p(dy), self._p(y), self._p(x), self._p(mr),
            self._p(self._f32(gamma, 'gamma')), self._p(self._f32(beta, 'beta')), act, self._p(dx), self._p(dres),
            self._p(sums), self._p(dx_add), self._stream())), (dy, x, y, dy, x, y, dx, dres, dx_add))
        return dx, dres, sums

    def instnorm_act2_fwd(self, xs, mrs, gamma_a, beta_a, gamma_b, beta_b, act):
        """Two heads act(gamma_h * xhat + beta_h) of the channel-concatenation of the 1-2 NHWC sources `xs` (statistics
        `mrs` per source); returns (y_a, y_b), [N, H, W, sum C].  gamma_b / beta_b None: one head, y_b None."""
        x, x2 = xs[0], (xs[1] if len(xs) > 1 else None)
        N, H, W, C = x.shape
        C2 = x2.shape[-1] if x2 is not None else 0
        y_a = torch.empty((N, H, W, C + C2), dtype=x.dtype, device=x.device)
        y_b = torch.empty_like(y_a) if gamma_b is not None else None
        self._timed('in_fwd', 0.0, lambda: self._ck(self.lib.eve_instnorm_act2_fwd(
            dt_code(x.dtype), N, H * W, C, self._p(x), self._p(mrs[0]), self._p(self._f32(gamma_a, 'gamma')),
            self._p(self._f32(beta_a, 'beta')), self._p(self._f32(gamma_b, 'gamma')), self._p(self._f32(beta_b, 'beta')), act,
            self._p(y_a), self._p(y_b), C + C2, C2, self._p(x2), self._p(mrs[1] if x2 is not None else None), self._stream())),
            (x, x2, y_a, y_b))
        return y_a, y_b

    def instnorm_act2_bwd(self, dy_a, dy_b, xs, mrs, gamma_a, beta_a, gamma_b, beta_b, act):
        """Backward of instnorm_act2_fwd: dy_a / dy_b [N, H, W, sum C] (dy_b None with one head).
        Returns ([dx per source], sums_a, sums_b) with sums [N, sum C, 2]."""
        x, x2 = xs[0], (xs[1] if len(xs) > 1 else None)
        N, H, W, C = x.shape
        C2 = x2.shape[-1] if x2 is not None else 0
        assert dy_a.shape[-1] == C + C2
        dx = torch.empty_like(x)
        dx2 = torch.empty_like(x2) if x2 is not None else None
        sums_a = torch.empty((N, C + C2, 2), dtype=torch.float32, device=x.device)
        sums_b = torch.empty_like(sums_a) if dy_b is not None else None
        # two passes over (dy_a, dy_b, x), then the gradient: this kernel's algorithmic traffic
        self._timed('in_bwd', 0.0, lambda: self._ck(self.lib.eve_instnorm_act2_bwd(
            dt_code(x.dtype), N, H * W, C, self._p(dy_a), self._p(dy_b), C + C2, self._p(x), self._p(mrs[0]),
            self._p(self._f32(gamma_a, 'gamma')), self._p(self._f32(beta_a, 'beta')), self._p(self._f32(gamma_b, 'gamma')),
            self._p(self._f32(beta_b, 'beta')), act, self._p(dx), self._p(sums_a), self._p(sums_b), C2, self._p(x2),
            self._p(mrs[1] if x2 is not None else None), self._p(dx2), self._stream())),
            (dy_a, dy_b, x, x2, dy_a, dy_b, x, x2, dx, dx2))
        return ([dx] if x2 is None else [dx, dx2]), sums_a, sums_b

    def instnorm_fwd_fused(self, x, gamma, beta, res, act, eps=1e-5, want_mask=False):
        """Single-launch stats + apply; returns (y, mean_rstd) or None when the plane is too large.
        want_mask: also the sign mask of y (one byte per 16-byte vector) -> (y, mean_rstd, mask)."""
        N, H, W, C = x.shape
        y = torch.empty_like(x)
        mr = torch.empty((N, C, 2), dtype=torch.float32, device=x.device)
        mask = torch.empty((x.numel() * x.element_size() // 16,), dtype=torch.uint8, device=x.device) if want_mask else None
        st = self._timed('in_fwd', 0.0, lambda: self.lib.eve_instnorm_fwd_fused(
            dt_code(x.dtype), N, H * W, C, self._p(x), self._p(self._f32(gamma, 'gamma')), self._p(self._f32(beta, 'beta')),
            self._p(res), act, eps, self._p(y), self._p(mr), self._p(mask), self._stream()), (x, res, y, mask))
        if st == -1:
            if self.prof:
                self.prof.pop()          # nothing was launched
            return None
        self._ck(st)
        return (y, mr, mask) if want_mask else (y, mr)

    def instnorm_bwd_fused(self, dy, y, x, mr, gamma, act, want_dres, dy2=None, mask=None, beta=None, dx_add=None):
        """Single-launch backward; returns (dx, dres, sums) or None when the plane is too large.
        dy2: optional second summand of the incoming gradient (added on load).
        beta: with gamma and y = None (no residual), act' is recomputed from x with the forward's scale / shift.
        mask: the forward's sign mask (ReLU only), read instead of y."""
        N, H, W, C = x.shape
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if want_dres else None
        sums = torch.empty((N, C, 2), dtype=torch.float32, device=x.device)
        st = self._timed('in_bwd', 0.0, lambda: self.lib.eve_instnorm_bwd_fused(
            dt_code(x.dtype), N, H * W, C, self._p(dy), self._p(dy2), self._p(None if mask is not None else y), self._p(x), self._p(mr),
            self._p(self._f32(gamma, 'gamma')), self._p(self._f32(beta, 'beta')), act, self._p(dx), self._p(dres), self._p(sums), self._p(mask),
            self._p(dx_add), self._stream()), (dy, dy2, y if mask is None else mask, x, dx, dres, dx_add))
        if st == -1:
            if self.prof:
                self.prof.pop()
            return None
        self._ck(st)
        return dx, dres, sums

    def sum_rows(self, t):
        """[N, ...] float32 -> [...]: the sum over the leading dimension in a fixed order (per-plane partials -> parameter gradient)."""
        assert t.dtype == torch.float32 and t.is_contiguous()
        out = torch.empty(t.shape[1:], dtype=torch.float32, device=t.device)
        self._ck(self.lib.eve_sum_rows(t.shape[0], out.numel(), self._p(t), self._p(out), self._stream()))
        return out

    def sum_rows_pairs(self, sums, out0, out1):
        """sums [N, C, 2] float32: out0 += sums[:, :, 0].sum(0), out1 += sums[:, :, 1].sum(0), fixed order, in place (contiguous
        float32 [C] vectors: an affine InstanceNorm's d beta / d gamma inside the flat gradient buffer)."""
        N, C, two = sums.shape
        assert two == 2 and sums.dtype == torch.float32 and sums.is_contiguous()
        for o in (out0, out1):
            assert o.dtype == torch.float32 and o.is_contiguous() and o.numel() == C
        self._ck(self.lib.eve_sum_rows_pairs(N, C, self._p(sums), self._p(out0), self._p(out1), self._stream()))

    # ------------------------------------------------------------------ element-wise
    def act_bwd(self, dy, y, act):
        dx = torch.empty_like(dy)
        self._ck(self.lib.eve_act_bwd(dt_code(dy.dtype), dy.numel(), self._p(dy), self._p(y), act,
                                      self._p(dx), self._stream()))
        return dx

    def add(self, a, b):
        out = torch.empty_like(a)
        self._ck(self.lib.eve_add(dt_code(a.dtype), a.numel(), self._p(a), self._p(b), self._p(out),
                                  self._stream()))
        return out

    # ------------------------------------------------------------------ pooling / resampling
    def maxpool3x3s2_fwd(self, x):
        N, IH, IW, C = x.shape
        OH, OW = (IH - 1) // 2 + 1, (IW - 1) // 2 + 1
        y = torch.empty((N, OH, OW, C), dtype=x.dtype, device=x.device)
        idx = torch.empty((N, OH, OW, C), dtype=torch.uint8, device=x.device)
        self._ck(self.lib.eve_maxpool3x3s2_fwd(dt_code(x.dtype), N, IH, IW, C, self._p(x), self._p(y),
                                               self._p(idx), self._stream()))
        return y, idx

    def maxpool3x3s2_bwd(self, dy, idx, in_hw):
        N, OH, OW, C = dy.shape
        IH, IW = in_hw
        dx = torch.empty((N, IH, IW, C), dtype=dy.dtype, device=dy.device)
        self._ck(self.lib.eve_maxpool3x3s2_bwd(dt_code(dy.dtype), N, IH, IW, C, self._p(dy), self._p(idx),
                                               self._p(dx), self._stream()))
        return dx

    def in_relu_maxpool_fwd(self, x, mr):
        N, IH, IW, C = x.shape
        OH, OW = (IH - 1) // 2 + 1, (IW - 1) // 2 + 1
        y = torch.empty((N, OH, OW, C), dtype=x.dtype, device=x.device)
        idx = torch.empty((N, OH, OW, C), dtype=torch.uint8, device=x.device)
        self._ck(self.lib.eve_in_relu_maxpool_fwd(dt_code(x.dtype), N, IH, IW, C, self._p(x), self._p(mr),
                                                  self._p(y), self._p(idx), self._stream()))
        return y, idx

    def in_relu_maxpool_bwd(self, dy_pool, y_pool, idx, x, mr):
        N, IH, IW, C = x.shape
        dx = torch.empty_like(x)
        self._ck(self.lib.eve_in_relu_maxpool_bwd(dt_code(x.dtype), N, IH, IW, C, self._p(dy_pool), self._p(y_pool),
                                                  self._p(idx), self._p(x), self._p(mr), self._p(dx),
                                                  self._stream()))
        return dx

    def avgpool_fwd(self, x):
        N, H, W, C = x.shape
        y = torch.empty((N, C), dtype=x.dtype, device=x.device)
        self._ck(self.lib.eve_avgpool_fwd(dt_code(x.dtype), N, H * W, C, self._p(x), self._p(y),
                                          self._stream()))
        return y

    def avgpool_fwd_f32(self, x):
        """avgpool_fwd with a float32 result holding the x.dtype-rounded means (= avgpool_fwd + cast, one launch)."""
        N, H, W, C = x.shape
        y = torch.empty((N, C), dtype=torch.float32, device=x.device)
        self._ck(self.lib.eve_avgpool_fwd_f32(dt_code(x.dtype), N, H * W, C, self._p(x), self._p(y), self._stream()))
        return y

    def avgpool_bwd_f32(self, dy, hw, dtype):
        """dy float32 [N, C] -> dx [N, H, W, C] in `dtype` (= cast + avgpool_bwd, one launch)."""
        N, C = dy.shape
        assert dy.dtype == torch.float32 and dy.is_contiguous()
        dx = torch.empty((N, hw[0], hw[1], C), dtype=dtype, device=dy.device)
        self._ck(self.lib.eve_avgpool_bwd_f32(dt_code(dtype), N, hw[0] * hw[1], C, self._p(dy), self._p(dx), self._stream()))
        return dx

    def avgpool_bwd(self, dy, hw):
        N, C = dy.shape
        dx = torch.empty((N, hw[0], hw[1], C), dtype=dy.dtype, device=dy.device)
        self._ck(self.lib.eve_avgpool_bwd(dt_code(dy.dtype), N, hw[0] * hw[1], C, self._p(dy), self._p(dx),
                                          self._stream()))
        return dx

    def adaptive_maxpool_fwd(self, x, out_hw):
        N, IH, IW, C = x.shape
        OH, OW = out_hw
        y = torch.empty((N, OH, OW, C), dtype=x.dtype, device=x.device)
        idx = torch.empty((N, OH, OW, C), dtype=torch.int32, device=x.device)
        self._ck(self.lib.eve_adaptive_maxpool_fwd(dt_code(x.dtype), N, IH, IW, OH, OW, C, self._p(x),
                                                   self._p(y), self._p(idx), self._stream()))
        return y, idx

    def adaptive_maxpool_bwd(self, dy, idx, in_hw, add=None):
        """add: a second gradient of the pool's input ([N, IH, IW, C]), summed in the kernel epilogue."""
        N, OH, OW, C = dy.shape
        IH, IW = in_hw
        dx = torch.empty((N, IH, IW, C), dtype=dy.dtype, device=dy.device)
        assert add is None or (tuple(add.shape) == (N, IH, IW, C) and add.dtype == dy.dtype)
        self._ck(self.lib.eve_adaptive_maxpool_bwd(dt_code(dy.dtype), N, IH, IW, OH, OW, C, self._p(dy),
                                                   self._p(idx), self._p(add), self._p(dx), self._stream()))
        return dx

    def bilinear_fwd(self, x, out_hw):
        N, IH, IW, C = x.shape
        OH, OW = out_hw
        y = torch.empty((N, OH, OW, C), dtype=x.dtype, device=x.device)
        self._ck(self.lib.eve_bilinear_fwd(dt_code(x.dtype), N, IH, IW, OH, OW, C, self._p(x), self._p(y),
                                           self._stream()))
        return y

    def bilinear_bwd(self, dy, in_hw):
        N, OH, OW, C = dy.shape
        IH, IW = in_hw
        dx = torch.empty((N, IH, IW, C), dtype=dy.dtype, device=dy.device)
        self._ck(self.lib.eve_bilinear_bwd(dt_code(dy.dtype), N, IH, IW, OH, OW, C, self._p(dy), self._p(dx),
                                           self._stream()))
        return dx

    # ------------------------------------------------------------------ layout / dtype
    def nchw_to_nhwc(self, src, dtype, cpad=None, out=None):
        N, C, H, W = src.shape
        cpad = cpad or pad_channels(C, dtype)
        src = src.contiguous()
        dst = out if out is not None else torch.empty((N, H, W, cpad), dtype=dtype, device=src.device)
        assert tuple(dst.shape) == (N, H, W, cpad) and dst.dtype == dtype
        self._ck(self.lib.eve_nchw_to_nhwc(dt_code(dtype), N, C, H, W, cpad, self._p(self._f32(src, 'src')),
                                           self._p(dst), self._stream()))
        return dst

    def nhwc_to_nchw(self, src, C):
        N, H, W, cpad = src.shape
        dst = torch.empty((N, C, H, W), dtype=torch.float32, device=src.device)
        self._ck(self.lib.eve_nhwc_to_nchw(dt_code(src.dtype), N, C, H, W, cpad, self._p(src), self._p(dst),
                                           self._stream()))
        return dst

    def cast(self, src, dtype):
        if src.dtype == dtype:
            return src
        dst = torch.empty(src.shape, dtype=dtype, device=src.device)
        self._ck(self.lib.eve_cast(dt_code(src.dtype), dt_code(dtype), src.numel(), self._p(src), self._p(dst),
                                   self._stream()))
        return dst

    def pack_weights(self, w_ohwi_f32, dtype, want_ihwo=True):
        Cout, KH, KW, Cin = w_ohwi_f32.shape
        ohwi = torch.empty((Cout, KH, KW, Cin), dtype=dtype, device=w_ohwi_f32.device)
        ihwo = torch.empty((Cin, KH, KW, Cout), dtype=dtype, device=w_ohwi_f32.device) if want_ihwo else None
        self._ck(self.lib.eve_pack_weights(dt_code(dtype), Cout, KH * KW, Cin,
                                           self._p(self._f32(w_ohwi_f32, 'weights')), self._p(ohwi),
                                           self._p(ihwo), self._stream()))
        return ohwi, ihwo

    def pack_weights_batch(self, ws_ohwi_f32, dtype, want_ihwo, padded=None):
        """pack_weights for a list of OHWI float32 weights (and per-weight want_ihwo flags) in ONE launch per
        EVE_PACK_BATCH_MAX weights.  padded: per weight None or (Cout_padded, Cin_padded) -- the packed copies are that wide, the
        extra channels zero (written by the same launch).  Returns [(ohwi, ihwo)]."""
        out, items, keep = [], [], []
        padded = padded if padded is not None else [None] * len(ws_ohwi_f32)
        for w, wi, pd in zip(ws_ohwi_f32, want_ihwo, padded):
            sCout, KH, KW, sCin = w.shape
            Cout, Cin = pd if pd is not None else (sCout, sCin)
            assert Cout >= sCout and Cin >= sCin
            w = self._f32(w, 'weights')
            self._p(w)                                 # (raises for a tensor that is not on the GPU)
            ohwi = torch.empty((Cout, KH, KW, Cin), dtype=dtype, device=w.device)
            ihwo = torch.empty((Cin, KH, KW, Cout), dtype=dtype, device=w.device) if wi else None
            keep.append(w)
            items.append(_lib.PackItem(w.data_ptr(), ohwi.data_ptr(), ihwo.data_ptr() if wi else None, Cout, KH * KW, Cin, sCout, sCin))
            out.append((ohwi, ihwo))
        for i in range(0, len(items), _lib.PACK_BATCH_MAX):
            chunk = items[i:i + _lib.PACK_BATCH_MAX]
            arr = (_lib.PackItem * len(chunk))(*chunk)
            self._ck(self.lib.eve_pack_weights_batch(dt_code(dtype), len(chunk), arr, self._stream()))
        return out

    # ------------------------------------------------------------------ recurrent
    def gru_scan_fwd(self, gi, whh_t, bhh, h0):
        S, T, H3 = gi.shape
        H = H3 // 3
        dev = gi.device
        hs = torch.empty((S, T, H), dtype=torch.float32, device=dev)
        gates = torch.empty((S, T, H3), dtype=torch.float32, device=dev)
        hn_pre = torch.empty((S, T, H), dtype=torch.float32, device=dev)
        self._ck(self.lib.eve_gru_scan_fwd(S, T, H, self._p(self._f32(gi, 'gi')), self._p(whh_t), self._p(bhh),
                                           self._p(h0), self._p(hs), self._p(gates), self._p(hn_pre),
                                           self._stream()))
        return hs, gates, hn_pre

    def gru_scan_bwd(self, dhs, whh, h0, hs, gates, hn_pre, want_dh0):
        S, T, H = dhs.shape
        dev = dhs.device
        dgi = torch.empty((S, T, 3 * H), dtype=torch.float32, device=dev)
        dgh = torch.empty((S, T, 3 * H), dtype=torch.float32, device=dev)
        dh0 = torch.empty((S, H), dtype=torch.float32, device=dev) if want_dh0 else None
        self._ck(self.lib.eve_gru_scan_bwd(S, T, H, self._p(dhs), self._p(whh), self._p(h0), self._p(hs),
                                           self._p(gates), self._p(hn_pre), self._p(dgi), self._p(dgh),
                                           self._p(dh0), self._stream()))
        return dgi, dgh, dh0

    def rnn_scan_fwd(self, gi, whh_t, bhh, h0):
        S, T, H = gi.shape
        hs = torch.empty((S, T, H), dtype=torch.float32, device=gi.device)
        self._ck(self.lib.eve_rnn_scan_fwd(S, T, H, self._p(self._f32(gi, 'gi')), self._p(whh_t), self._p(bhh), self._p(h0),
                                           self._p(hs), self._stream()))
        return hs

    def rnn_scan_bwd(self, dhs, whh, hs, want_dh0):
        S, T, H = dhs.shape
        dpre = torch.empty((S, T, H), dtype=torch.float32, device=dhs.device)
        dh0 = torch.empty((S, H), dtype=torch.float32, device=dhs.device) if want_dh0 else None
        self._ck(self.lib.eve_rnn_scan_bwd(S, T, H, self._p(dhs), self._p(whh), self._p(hs), self._p(dpre), self._p(dh0),
                                           self._stream()))
        return dpre, dh0

    def lstm_scan_fwd(self, gi, whh_t, bhh, h0, c0):
        S, T, H4 = gi.shape
        H = H4 // 4
        dev = gi.device
        hs = torch.empty((S, T, H), dtype=torch.float32, device=dev)
        cs = torch.empty((S, T, H), dtype=torch.float32, device=dev)
        gates = torch.empty((S, T, H4), dtype=torch.float32, device=dev)
        self._ck(self.lib.eve_lstm_scan_fwd(S, T, H, self._p(self._f32(gi, 'gi')), self._p(whh_t), self._p(bhh), self._p(h0),
                                            self._p(c0), self._p(hs), self._p(cs), self._p(gates), self._stream()))
        return hs, cs, gates

    def lstm_scan_bwd(self, dhs, dcs, whh, c0, hs, cs, gates, want_d0):
        S, T, H = dhs.shape
        dev = dhs.device
        dpre = torch.empty((S, T, 4 * H), dtype=torch.float32, device=dev)
        dh0 = torch.empty((S, H), dtype=torch.float32, device=dev) if want_d0 else None
        dc0 = torch.empty((S, H), dtype=torch.float32, device=dev) if want_d0 else None
        self._ck(self.lib.eve_lstm_scan_bwd(S, T, H, self._p(dhs), self._p(dcs), self._p(whh), self._p(c0), self._p(hs),
                                            self._p(cs), self._p(gates), self._p(dpre), self._p(dh0), self._p(dc0),
                                            self._stream()))
        return dpre, dh0, dc0

    def cgru_scan_fwd(self, xs, h0, w1_ohwi, b1, w2_ohwi, b2):
        """CGRUCell over T in one launch.  xs [B, T, 5, 8, C] bf16 / fp16 / float32 -> hs [B, T, 5, 8, C] and, time-major
        [T, B, 5, 8, .] for the backward: hs_tm, ru, rh, og.  (C in SCAN_WIDTHS; float32 and the 16-bit formats at C = 32 / 128:
        csrc/cell_scan_f32.hip.)"""
        B, T, H, W, C = xs.shape
        assert (H, W) == (5, 8) and xs.dtype in HALF_DTYPES + (torch.float32,) and xs.is_contiguous()
        assert w1_ohwi.dtype == w2_ohwi.dtype == xs.dtype and w1_ohwi.is_contiguous() and w2_ohwi.is_contiguous()
        assert tuple(w1_ohwi.shape) == (2 * C, 3, 3, 2 * C) and tuple(w2_ohwi.shape) == (C, 3, 3, 2 * C)
        dev = xs.device
        hdt = xs.dtype
        hs = torch.empty((B, T, H, W, C), dtype=hdt, device=dev)
        hs_tm = torch.empty((T, B, H, W, C), dtype=hdt, device=dev)
        ru = torch.empty((T, B, H, W, 2 * C), dtype=hdt, device=dev)
        rh = torch.empty((T, B, H, W, C), dtype=hdt, device=dev)
        og = torch.empty((T, B, H, W, C), dtype=hdt, device=dev)
        self._ck(self.lib.eve_cgru_scan_fwd_c(dt_code(hdt), B, T, C, self._p(xs), self._p(h0), self._p(w1_ohwi), self._p(self._f32(b1, 'b1')),
                                            self._p(w2_ohwi), self._p(self._f32(b2, 'b2')), self._p(hs), self._p(hs_tm),
                                            self._p(ru), self._p(rh), self._p(og), self._stream()))
        return hs, hs_tm, ru, rh, og

    def cgru_scan_bwd(self, dhs_tm, ru, og, hs_tm, h0, w1_ihwo, w2_ihwo, want_dh0=False):
        """Backward of cgru_scan_fwd in one launch.  Time-major [T, B, 5, 8, .] inputs (16-bit or float32); returns (dg1_all
        [T,B,5,8,2C], dg2_all [T,B,5,8,C], dxs_tm [T,B,5,8,C], dh0 [B,5,8,C] or None)."""
        T, B, H, W, C = dhs_tm.shape
        assert (H, W) == (5, 8) and dhs_tm.dtype in HALF_DTYPES + (torch.float32,) and dhs_tm.is_contiguous()
        assert w1_ihwo.dtype == w2_ihwo.dtype == dhs_tm.dtype and w1_ihwo.is_contiguous() and w2_ihwo.is_contiguous()
        assert all(t.is_contiguous() and t.dtype == dhs_tm.dtype for t in (ru, og, hs_tm))
        assert tuple(ru.shape) == (T, B, H, W, 2 * C) and tuple(og.shape) == tuple(hs_tm.shape) == (T, B, H, W, C)
        assert tuple(w1_ihwo.shape) == (2 * C, 3, 3, 2 * C) and tuple(w2_ihwo.shape) == (2 * C, 3, 3, C)
        dev = dhs_tm.device
        hdt = dhs_tm.dtype
        dg1 = torch.empty((T, B, H, W, 2 * C), dtype=hdt, device=dev)
        dg2 = torch.empty((T, B, H, W, C), dtype=hdt, device=dev)
        dxs = torch.empty((T, B, H, W, C), dtype=hdt, device=dev)
        dh0 = torch.empty((B, H, W, C), dtype=hdt, device=dev) if want_dh0 else None
        self._ck(self.lib.eve_cgru_scan_bwd_c(dt_code(hdt), B, T, C, self._p(dhs_tm), self._p(ru), self._p(og), self._p(hs_tm), self._p(h0),
                                            self._p(w1_ihwo), self._p(w2_ihwo), self._p(dg1), self._p(dg2), self._p(dxs),
                                            self._p(dh0), self._stream()))
        return dg1, dg2, dxs, dh0

    def crnn_scan_fwd(self, xs, h0, w_ohwi, bias):
        """CRNNCell over T in one launch (float32, csrc/cell_scan_f32.hip).  xs [B, T, 5, 8, C] -> (hs [B, T, 5, 8, C], hs_tm
        [T, B, 5, 8, C]), C in SCAN_WIDTHS."""
        B, T, H, W, C = xs.shape
        assert (H, W) == (5, 8) and xs.dtype == torch.float32 and xs.is_contiguous()
        assert tuple(w_ohwi.shape) == (C, 3, 3, 2 * C) and w_ohwi.dtype == torch.float32 and w_ohwi.is_contiguous()
        assert h0 is None or (h0.dtype == torch.float32 and h0.is_contiguous() and tuple(h0.shape) == (B, H, W, C))
        hs = torch.empty((B, T, H, W, C), dtype=torch.float32, device=xs.device)
        hs_tm = torch.empty((T, B, H, W, C), dtype=torch.float32, device=xs.device)
        self._ck(self.lib.eve_crnn_scan_fwd_c(B, T, C, self._p(xs), self._p(h0), self._p(w_ohwi), self._p(self._f32(bias, 'bias')),
                                            self._p(hs), self._p(hs_tm), self._stream()))
        return hs, hs_tm

    def crnn_scan_bwd(self, dhs_tm, hs_tm, w_ihwo, want_dh0=False):
        """Backward of crnn_scan_fwd in one launch: (dpre_all, dxs_tm [T, B, 5, 8, C], dh0 [B, 5, 8, C] or None)."""
        T, B, H, W, C = dhs_tm.shape
        assert (H, W) == (5, 8) and dhs_tm.dtype == hs_tm.dtype == torch.float32
        assert dhs_tm.is_contiguous() and hs_tm.is_contiguous() and tuple(hs_tm.shape) == (T, B, H, W, C)
        assert tuple(w_ihwo.shape) == (2 * C, 3, 3, C) and w_ihwo.dtype == torch.float32 and w_ihwo.is_contiguous()
        dpre = torch.empty((T, B, H, W, C), dtype=torch.float32, device=dhs_tm.device)
        dxs = torch.empty((T, B, H, W, C), dtype=torch.float32, device=dhs_tm.device)
        dh0 = torch.empty((B, H, W, C), dtype=torch.float32, device=dhs_tm.device) if want_dh0 else None
        self._ck(self.lib.eve_crnn_scan_bwd_c(B, T, C, self._p(dhs_tm), self._p(hs_tm), self._p(w_ihwo), self._p(dpre), self._p(dxs),
                                            self._p(dh0), self._stream()))
        return dpre, dxs, dh0

    def clstm_scan_fwd(self, xs, h0, c0, w_ohwi, bias):
        """CLSTMCell over T in one launch (float32, forward only).  xs [B, T, 5, 8, C] -> (hs, cs) [B, T, 5, 8, C], C in SCAN_WIDTHS."""
        B, T, H, W, C = xs.shape
        assert (H, W) == (5, 8) and xs.dtype == torch.float32 and xs.is_contiguous()
        assert tuple(w_ohwi.shape) == (4 * C, 3, 3, 2 * C) and w_ohwi.dtype == torch.float32 and w_ohwi.is_contiguous()
        for s0 in (h0, c0):
            assert s0 is None or (s0.dtype == torch.float32 and s0.is_contiguous() and tuple(s0.shape) == (B, H, W, C))
        hs = torch.empty((B, T, H, W, C), dtype=torch.float32, device=xs.device)
        cs = torch.empty((B, T, H, W, C), dtype=torch.float32, device=xs.device)
        self._ck(self.lib.eve_clstm_scan_fwd_c(B, T, C, self._p(xs), self._p(h0), self._p(c0), self._p(w_ohwi),
                                             self._p(self._f32(bias, 'bias')), self._p(hs), self._p(cs), self._stream()))
        return hs, cs

    def clstm_scan_fwd_train(self, xs, h0, c0, w_ohwi, bias):
        """clstm_scan_fwd for a cell that trains: the same (hs, cs), plus the time-major tensors clstm_scan_bwd reads --
        gates_tm [T, B, 5, 8, 4C] (post-activation, in / forget / out / cell), cs_tm, hs_tm [T, B, 5, 8, C]."""
        B, T, H, W, C = xs.shape
        assert (H, W) == (5, 8) and xs.dtype == torch.float32 and xs.is_contiguous()
        assert tuple(w_ohwi.shape) == (4 * C, 3, 3, 2 * C) and w_ohwi.dtype == torch.float32 and w_ohwi.is_contiguous()
        for s0 in (h0, c0):
            assert s0 is None or (s0.dtype == torch.float32 and s0.is_contiguous() and tuple(s0.shape) == (B, H, W, C))
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=xs.device)
        hs, cs = new(B, T, H, W, C), new(B, T, H, W, C)
        gates_tm, cs_tm, hs_tm = new(T, B, H, W, 4 * C), new(T, B, H, W, C), new(T, B, H, W, C)
        self._ck(self.lib.eve_clstm_scan_fwd_train_c(B, T, C, self._p(xs), self._p(h0), self._p(c0), self._p(w_ohwi),
                                                   self._p(self._f32(bias, 'bias')), self._p(hs), self._p(cs), self._p(gates_tm),
                                                   self._p(cs_tm), self._p(hs_tm), self._stream()))
        return hs, cs, gates_tm, cs_tm, hs_tm

    def clstm_scan_bwd(self, dhs_tm, dcs_tm, gates_tm, cs_tm, c0, w_ihwo, want_d0=False):
        """Backward of clstm_scan_fwd_train in one launch.  dhs_tm [T, B, 5, 8, C]; dcs_tm likewise or None (no gradient reached
        the stored cell states); w_ihwo [2C, 3, 3, 4C].  -> (dpre_all [T, B, 5, 8, 4C], dxs_tm [T, B, 5, 8, C], dh0, dc0
        [B, 5, 8, C] or None)."""
        T, B, H, W, C = dhs_tm.shape
        assert (H, W) == (5, 8)
        for t, ch in ((dhs_tm, C), (dcs_tm, C), (gates_tm, 4 * C), (cs_tm, C)):
            assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (T, B, H, W, ch))
        assert c0 is None or (c0.dtype == torch.float32 and c0.is_contiguous() and tuple(c0.shape) == (B, H, W, C))
        assert tuple(w_ihwo.shape) == (2 * C, 3, 3, 4 * C) and w_ihwo.dtype == torch.float32 and w_ihwo.is_contiguous()
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dhs_tm.device)
        dpre, dxs = new(T, B, H, W, 4 * C), new(T, B, H, W, C)
        dh0, dc0 = (new(B, H, W, C), new(B, H, W, C)) if want_d0 else (None, None)
        self._ck(self.lib.eve_clstm_scan_bwd_c(B, T, C, self._p(dhs_tm), self._p(dcs_tm), self._p(gates_tm), self._p(cs_tm),
                                             self._p(c0), self._p(w_ihwo), self._p(dpre), self._p(dxs), self._p(dh0), self._p(dc0),
                                             self._stream()))
        return dpre, dxs, dh0, dc0

    # ------------------------------------------------------------------ streaming inference (eve_amd/stream.py)
    def eye_tail_stream_fwd(self, feats, head_pose, weights, h, reset=None, want_hs=False):
        """The EyeNet tail forward in one launch with the GRU state `h` [S, 128] float32 read and overwritten in place.
        feats [S*T, 512] float32 (sequence-major), head_pose [S*T, 2]; weights: the 17 float32 tensors of eve_eye_tail_weights in
        field order; reset: int32 [S] or None.  -> gaze [S, T, 2], pupil [S, T], hs [S, T, 128] or None."""
        return self._eye_tail_stream(feats, head_pose, weights, h, reset, None, want_hs)

    def eye_tail_stream_fwd_len(self, feats, head_pose, weights, h, lengths, reset=None, want_hs=False):
        """eye_tail_stream_fwd for a ragged chunk: lengths int32 [>= S] on the device; `h[s]` becomes the state after frame
        lengths[s] - 1 (kept for a length of 0, zeroed where reset).  The outputs at t >= lengths[s] are unspecified."""
        assert lengths is not None and lengths.dtype == torch.int32 and lengths.is_contiguous() and lengths.is_cuda
        assert lengths.numel() >= h.shape[0]
        return self._eye_tail_stream(feats, head_pose, weights, h, reset, lengths, want_hs)

    def _eye_tail_stream(self, feats, head_pose, weights, h, reset, lengths, want_hs):
        S = h.shape[0]
        M = feats.shape[0]
        T = M // S
        assert tuple(h.shape) == (S, 128) and M == S * T and tuple(feats.shape) == (M, 512) and tuple(head_pose.shape) == (M, 2)
        for t in (feats, head_pose, h) + tuple(weights):
            assert t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda
        assert reset is None or (reset.dtype == torch.int32 and reset.is_contiguous() and reset.numel() >= S)
        assert len(weights) == len(_lib.EyeTailWeights._fields_)
        w = _lib.EyeTailWeights(*[t.data_ptr() for t in weights])
        dev = feats.device
        gaze = torch.empty((S, T, 2), dtype=torch.float32, device=dev)
        pupil = torch.empty((S, T), dtype=torch.float32, device=dev)
        hs = torch.empty((S, T, 128), dtype=torch.float32, device=dev) if want_hs else None
        if lengths is None:
            self._ck(self.lib.eve_eye_tail_stream_fwd(S, T, self._p(feats), self._p(head_pose), ctypes.byref(w), self._p(h),
                                                      self._p(reset), self._p(gaze), self._p(pupil), self._p(hs), self._stream()))
        else:
            self._ck(self.lib.eve_eye_tail_stream_fwd_len(S, T, self._p(feats), self._p(head_pose), ctypes.byref(w), self._p(h),
                                                          self._p(reset), self._p(lengths), self._p(gaze), self._p(pupil),
                                                          self._p(hs), self._stream()))
        return gaze, pupil, hs

    def stream_state_rows(self, src, dst, reset=None):
        """dst[s] = 0 where reset[s] != 0, else src[s], for the S rows (dim 0) of two same-shape tensors whose rows are contiguous
        (row strides may differ: `src` may be the last frame of a [S, T, ...] scan output).  In place when src is dst."""
        S = dst.shape[0]
        assert tuple(src.shape) == tuple(dst.shape) and src.dtype == dst.dtype and src.is_cuda and dst.is_cuda
        row = dst[0].numel() if S else 0
        for t in (src, dst):
            assert t[0].is_contiguous() and (S == 1 or t.stride(0) >= row), 'stream_state_rows: rows must be contiguous'
        assert reset is None or (reset.dtype == torch.int32 and reset.is_contiguous() and reset.numel() >= S and reset.is_cuda)
        self._ck(self.lib.eve_stream_state_rows(dt_code(dst.dtype), S, row, src.stride(0) if S > 1 else row,
                                                dst.stride(0) if S > 1 else row, ctypes.c_void_p(src.data_ptr()),
                                                ctypes.c_void_p(dst.data_ptr()), self._p(reset), self._stream()))
        return dst

    def stream_state_rows_at(self, src, dst, lengths):
        """dst[s] = src[s, lengths[s] - 1] where lengths[s] > 0, dst[s] kept otherwise: src [S, T, ...] (a scan's per-frame
        states; each frame contiguous), dst [S, ...], lengths int32 [>= S] on
        the device -- the commit of a ragged EVEStream step."""
        S, T = src.shape[:2]
        assert tuple(dst.shape) == (S,) + tuple(src.shape[2:]) and src.dtype == dst.dtype and src.is_cuda and dst.is_cuda and S > 0
        row = dst[0].numel()
        assert src[0, 0].is_contiguous() and dst[0].is_contiguous(), 'stream_state_rows_at: rows must be contiguous'
        fs, ss = src.stride(1) if T > 1 else row, src.stride(0) if S > 1 else row
        assert fs >= row and ss >= row and (S == 1 or dst.stride(0) >= row), 'stream_state_rows_at: strides'
        assert lengths.dtype == torch.int32 and lengths.is_contiguous() and lengths.numel() >= S and lengths.is_cuda
        self._ck(self.lib.eve_stream_state_rows_at(dt_code(dst.dtype), S, T, row, fs, ss, dst.stride(0) if S > 1 else row,
                                                   ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()),
                                                   self._p(lengths), self._stream()))
        return dst

    def stream_mask_plan(self, B, T, mask=None, pose_valid=None, lengths=None, device=None):
        """The plan of a masked EVEStream step, one launch: mask, pose_valid uint8 or bool [B, T, 2] (left, right) or None,
        lengths int32 [2B] (the ragged layout) or None, all on the device.  -> dict: count int32 [3B], perm, inv int32 [3B, T] --
        the 2B eye sequences (left rows, then right rows), then the B frame sequences; perm lists a sequence's usable frames
        ascending and then the others -- and eye_valid [B, T, 2], valid [B, T] uint8 (include/eve_hip.h eve_stream_mask_plan)."""
        given = [t for t in (mask, pose_valid, lengths) if t is not None]
        device = given[0].device if given else device
        for t in (mask, pose_valid):
            assert t is None or (t.dtype in (torch.uint8, torch.bool) and tuple(t.shape) == (B, T, 2) and t.is_cuda)
        assert lengths is None or (lengths.dtype == torch.int32 and lengths.numel() >= 2 * B and lengths.is_cuda)
        new = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)
        plan = {'count': new((3 * B,), torch.int32), 'perm': new((3 * B, T), torch.int32), 'inv': new((3 * B, T), torch.int32),
                'eye_valid': new((B, T, 2), torch.uint8), 'valid': new((B, T), torch.uint8)}
        self._ck(self.lib.eve_stream_mask_plan(B, T, self._p(mask), self._p(pose_valid), self._p(lengths), self._p(plan['count']),
                                               self._p(plan['perm']), self._p(plan['inv']), self._p(plan['eye_valid']),
                                               self._p(plan['valid']), self._stream()))
        return plan

    def stream_permute_rows(self, src, index):
        """-> dst [S, T, ...] dense with dst[s, j] = src[s, index[s, j]]: src [S, T, ...] whose frames are contiguous (the frame
        and sequence strides are free: a view into wider rows, a scan's output), index int32 [S, T] on the device (a plan's perm
        or inv; clamped to 0..T-1 by the kernel).  A frame holds a multiple of 4 bytes."""
        S, T = src.shape[:2]
        assert src.is_cuda and S > 0 and T > 0 and (src.dim() == 2 or src[0, 0].is_contiguous()), 'stream_permute_rows: rows must be contiguous'
        assert index.dtype == torch.int32 and tuple(index.shape) == (S, T) and index.is_cuda
        es = src.element_size()
        row = src[0, 0].numel() * es
        fs, ss = src.stride(1) * es if T > 1 else row, src.stride(0) * es if S > 1 else row
        dst = torch.empty(src.shape, dtype=src.dtype, device=src.device)
        self._ck(self.lib.eve_stream_permute_rows(S, T, row, fs, ss, ctypes.c_void_p(src.data_ptr()), self._p(dst), self._p(index),
                                                  self._stream()))
        return dst

    def cgru_gates1(self, g1, h):
        C = h.shape[-1]
        P = h.numel() // C
        ru = torch.empty_like(g1)
        rh = torch.empty_like(h)
        self._ck(self.lib.eve_cgru_gates1(dt_code(h.dtype), P, C, self._p(g1), self._p(h), self._p(ru),
                                          self._p(rh), self._stream()))
        return ru, rh

    def cgru_gates2(self, g2, ru, h):
        C = h.shape[-1]
        P = h.numel() // C
        o = torch.empty_like(h)
        hnew = torch.empty_like(h)
        self._ck(self.lib.eve_cgru_gates2(dt_code(h.dtype), P, C, self._p(g2), self._p(ru), self._p(h),
                                          self._p(o), self._p(hnew), self._stream()))
        return o, hnew

    def cgru_gates2_bwd(self, dhnew, ru, h, o):
        C = h.shape[-1]
        P = h.numel() // C
        dg2 = torch.empty_like(h)
        dru = torch.empty_like(ru)
        dh = torch.empty_like(h)
        self._ck(self.lib.eve_cgru_gates2_bwd(dt_code(h.dtype), P, C, self._p(dhnew), self._p(ru), self._p(h),
                                              self._p(o), self._p(dg2), self._p(dru), self._p(dh),
                                              self._stream()))
        return dg2, dru, dh

    def cgru_gates1_bwd(self, drh, dru, ru, h):
        C = h.shape[-1]
        P = h.numel() // C
        dg1 = torch.empty_like(ru)
        dh = torch.empty_like(h)
        self._ck(self.lib.eve_cgru_gates1_bwd(dt_code(h.dtype), P, C, self._p(drh), self._p(dru), self._p(ru),
                                              self._p(h), self._p(dg1), self._p(dh), self._stream()))
        return dg1, dh

    def clstm_gates_fwd(self, gates, c_prev):
        C = c_prev.shape[-1]
        P = c_prev.numel() // C
        h = torch.empty_like(c_prev)
        c = torch.empty_like(c_prev)
        self._ck(self.lib.eve_clstm_gates_fwd(dt_code(c_prev.dtype), P, C, self._p(gates), self._p(c_prev),
                                              self._p(h), self._p(c), self._stream()))
        return h, c

    def clstm_gates_bwd(self, dh, dc_in, gates, c_prev):
        """Adjoint of clstm_gates_fwd: (dgates [.., 4C] w.r.t. the pre-activations, dc_prev [.., C]); dc_in may be None."""
        C = c_prev.shape[-1]
        P = c_prev.numel() // C
        dgates = torch.empty_like(gates)
        dc_prev = torch.empty_like(c_prev)
        self._ck(self.lib.eve_clstm_gates_bwd(dt_code(c_prev.dtype), P, C, self._p(dh), self._p(dc_in), self._p(gates),
                                              self._p(c_prev), self._p(dgates), self._p(dc_prev), self._stream()))
        return dgates, dc_prev

    # ------------------------------------------------------------------ optimiser
    # ------------------------------------------------------------------ masked [B, T, D] loss / metric terms, batched
    VEC_KINDS = {'mse': 0, 'euclidean': 1, 'l1': 2, 'angular': 3}

    def vector_terms(self, items, want_grad):
        """items: list of (kind, pred [B, T(, D)], target, validity [B, T]) float32 / bool on the GPU; want_grad: per item, whether
        d term / d pred is wanted (not for 'euclidean').  ONE launch per 32 terms -> (out [n] float32, [dpred or None])."""
        B, T = items[0][3].shape
        dev = items[0][1].device
        out = torch.empty((len(items),), dtype=torch.float32, device=dev)
        keep, dps, recs = [], [], []
        for (kind, pred, tgt, val), wg in zip(items, want_grad):
            D = 1 if pred.dim() == 2 else pred.shape[2]
            pred, tgt = pred.contiguous(), tgt.contiguous()
            val = val.contiguous()
            val = val.view(torch.uint8) if val.dtype == torch.bool else val.to(torch.uint8)
            assert pred.dtype == tgt.dtype == torch.float32 and tuple(pred.shape) == tuple(tgt.shape) and tuple(val.shape) == (B, T)
            assert tuple(pred.shape[:2]) == (B, T) and 1 <= D <= 3 and pred.dim() <= 3
            dp = torch.empty_like(pred) if wg else None
            keep.append((pred, tgt, val))
            dps.append(dp)
            recs.append(_lib.VecTerm(self._p(pred), self._p(tgt), self._p(val), self._p(dp), D, self.VEC_KINDS[kind]))
        for i in range(0, len(recs), _lib.VEC_TERMS_MAX):
            chunk = recs[i:i + _lib.VEC_TERMS_MAX]
            arr = (_lib.VecTerm * len(chunk))(*chunk)
            self._ck(self.lib.eve_vector_terms(arr, len(chunk), B, T, ctypes.c_void_p(out.data_ptr() + 4 * i), self._stream()))
        return out, dps

    # ------------------------------------------------------------------ stream gates (parallel.GradSync)
    def gate_signal(self, flags, index):
        """One-thread kernel on the current stream (capturable): release, then flags[index] += 1."""
        assert flags.dtype == torch.int32 and flags.is_contiguous() and 0 <= index < flags.numel()
        self._ck(self.lib.eve_gate_signal(ctypes.c_void_p(flags.data_ptr() + 4 * index), self._stream()))

    def gate_wait(self, flags, index, value, timeouts, value_index=None, poison=None, max_polls=0):
        """One-wave kernel on the current stream that returns once flags[index] has reached `value` -- or flags[value_index],
        read on the device, when value_index is given (a capturable wait: the target is not baked into the node).  Bounded poll
        (max_polls; 0 = eve_dispatch_config.gate_wait_polls, seconds): a gate that never opens increments timeouts[0] and writes
        +inf to poison[0] (a float32 tensor inside the last all-reduced gradient bucket: adam_step(poison=...) then skips the
        update on every rank) instead of hanging the device."""
        assert flags.dtype == timeouts.dtype == torch.int32 and 0 <= index < flags.numel()
        assert poison is None or (poison.dtype == torch.float32 and poison.numel() >= 1)
        ref = None if value_index is None else ctypes.c_void_p(flags.data_ptr() + 4 * value_index)
        self._ck(self.lib.eve_gate_wait(ctypes.c_void_p(flags.data_ptr() + 4 * index), int(value) & 0xffffffff, ref, self._p(timeouts),
                                        self._p(poison), int(max_polls), self._stream()))

    SUMSQ_WORKSPACE = 1024          # include/eve_hip.h EVE_SUMSQ_WORKSPACE

    def sumsq(self, g, out, workspace=None):
        """out[0] += sum g^2, in a fixed summation order (bit-reproducible).  workspace: float32 [1024] scratch."""
        if workspace is None:
            workspace = torch.empty((self.SUMSQ_WORKSPACE,), dtype=torch.float32, device=g.device)
        assert workspace.numel() >= self.SUMSQ_WORKSPACE and workspace.dtype == torch.float32
        self._ck(self.lib.eve_sumsq(g.numel(), self._p(self._f32(g, 'g')), self._p(out), self._p(workspace), self._stream()))
        return out

    ADAM_GUARD_WORDS = 12        # include/eve_hip.h eve_adam_guard: 4 ints, then floats (loss_scale at word 4), skipped_gate (int) at word 9

    @staticmethod
    def new_adam_guard(device, loss_scale=1.0, step=0):
        """Device-resident optimiser state (eve_adam_guard) as an int32 tensor of 12 words; .view(torch.float32)[4] is the loss scale."""
        g = torch.zeros(HipKernels.ADAM_GUARD_WORDS, dtype=torch.int32, device=device)
        g[0] = int(step)
        g.view(torch.float32)[4] = float(loss_scale)
        return g

    def adam_step(self, p, g, m, v, sumsq, max_norm, gscale, lr, beta1, beta2, eps, weight_decay, step,
                  guard=None, check_finite=False, lr_dev=None, poison=None):
        """poison: float32 device word (gate_wait writes +inf there on a time-out); non-zero skips the step on the device."""
        if guard is not None:
            assert guard.dtype == torch.int32 and guard.numel() >= self.ADAM_GUARD_WORDS and guard.is_contiguous()
        assert poison is None or (guard is not None and poison.dtype == torch.float32)
        self._ck(self.lib.eve_adam_step(p.numel(), self._p(p), self._p(g), self._p(m), self._p(v),
                                        self._p(sumsq), max_norm, gscale, lr, beta1, beta2, eps,
                                        weight_decay, step, self._p(guard), 1 if check_finite else 0, self._p(lr_dev), self._p(poison),
                                        self._stream()))


def dispatch_flag(k, name, default):
    """Field `name` of k's kernel-selection table (include/eve_hip.h eve_dispatch_config: resolved once when the library is
    loaded, overridden only through eve_set_dispatch_config); `default` for a test stand-in that has no table."""
    if hasattr(k, 'dispatch_config'):
        return int(getattr(k.dispatch_config(), name))
    return default


_default = None


def default_kernels():
    """The process-wide HipKernels; raises (no fallback) if libeve_hip.so is not built."""
    global _default
    if _default is None:
        _default = HipKernels()
    return _default


def set_default_kernels(k):
    """Test hook: tests/ installs a torch-CPU stand-in to exercise the HOST logic without a GPU."""
    global _default
    _default = k
